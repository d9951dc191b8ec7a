"""The error model of the float matcher's bf16 prefilter (csrc/fm3d_match.hip, DESIGN.md §"f32 with
the bf16 MFMA prefilter"), pinned on the CPU with the numpy emulation of tests/f32_prefilter_pyref.py.

The prefilter ranks train row j for query a by s'_j = |b_j|^2 - 2 bf16(a).bf16(b_j) and keeps the rows
under s'_(2) + 2 eps_q + 2 phi_q + slack, eps_q = C |a| B_max + 1e-5 B_max^2.  C is derived, not fitted:

    bf16 keeps 8 significand bits: round-to-nearest moves an element by at most u = 2^-8 relative;
    a product of two rounded elements is off by at most 2u + u^2 relative, so by Cauchy-Schwarz
    |bf16(a).bf16(b) - a.b| <= (2u + u^2) |a||b|, and the key carries twice the dot product:
        2 (2u + u^2)                                   = 0.0156555...
    the dot's fp32 accumulation, dim <= 128 roundings of 2^-24 each, again doubled:
        2 * 128 * 2^-24 = 2^-16                        = 0.0000153
    sum 0.0156708, rounded up:                       C = 0.0158

The parent's coefficient 0.0079 assumed 2^-9 per element, half of u.  The tests below show that (1) the
adversarial input of correlated_rounding_case separates the two constants without trusting the library,
(2) that input's candidate lists keep it away from the exact rescan and the VALU scan, so no fallback
route can hide a wrong constant on the GPU, (3) the worst case really approaches 2 (2u + u^2), and (4) the route inputs of the GPU tests
(tests/test_gpu_f32_mfma.py) produce the list lengths that send them down the intended routes."""
import functools

import numpy as np
import pytest

import f32_prefilter_pyref as pf
from conftest import oracle_threads

U = 2.0 ** -8
C_EXACT = 2 * (2 * U + U * U) + 2 * 128 * 2.0 ** -24
C = 0.0158       # C_EXACT rounded up: the library's kBf16KeyCoef
C_PARENT = 0.0079
NA, NB, K = 2048, 2051, 12


def test_coefficient_derivation():
    assert 0.01567 < C_EXACT <= C < C_EXACT * 1.01 and C >= 2 * C_PARENT


@functools.lru_cache(maxsize=None)
def adversarial(dim):
    A, B, queries, rows = pf.correlated_rounding_case(dim, NA, NB, K, seed=dim)
    for x in (A, B, queries, rows):
        x.setflags(write=False)
    return A, B, queries, rows


@functools.lru_cache(maxsize=None)
def adversarial_lists(dim, c):
    A, B, _, _ = adversarial(dim)
    return pf.final_lists(A, B, c)


def test_generator_placements():
    """the triples cover row 0 of tile 0, the last two rows, one tile's blocks, the parts, both halves"""
    _, B, queries, rows = adversarial(128)
    assert rows.shape == (K, 3) and len(np.unique(rows)) == 3 * K and len(np.unique(queries)) == K
    assert np.all(rows[:, 1] < rows[:, 2]) and np.array_equal(B[rows[:, 1]], B[rows[:, 2]])
    assert rows[0, 0] == 0 and list(rows[0, 1:]) == [NB - 2, NB - 1] and NB % pf.K_T >= 2
    assert len({int(r) // pf.K_T for r in rows[1]}) == 1 and len({int(r) % pf.K_T // 32 for r in rows[1]}) == 3
    parts, _ = pf.part_tiles(NA, NB)
    assert parts >= 3 and len(set(pf.row_part(rows[2], NA, NB).tolist())) == 3
    assert set(pf.row_part(rows.ravel(), NA, NB).tolist()) == set(range(parts))
    assert set(pf.row_half(rows.ravel()).tolist()) == {0, 1}
    assert queries[0] == 0 and queries[-1] == NA - 1
    # the special rows set B_max
    n2 = pf.norms2_f32(B)
    assert int(np.argmax(n2)) in rows[:, 1:] and n2[np.setdiff1d(np.arange(NB), rows.ravel())].max() < n2[rows].min()


@pytest.mark.parametrize("dim", [128, 64])
def test_generator_is_discriminating(orc, dim):
    """the oracle's exact top-2 of every adversarial query is (b*, lower decoy); that pair leaves the
    parent's bound and every query's exact top-2 lies inside the derived one"""
    A, B, queries, rows = adversarial(dim)
    idx, dist = orc.knn2(A, B, orc.F32, oracle_threads())
    assert np.array_equal(idx[queries], rows[:, :2])
    assert np.all(dist[queries, 0] < dist[queries, 1])  # b* is strictly nearer in FLANN's fp32
    old = adversarial_lists(dim, C_PARENT)
    new = adversarial_lists(dim, C)
    lost = [q for q in range(NA) if not np.isin(idx[q], old[q]).all()]
    assert lost == queries.tolist()  # the adversarial queries and no other
    for i, q in enumerate(queries):
        assert rows[i, 0] not in old[q] and rows[i, 1] in old[q] and rows[i, 2] in old[q]
    assert all(np.isin(idx[q], new[q]).all() for q in range(NA))
    # the per-row error of the triples alone exceeds the parent's coefficient
    err = np.abs(pf.prefilter_keys(A[queries], B) - pf.exact_keys(A[queries], B))
    a = np.sqrt(pf.norms2_f32(A[queries]).astype(np.float64))
    bmax = np.sqrt(float(pf.norms2_f32(B).max()))
    ratio = err[np.arange(K), rows[:, 1]] / (a * bmax)
    print("dim", dim, "decoy |s'-s| / (|a| Bmax):", ratio.min(), ratio.max())
    assert np.all(ratio > C_PARENT) and np.all(ratio <= C)


@pytest.mark.parametrize("dim", [128, 64])
def test_no_fallback_hides_a_failure(dim):
    """No adversarial query of the GPU run may reach the exact rescan or the VALU scan, which would
    return the right rows whatever the constant.  Under both constants every final list fits kCandMax
    (longest: 14 and 28 at dim 128, 11 and 19 at dim 64), so the two-pass form rescans nothing.

    The fused lists cannot all fit kCandMax2 at this shape, whatever the rows: 2048 x 2051 runs as
    4 train parts x 2 half-waves = 8 lane streams of ~256 rows, each emits its first two rows and
    every later row that is among its two smallest so far (2 / n of the time), 8 * 11.2 = 90 rows on
    average before the margin adds any, and the longest of 2048 such lists passes 128 (modelled
    longest: 144 and 184 at dim 128, 138 and 167 at dim 64).  What keeps the fallback out is the 1/8
    rule: under C more than nA / 8 lists overflow (1674 at dim 128, 739 at dim 64), the host drops
    the fused pass for the two-pass form and nothing is rescanned.  Under the parent's coefficient
    few overflow (129 and 13), the fused form stands, and all adversarial queries but one (dim 128)
    keep their lists, so both forms lose b* there."""
    A, B, queries, _ = adversarial(dim)
    for c in (C_PARENT, C):
        final = max(len(l) for l in adversarial_lists(dim, c))
        fused = pf.fused_list_lengths(A, B, c)
        over = int((fused > pf.K_CAND_MAX2).sum())
        print("dim", dim, "c", c, "longest final list", final, "longest fused list", int(fused.max()), "fused lists over",
              pf.K_CAND_MAX2, ":", over, "adversarial:", fused[queries].tolist())
        assert final <= pf.K_CAND_MAX
        if c == C:  # the call ends on the two-pass form (or no list overflows): no rescan
            assert over == 0 or over > NA // 8
        else:       # the fused form stands and serves (nearly) every adversarial query from its lists
            assert over <= NA // 8 and (fused[queries] <= pf.K_CAND_MAX2).sum() >= K - 1


@pytest.mark.parametrize("above", [False, True], ids=["below-tie", "above-tie"])
@pytest.mark.parametrize("dim", [128, 64])
def test_aligned_family_approaches_the_bound(dim, above):
    """a parallel to b, every element next to a bf16 tie: |s' - s| / (|a||b|) comes within 1 % of
    2 (2u + u^2) and stays under C -- the coefficient is the derived one, not 'twice the old number'"""
    A, B = pf.aligned_case(dim, above, seed=dim + above)
    err = abs(pf.prefilter_keys(A, B)[0, 0] - pf.exact_keys(A, B)[0, 0])
    ratio = err / float(np.sqrt((A.astype(np.float64) ** 2).sum() * (B.astype(np.float64) ** 2).sum()))
    print("dim", dim, "above" if above else "below", "|s'-s| / (|a||b|) =", ratio)
    assert 0.015 < ratio <= C and ratio > 2 * C_PARENT * 0.98
    assert ratio <= 2 * (2 * U + U * U)


def test_bf16_rne_ties_and_overflow():
    x = np.array([1 + 2.0 ** -8, 1 + 3 * 2.0 ** -8, 1 + 2.0 ** -8 - 2.0 ** -12, 1 + 2.0 ** -8 + 2.0 ** -12, -1.5,
                  3.4e38, 3.39e38], dtype=np.float32)
    want = np.array([1.0, 1 + 2.0 ** -6, 1.0, 1 + 2.0 ** -7, -1.5, np.inf, 255 * 2.0 ** 120], dtype=np.float32)
    assert np.array_equal(pf.bf16_rne(x), want)  # ties to even; the largest floats round to +inf


# ---------------------------------------------------------------- the route inputs of the GPU tests
def test_retry_route_lists():
    """|b_j|^2 falls by more than a tiny query's margin per row: the tiny queries' fused lists overflow
    (every row is a running best) while their final lists hold two rows -> the two-pass retry serves
    the call and nothing is rescanned"""
    A, B, nTiny = pf.retry_route_case(128, NA, NB, seed=21)
    n2 = pf.norms2_f32(B).astype(np.float64)
    m = pf.margin(A, B, C)
    a = np.sqrt(pf.norms2_f32(A[:nTiny]).astype(np.float64))
    assert nTiny >= NA / 4 and np.all(a + np.sqrt(n2.max()) > 1e-10) and np.all(a < 1e-5) and np.all(np.isfinite(m))
    assert np.all(n2[:-1] - n2[1:] > m[:nTiny].max())
    fused = pf.fused_list_lengths(A, B, C)
    final = np.array([len(l) for l in pf.final_lists(A, B, C)])
    print("tiny queries: fused", fused[:nTiny].min(), "final", final[:nTiny].max(), "| others: fused",
          fused[nTiny:].max(), "final", final[nTiny:].max())
    assert np.all(fused[:nTiny] > pf.K_CAND_MAX2) and (fused > pf.K_CAND_MAX2).sum() > NA // 8
    assert np.all(final[:nTiny] == 2) and np.all(final <= pf.K_CAND_MAX)


@pytest.mark.parametrize("share,route", [(16, "rescan"), (4, "valu")])
def test_duplicate_rows_lists(share, route):
    """140 copies of a query's nearest row overflow both lists; at a 1/16 share the fused pass keeps
    its lists and the rescan kernel serves those queries, at 1/4 both forms break the 1/8 rule"""
    A, B, dupq, top2 = pf.duplicates_case(128, NA, NB, share, seed=share)
    fused = pf.fused_list_lengths(A, B, C)
    final = np.array([len(l) for l in pf.final_lists(A, B, C)])
    assert len(dupq) == NA // share and np.all(top2[:, 0] < top2[:, 1])
    assert np.all(final[dupq] >= 140) and np.all(fused[dupq] > pf.K_CAND_MAX2)
    rest = np.setdiff1d(np.arange(NA), dupq)
    assert np.all(final[rest] <= pf.K_CAND_MAX) and np.all(fused[rest] <= pf.K_CAND_MAX2)
    spread = pf.final_lists(A[dupq[:1]], B, C)[0]
    assert len(set((spread // pf.K_T).tolist())) > 8 and len(set(pf.row_part(spread, NA, NB).tolist())) == pf.part_tiles(NA, NB)[0]
    over = int((fused > pf.K_CAND_MAX2).sum())
    assert (0 < over <= NA // 8) if route == "rescan" else (over > NA // 8 and (final > pf.K_CAND_MAX).sum() > NA // 8)


def test_magnitude_cases_margins():
    """which queries the bound covers at each magnitude"""
    cases = pf.magnitude_cases(128, NA, NB, seed=31)
    ok = {k: np.isfinite(pf.margin(a, b, C)) for k, (a, b) in cases.items()}
    assert not ok["tiny"].any()                       # |a| + B_max <= 1e-10
    assert ok["large"].all()
    bad = np.flatnonzero(~ok["huge_query"])
    assert list(bad) == [5, 700]
    a, b = cases["huge_query"]
    assert np.isinf(pf.norms2_f32(a)[5]) and np.isfinite(pf.norms2_f32(a)[700]) and pf.norms2_f32(a)[700] >= 1e36
    a, b = cases["outlier_row"]
    assert ok["outlier_row"].all() and min(len(l) for l in pf.final_lists(a[:64], b, C)) == NB - 1  # every unit row
    a, b = cases["bf16_inf"]
    assert np.isfinite(b).all() and np.isinf(pf.bf16_rne(b)).sum() == 1 and not ok["bf16_inf"].any()
