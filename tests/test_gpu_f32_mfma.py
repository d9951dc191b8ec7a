"""The float-row matcher's bf16 MFMA prefilter (csrc/fm3d_match.hip, knn2_bf16_kernel + recheck):
knnMatch(k = 2) of SURF-type float descriptors (descriptorsmatcher.cpp:89-131) must return exactly
what the full FLANN-order scan returns -- the same two train rows per query, lowest index on equal
distances, bit-identical float distances -- against the oracle and against the VALU scan of the
same library (FM3D_F32_MFMA=0).  The prefilter serves calls with nA * nB >= 2^22 at dim 64 / 128."""
import os

import numpy as np
import pytest

import f32_prefilter_pyref as pf
from conftest import oracle_threads

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx(fm3d):
    c = fm3d.Context(fm3d.Settings.default())
    yield c
    c.close()


def _knn(dm, A, B, **env):
    for k, v in env.items():
        os.environ[k] = v
    try:
        return dm.knn_match(A, B)
    finally:
        for k in env:
            del os.environ[k]


def _check(fm3d, orc, ctx, A, B, eps=0.7):
    """the fused prefilter (default), the two-pass prefilter (FM3D_F32_FUSED=0) and the VALU scan
    (FM3D_F32_MFMA=0) byte-identical, and equal to the oracle"""
    dm = fm3d.DescriptorsMatcher(ctx)
    got = dm.knn_match(A, B)
    assert got.tobytes() == _knn(dm, A, B, FM3D_F32_FUSED="0").tobytes()
    ref = _knn(dm, A, B, FM3D_F32_MFMA="0")
    assert got.tobytes() == ref.tobytes()
    idx, dist = orc.knn2(A, B, orc.F32, oracle_threads())
    assert np.array_equal(got["trainIdx"], idx)
    ok = idx >= 0
    assert np.array_equal(got["distance"][ok], dist[ok])
    m = dm.compareWithNNDR(eps, A, B)
    q, t, d = orc.nndr(idx, dist, eps)
    assert np.array_equal(m["queryIdx"], q) and np.array_equal(m["trainIdx"], t) and np.array_equal(m["distance"], d)


@pytest.mark.parametrize("dim", [128, 64])
def test_f32_mfma_surf_descriptors(fm3d, orc, synth, ctx, dim):
    """SURF descriptors of the synthetic frames (unit rows), extended and not"""
    fp = synth.make_frame_pair(4000, seed=3)
    s = fm3d.Settings.default()
    s.surfExtended = 1 if dim == 128 else 0
    c = fm3d.Context(s)
    try:
        _, da = fm3d.SURF(c).detect(fp.img1, with_descriptors=True)
        _, db = fm3d.SURF(c).detect(fp.img2, with_descriptors=True)
    finally:
        c.close()
    assert da.shape[1] == dim and len(da) * len(db) >= 1 << 22
    _check(fm3d, orc, ctx, da, db)


@pytest.mark.parametrize("dim,nA,nB", [(128, 3000, 9000), (64, 2500, 12000)])
def test_f32_mfma_random_rows(fm3d, orc, ctx, dim, nA, nB):
    """near neighbours among clutter, un-normalised rows of varied length"""
    rng = np.random.default_rng(dim + nA)
    B = (rng.normal(0, 1, (nB, dim)) * rng.uniform(0.2, 3, (nB, 1))).astype(np.float32)
    A = np.concatenate([B[: nA // 2] + rng.normal(0, 0.05, (nA // 2, dim)),
                        rng.normal(0, 1, (nA - nA // 2, dim))]).astype(np.float32)
    _check(fm3d, orc, ctx, A, B)


def test_f32_mfma_ties_and_duplicates(fm3d, orc, ctx):
    """exact duplicates among the train rows (equal distances: the lowest index first), queries equal
    to train rows (distance 0), many rows inside the prefilter's bound (more than either candidate
    list holds: those queries are rescanned)"""
    rng = np.random.default_rng(7)
    B = rng.normal(0, 0.1, (4096, 128)).astype(np.float32)
    B[2000] = B[17]
    B[3000] = B[17]
    B[100:300] = B[99]  # 201 identical rows: one query's bound holds them all
    A = np.concatenate([B[17:18], B[99:100], B[:1500], rng.normal(0, 0.1, (1000, 128))]).astype(np.float32)
    _check(fm3d, orc, ctx, A, B)
    got = fm3d.DescriptorsMatcher(ctx).knn_match(A, B)
    assert list(got["trainIdx"][0]) == [17, 2000] and list(got["trainIdx"][1]) == [99, 100]


def test_f32_mfma_nonfinite_rows_rescanned(fm3d, orc, ctx):
    """a NaN / inf in the train rows voids the prefilter's bound: every query takes the exact rescan"""
    rng = np.random.default_rng(8)
    B = rng.normal(0, 0.1, (3000, 64)).astype(np.float32)
    A = rng.normal(0, 0.1, (1500, 64)).astype(np.float32)
    B[5, 3] = np.inf
    dm = fm3d.DescriptorsMatcher(ctx)
    got = dm.knn_match(A, B)
    assert got.tobytes() == _knn(dm, A, B, FM3D_F32_FUSED="0").tobytes()
    assert got.tobytes() == _knn(dm, A, B, FM3D_F32_MFMA="0").tobytes()


# ---------------------------------------------------------------- the bound's error model and the routes
# (inputs and their expected list lengths: tests/f32_prefilter_pyref.py, tests/test_f32_prefilter_bound.py)
NA, NB = 2048, 2051  # the smallest calls that take the prefilter: 2^22 pairs, a partial last tile, 4 train parts


@pytest.mark.parametrize("dim", [128, 64])
def test_f32_mfma_correlated_bf16_rounding(fm3d, orc, ctx, dim):
    """triples whose bf16 rounding errors all push the same way: |s' - s| reaches 0.00996 |a| B_max, and
    a bound built on 2^-9 per element (0.0079 |a| B_max) drops the exact nearest row b* (with that
    coefficient the library returned the two decoys, e.g. rows [2049, 2050] for query 0 where the exact
    scan returns [0, 2049]: 11 of the 12 queries at dim 128, all 12 at dim 64)"""
    A, B, queries, rows = pf.correlated_rounding_case(dim, NA, NB, 12, seed=dim)
    dm = fm3d.DescriptorsMatcher(ctx)
    for env in ({}, {"FM3D_F32_FUSED": "0"}):
        got = _knn(dm, A, B, **env)["trainIdx"][queries]
        print("dim", dim, env, "query", int(queries[0]), "got", got[0].tolist(), "want", rows[0, :2].tolist(),
              "| queries off:", queries[(got != rows[:, :2]).any(axis=1)].tolist())
        assert np.array_equal(got, rows[:, :2])
    _check(fm3d, orc, ctx, A, B)


def test_f32_mfma_retry_route(fm3d, orc, ctx):
    """|b_j|^2 strictly decreasing, a quarter of the queries tiny: their fused lists overflow (every
    row a running best), the two-pass retry lists two rows for each"""
    A, B, nTiny = pf.retry_route_case(128, NA, NB, seed=21)
    _check(fm3d, orc, ctx, A, B)
    got = fm3d.DescriptorsMatcher(ctx).knn_match(A, B)
    assert np.all(got["trainIdx"][:nTiny] >= 0)


def _duplicates(fm3d, orc, ctx, share):
    A, B, dupq, top2 = pf.duplicates_case(128, NA, NB, share, seed=share)
    _check(fm3d, orc, ctx, A, B)
    got = fm3d.DescriptorsMatcher(ctx).knn_match(A, B)
    assert np.array_equal(got["trainIdx"][dupq], top2)


def test_f32_mfma_rescan_route(fm3d, orc, ctx):
    """140 copies of the nearest row of 1/16 of the queries, over all tiles and parts: the fused pass
    keeps its lists and the rescan kernel serves those queries (lowest two copies, equal distances)"""
    _duplicates(fm3d, orc, ctx, 16)


def test_f32_mfma_valu_fallback_route(fm3d, orc, ctx):
    """the same for 1/4 of the queries: both forms break the 1/8 rule and the call ends on the VALU scan"""
    _duplicates(fm3d, orc, ctx, 4)


@pytest.fixture(scope="module")
def magnitudes():
    return pf.magnitude_cases(128, NA, NB, seed=31)


@pytest.mark.parametrize("case", ["tiny", "large", "huge_query", "outlier_row", "bf16_inf"])
def test_f32_mfma_magnitudes(fm3d, orc, ctx, magnitudes, case):
    """the problem scaled by 1e-12 (norms under the 1e-10 rescan threshold) and by 1e15, queries of norm
    2e18 and 2e19 (|a| >= 1e18; the larger one's fp32 norm overflows), a train row of norm 1e6 among
    unit rows (the margin swallows every row), a finite fp32 element that is +inf in bf16"""
    A, B = magnitudes[case]
    _check(fm3d, orc, ctx, A, B)
