"""3D-3D alignment on the GPU: fm3d_align_points and fm3d_match_models against the
plain-Python restatement (tests/align_pyref.py) -- every hypothesis's model and count, the best, the
rounds of the refit, the final transform, its mask and the compacted inliers, bit for bit -- over the
shapes at which the kernels take another path, the edge cases of the predicate and the argument rules.
No case provokes a fault: every index is validated on the host, and the NaN cases are data."""
import ctypes
import math

import numpy as np
import pytest

import align_pyref as ref

pytestmark = pytest.mark.gpu

MAX_DIST = 0.005


@pytest.fixture(scope="module")
def ctx(fm3d):
    c = fm3d.Context(fm3d.Settings.default(), device=0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def big():
    """the quality recipe at 1,800 points: the shapes' inputs"""
    return ref.model_pair(N=1800)


def run_both(fm3d, orc, ctx, p, m, H, seed, refine=0, normals=False, min_cos=0.9, max_dist=MAX_DIST):
    """(the library's debug result, the restatement's) on the same inputs"""
    na, nb = (p["nA"], p["nB"]) if normals else (None, None)
    got = fm3d.ModelAligner(ctx).align(p["A"], p["B"], m, max_dist, na, nb, min_cos, hypotheses=H, seed=seed,
                                       refine=refine, debug=True)
    return got, ref.align(orc, p["A"], p["B"], m, max_dist, H, seed, refine, na, nb, min_cos)


def assert_same(fm3d, got, want, m):
    g, mask, inl, best, counts, models = got[:6]
    assert np.array_equal(counts, want["counts"])
    assert np.array_equal(models, want["models"])
    assert best == want["best"]
    assert np.array_equal(g, want["g"])
    assert np.array_equal(mask, want["mask"])
    assert inl.tobytes() == np.ascontiguousarray(np.asarray(m)[want["mask"]], dtype=fm3d.DMATCH).tobytes()
    if len(got) > 6:
        rc, rm, adopted = got[6:]
        assert np.array_equal(rc, want["roundCounts"]) and np.array_equal(rm, want["roundModels"])
        assert adopted == want["adopted"]


# ---------------------------------------------------------------- shapes
@pytest.mark.parametrize("normals", [False, True])
@pytest.mark.parametrize("M", [2, 3, 4, 63, 64, 65, 257, 1025, 1800])
@pytest.mark.parametrize("H", [1, 5, 64, 257])
def test_shapes(fm3d, orc, ctx, big, M, H, normals):
    """no model (M = 2), the minimum, partial waves, blocks and tiles; one hypothesis to several chunks;
    both instances of the scoring kernel"""
    m = big["matches"][:M]
    got, want = run_both(fm3d, orc, ctx, big, m, H, 0, normals=normals)
    assert_same(fm3d, got, want, m)
    if M < 3:
        assert got[3] == -1 and not got[0].any() and not got[1].any() and len(got[2]) == 0 and (got[4] == -1).all()
    if M >= 257 and H >= 64:
        assert got[3] >= 0 and got[1][big["true"][:M]].sum() >= 0.99 * big["true"][:M].sum()
        assert np.array_equal(got[0][3], [0, 0, 0, 1])


def test_normals_are_a_second_test(fm3d, orc, ctx, big):
    """at a loose distance the wrong pairs pass the first test; the normals take them out again"""
    m = big["matches"][:1025]
    loose, want0 = run_both(fm3d, orc, ctx, big, m, 64, 0, max_dist=5.0)
    both, want1 = run_both(fm3d, orc, ctx, big, m, 64, 0, normals=True, min_cos=0.99, max_dist=5.0)
    assert_same(fm3d, loose, want0, m)
    assert_same(fm3d, both, want1, m)
    assert loose[1].all() and int(both[1].sum()) < len(m)


# ---------------------------------------------------------------- the predicate's edges
def boundary_case(orc):
    """200 clean pairs and three more at the threshold, max_dist = 2^-8 (tau2 = 2^-16 exactly): with
    p = R a + t of the best model in the contract's order, b = p -+ (2^-8, 0, 0) (towards zero, so that
    the difference is exact) is at d . d == tau2 exactly, and one ulp of b.x either side of it lies
    inside and outside"""
    p = ref.model_pair(N=203, wrong_frac=0.0, sigma=0.0005)
    md = 2.0 ** -8
    m = p["matches"].copy()
    ext = [200, 201, 202]
    p["B"][m["trainIdx"][ext]] += 100.0  # far off: no sample with one of them wins
    r = ref.align(orc, p["A"], p["B"], m, md, 64, 0)
    assert r["best"] >= 0 and not set(r["ransac"]["samples"][r["best"]]) & set(ext)
    mod = [float(v) for v in r["model"]]
    for k, i in enumerate(ext):
        a = [float(v) for v in p["A"][m["queryIdx"][i]]]
        q = [(ref._rot_row(mod, j, a[0], a[1], a[2]) + mod[9 + j]) for j in range(3)]
        sg = 1.0 if q[0] > 0 else -1.0  # towards zero: the difference is exact
        bx = q[0] - sg * md
        assert abs(q[0]) > 4 * md and abs(q[0] - bx) == md
        bx = [bx, np.nextafter(bx, q[0]), np.nextafter(bx, -sg * math.inf)][k]  # at, inside, outside
        p["B"][m["trainIdx"][i]] = [bx, q[1], q[2]]
    return p, m, md, ext, r["model"]


def test_pair_exactly_at_the_threshold(fm3d, orc, ctx):
    p, m, md, ext, model = boundary_case(orc)
    got, want = run_both(fm3d, orc, ctx, p, m, 64, 0, max_dist=md)
    assert np.array_equal(want["model"], model)  # the three pairs did not change the best model
    assert list(want["mask"][ext]) == [True, True, False]
    assert_same(fm3d, got, want, m)
    assert list(got[1][ext]) == [True, True, False]


def test_nan_point_is_never_an_inlier(fm3d, orc, ctx, big):
    p = dict(big)
    p["A"], p["B"], p["nA"] = big["A"].copy(), big["B"].copy(), big["nA"].copy()
    m = big["matches"][:300]
    true = np.nonzero(big["true"][:300])[0]
    ia, ib, ic = true[:3]
    p["A"][m["queryIdx"][ia], 1] = math.nan
    p["B"][m["trainIdx"][ib], 2] = math.nan
    p["nA"][m["queryIdx"][ic], 0] = math.nan
    for normals in (False, True):
        got, want = run_both(fm3d, orc, ctx, p, m, 64, 0, normals=normals, refine=2)
        assert_same(fm3d, got, want, m)
        assert got[3] >= 0 and not got[1][ia] and not got[1][ib] and got[1][ic] == (not normals)
        assert np.isfinite(got[0]).all() and got[1][true[3:]].all()


def test_duplicate_matches(fm3d, orc, ctx, big):
    """every match three times over: some samples hold one pair twice (a cross matrix of rank 1: invalid,
    or a model of rounding noise that wins nothing), and every copy is counted and kept"""
    m = np.repeat(big["matches"][:100], 3)
    got, want = run_both(fm3d, orc, ctx, big, m, 257, 0, refine=1)
    assert_same(fm3d, got, want, m)
    twice = [h for h, s in enumerate(want["ransac"]["samples"]) if len({i // 3 for i in s}) < 3]
    assert twice and got[3] >= 0 and got[3] not in twice and got[4][twice].max() < got[4][got[3]]
    assert np.array_equal(got[1][0::3], got[1][1::3]) and np.array_equal(got[1][0::3], got[1][2::3])


def test_tie_takes_the_lowest_hypothesis(fm3d, orc, ctx):
    """three exact pairs: every valid hypothesis accepts all three, so the first valid one is the best"""
    p = ref.model_pair(N=3, wrong_frac=0.0, sigma=0.0)
    got, want = run_both(fm3d, orc, ctx, p, p["matches"], 64, 5, max_dist=1e-6)
    assert_same(fm3d, got, want, p["matches"])
    counts = got[4]
    valid = np.nonzero(counts >= 0)[0]
    assert len(valid) >= 32 and (counts[valid] == 3).all() and got[3] == valid[0]
    # four exact pairs, the first one of hypothesis 0's sample made NaN: the hypotheses that draw it are
    # invalid, the others tie at three, and the lowest of those is not hypothesis 0
    p = ref.model_pair(N=4, wrong_frac=0.0, sigma=0.0)
    p["A"][p["matches"]["queryIdx"][ref.sample3(5, 0, 4)[0]]] = math.nan
    got, want = run_both(fm3d, orc, ctx, p, p["matches"], 64, 5, max_dist=1e-6)
    assert_same(fm3d, got, want, p["matches"])
    counts = got[4]
    valid = np.nonzero(counts >= 0)[0]
    assert counts[0] == -1 and len(valid) >= 4 and (counts[valid] == 3).all() and got[3] == valid[0] > 0


def test_seed_determinism(fm3d, ctx, big):
    al = fm3d.ModelAligner(ctx)
    m = big["matches"]
    runs = [al.align(big["A"], big["B"], m, MAX_DIST, hypotheses=257, seed=s, refine=2, debug=True) for s in (3, 3, 4)]
    for x, y in zip(runs[0], runs[1]):
        assert np.asarray(x).tobytes() == np.asarray(y).tobytes()
    assert runs[0][3] != runs[2][3] and not np.array_equal(runs[0][5], runs[2][5])


# ---------------------------------------------------------------- refinement
@pytest.mark.parametrize("normals", [False, True])
@pytest.mark.parametrize("refine", [1, 4, 16])
def test_refine_rounds(fm3d, orc, ctx, big, refine, normals):
    """1,800 matches (two tiles): every round's model and count; codes >= 0 adopted or rejected, -2 not run"""
    m = big["matches"]
    got, want = run_both(fm3d, orc, ctx, big, m, 64, 0, refine=refine, normals=normals)
    assert_same(fm3d, got, want, m)
    rc, rm, adopted = got[6:]
    assert rc.shape == (refine + 1,) and rm.shape == (refine, 12) and 1 <= adopted <= refine
    assert rc[0] == got[4][got[3]] and (rc[1:1 + adopted] >= rc[0]).all()
    ran = int((rc[1:] != -2).sum())
    assert ran in (adopted, adopted + 1) and (rc[1 + ran:] == -2).all() and not rm[ran:].any()
    assert int(got[1].sum()) == rc[adopted]


def test_refine_zero_is_the_unrefined_call(fm3d, ctx, big):
    """refineIters == 0 through the same entry point: byte for byte what the RANSAC alone gives, and
    the rounds' outputs say that none ran"""
    m = big["matches"][:1025]
    al = fm3d.ModelAligner(ctx)
    plain = al.align(big["A"], big["B"], m, MAX_DIST, hypotheses=64, seed=1, debug=True)
    L, o = fm3d.lib(), fm3d.AlignOpts(64, 0, MAX_DIST, 0.0, 1)
    g, mask, out = np.zeros(16), np.zeros(len(m), dtype=np.uint8), np.zeros(len(m), dtype=fm3d.DMATCH)
    n, best, adopted = ctypes.c_int(0), ctypes.c_int(0), ctypes.c_int(99)
    rc = np.full(1, 77, dtype=np.int32)
    vp = lambda a: ctypes.c_void_p(a.ctypes.data)
    mm = np.ascontiguousarray(m)
    assert L.fm3d_align_points(ctx.handle, vp(big["A"]), None, len(big["A"]), vp(big["B"]), None, len(big["B"]), vp(mm),
                               len(mm), ctypes.byref(o), vp(g), vp(mask), vp(out), ctypes.byref(n), ctypes.byref(best),
                               None, None, vp(rc), None, ctypes.byref(adopted)) == 0
    assert np.array_equal(g.reshape(4, 4), plain[0]) and np.array_equal(mask.astype(bool), plain[1])
    assert out[:n.value].tobytes() == plain[2].tobytes() and best.value == plain[3]
    assert adopted.value == 0 and rc[0] == n.value == plain[4][plain[3]]


def rejected_case():
    """Three groups under the identity: 50 exact pairs, 40 shifted by +0.95 max_dist in x and 5 by
    -0.9 max_dist.  A model from exact pairs accepts all 95; its refit moves t towards the 40 and loses
    the 5: fewer pairs, so the round is rejected and the RANSAC's model stays."""
    rng = np.random.default_rng(21)
    A = rng.uniform(-1, 1, (95, 3)) + [0, 0, 2.0]
    B = A.copy()
    B[50:90, 0] += 0.95 * MAX_DIST
    B[90:, 0] -= 0.9 * MAX_DIST
    m = np.zeros(95, dtype=ref.DMATCH)
    m["queryIdx"] = m["trainIdx"] = np.arange(95)
    return dict(A=A, B=B, nA=None, nB=None, matches=m)


def test_refine_round_rejected(fm3d, orc, ctx):
    p = rejected_case()
    got, want = run_both(fm3d, orc, ctx, p, p["matches"], 64, 0, refine=4)
    assert_same(fm3d, got, want, p["matches"])
    rc, rm, adopted = got[6:]
    assert adopted == 0 and 0 <= rc[1] < rc[0] == 95 and (rc[2:] == -2).all() and rm[0].any() and not rm[1:].any()
    assert np.array_equal(got[0][:3, :3].ravel(), got[5][got[3]][:9]) and got[1].all()


def test_refine_without_a_model(fm3d, orc, ctx, big):
    """every hypothesis invalid (all matches name one pair): best -1, c_0 = -1, no round runs"""
    m = np.repeat(big["matches"][:1], 10)
    got, want = run_both(fm3d, orc, ctx, big, m, 5, 0, refine=3)
    assert_same(fm3d, got, want, m)
    assert got[3] == -1 and not got[0].any() and list(got[6]) == [-1, -2, -2, -2] and got[8] == 0


# ---------------------------------------------------------------- quality
# twice what the restatement alone is off (tests/test_align_host.py)
ROT_BOUND_DEG = {0: 2 * 0.1105, 3: 2 * 0.1741, 7: 2 * 0.1078}
ROT_BOUND_REFINED_DEG = 2 * 0.0057


@pytest.mark.parametrize("seed", [0, 3, 7])
def test_quality_case(fm3d, orc, ctx, seed):
    p, r = ref.quality_case(orc, seed)
    _, r4 = ref.quality_case(orc, seed, refine=4)
    al = fm3d.ModelAligner(ctx)
    got = al.align(p["A"], p["B"], p["matches"], MAX_DIST, hypotheses=256, seed=seed, debug=True)
    got4 = al.align(p["A"], p["B"], p["matches"], MAX_DIST, hypotheses=256, seed=seed, refine=4, debug=True)
    assert_same(fm3d, got, r, p["matches"])
    assert_same(fm3d, got4, r4, p["matches"])
    true = p["true"]
    for g in (got, got4):
        kt, kw = int((g[1] & true).sum()), int((g[1] & ~true).sum())
        print("seed", seed, ": kept", kt, "of", int(true.sum()), "true pairs and", kw, "of", int((~true).sum()), "wrong")
        assert kt >= 0.99 * true.sum() and kw <= 0.01 * (~true).sum()
    e0, e4 = ref.rot_err_deg(got[0][:3, :3], p["R"]), ref.rot_err_deg(got4[0][:3, :3], p["R"])
    print("rotation error %.4f deg, refined %.4f deg" % (e0, e4))
    assert e4 <= e0 and e0 <= ROT_BOUND_DEG[seed] and e4 <= ROT_BOUND_REFINED_DEG


# ---------------------------------------------------------------- the matcher in front
def described_models(binary):
    """300 points per model with one descriptor row each: B's rows are A's, permuted with the points
    and lightly disturbed, a fifth of them replaced by noise (those queries fail the ratio test or
    match wrongly)"""
    p = ref.model_pair(N=300, wrong_frac=0.0)
    rng = np.random.default_rng(2)
    perm = p["matches"]["trainIdx"]
    if binary:
        da = rng.integers(0, 256, (300, 32), dtype=np.uint8)
        flip = (rng.random((300, 32, 8)) < 0.03)
        db_rows = da ^ np.packbits(flip, axis=2).reshape(300, 32)
    else:
        da = rng.integers(0, 256, (300, 128), dtype=np.uint8)
        db_rows = np.clip(da.astype(np.int32) + rng.integers(-6, 7, da.shape), 0, 255).astype(np.uint8)
    lost = rng.random(300) < 0.2
    db_rows[lost] = rng.integers(0, 256, (int(lost.sum()), da.shape[1]), dtype=np.uint8)
    db = np.zeros_like(da)
    db[perm] = db_rows
    return p, da, db


@pytest.mark.parametrize("cross", [0, 1])
@pytest.mark.parametrize("binary", [False, True])
def test_match_and_align_equals_the_two_calls(fm3d, binary, cross):
    p, da, db = described_models(binary)
    s = fm3d.Settings.default()
    s.crossCheck = cross
    c = fm3d.Context(s, device=0)
    try:
        dm, al = fm3d.DescriptorsMatcher(c, binary=binary), fm3d.ModelAligner(c)
        m = dm.compareWithNNDRMutual(0.8, da, db, mode=1) if cross else dm.compareWithNNDR(0.8, da, db)
        assert 150 <= len(m) <= 300
        for normals, refine in ((False, 0), (True, 3)):
            na, nb = (p["nA"], p["nB"]) if normals else (None, None)
            two = al.align(p["A"], p["B"], m, MAX_DIST, na, nb, 0.9, hypotheses=64, seed=2, refine=refine, debug=True)
            one = al.match_and_align(da, db, p["A"], p["B"], 0.8, MAX_DIST, na, nb, 0.9, hypotheses=64, seed=2,
                                     refine=refine, debug=True, binary=binary)
            assert one[0].tobytes() == m.tobytes()
            assert len(one) == 1 + len(two)
            for x, y in zip(one[1:], two):
                assert np.asarray(x).tobytes() == np.asarray(y).tobytes()
            assert two[3] >= 0 and two[1].sum() >= 0.9 * len(m)
    finally:
        c.close()


def test_match_and_align_few_matches(fm3d, ctx):
    """unrelated random rows: fewer than three queries pass the ratio test, so no model, FM3D_OK"""
    p = ref.model_pair(N=8, wrong_frac=0.0)
    rng = np.random.default_rng(6)
    da, db = rng.integers(0, 256, (8, 128), dtype=np.uint8), rng.integers(0, 256, (8, 128), dtype=np.uint8)
    m = fm3d.DescriptorsMatcher(ctx).compareWithNNDR(0.5, da, db)
    assert len(m) < 3
    out = fm3d.ModelAligner(ctx).match_and_align(da, db, p["A"], p["B"], 0.5, MAX_DIST, hypotheses=5, refine=2, debug=True)
    assert out[0].tobytes() == m.tobytes() and out[4] == -1 and not out[1].any() and not out[2].any()
    assert len(out[3]) == 0 and (out[5] == -1).all() and not out[6].any() and list(out[7]) == [-1, -2, -2] and out[9] == 0


# ---------------------------------------------------------------- refusals
def test_refusals(fm3d, ctx, big):
    """every refusal with its code, before any launch (the Python mirror's own checks are bypassed)"""
    L = fm3d.lib()
    A, B = np.ascontiguousarray(big["A"][:50]), np.ascontiguousarray(big["B"][:50])
    m = np.zeros(10, dtype=fm3d.DMATCH)
    m["queryIdx"] = m["trainIdx"] = np.arange(10)
    g, mask, out = np.zeros(16), np.zeros(10, dtype=np.uint8), np.zeros(10, dtype=fm3d.DMATCH)
    n, best = ctypes.c_int(0), ctypes.c_int(0)
    vp = lambda a: ctypes.c_void_p(a.ctypes.data) if a is not None else None

    def call(o=None, ptsA=A, nrmA=None, ptsB=B, nrmB=None, mm=m, gg=g, mk=mask, oo=out, pn=ctypes.byref(n),
             pb=ctypes.byref(best), nA=50, nB=50, opts=True):
        o = o or fm3d.AlignOpts(16, 0, 0.01, 0.0, 0)
        return L.fm3d_align_points(ctx.handle, vp(ptsA), vp(nrmA), nA, vp(ptsB), vp(nrmB), nB, vp(mm), len(mm),
                                   ctypes.byref(o) if opts else None, vp(gg), vp(mk), vp(oo), pn, pb, None, None, None,
                                   None, None)

    inv, uns = fm3d.ERR_INVALID, fm3d.ERR_UNSUPPORTED
    assert call() == 0
    assert call(ptsA=None) == inv and call(ptsB=None) == inv and call(gg=None) == inv and call(mk=None) == inv
    assert call(oo=None) == inv and call(pn=None) == inv and call(pb=None) == inv and call(opts=False) == inv
    assert call(nrmA=A) == inv and call(nrmB=B) == inv and call(nrmA=A, nrmB=B) == 0
    assert call(nA=-1) == inv
    assert call(fm3d.AlignOpts(0, 0, 0.01, 0.0, 0)) == inv and call(fm3d.AlignOpts(-5, 0, 0.01, 0.0, 0)) == inv
    for bad in (0.0, -1.0, math.nan, math.inf):
        assert call(fm3d.AlignOpts(16, 0, bad, 0.0, 0)) == inv
    for bad in (1.0000001, -1.5, math.nan):
        assert call(fm3d.AlignOpts(16, 0, 0.01, bad, 0)) == inv
    assert call(fm3d.AlignOpts(16, 0, 0.01, -1.0, 0)) == 0 and call(fm3d.AlignOpts(16, 0, 0.01, 1.0, 0)) == 0
    assert call(fm3d.AlignOpts(16, -1, 0.01, 0.0, 0)) == inv and call(fm3d.AlignOpts(16, 17, 0.01, 0.0, 0)) == inv
    assert call(fm3d.AlignOpts(16, 16, 0.01, 0.0, 0)) == 0
    assert call(fm3d.AlignOpts((1 << 20) + 1, 0, 0.01, 0.0, 0)) == uns
    for field, bad in (("queryIdx", -1), ("queryIdx", 50), ("trainIdx", -1), ("trainIdx", 50)):
        mb = m.copy()
        mb[field][7] = bad
        assert call(mm=mb) == inv
        assert b"index" in L.fm3d_last_error(ctx.handle)
    # the one-call form: the same rules
    d = np.zeros((50, 128), dtype=np.uint8)
    mo = np.zeros(50, dtype=fm3d.DMATCH)
    mk, oo, nm = np.zeros(50, dtype=np.uint8), np.zeros(50, dtype=fm3d.DMATCH), ctypes.c_int(0)

    def call2(o, nrmA=None, descA=d):
        return L.fm3d_match_models(ctx.handle, vp(descA), vp(A), vp(nrmA), 50, vp(d), vp(B), None, 50, 128, fm3d.DESC_U8,
                                   ctypes.c_double(0.8), ctypes.byref(o), vp(mo), ctypes.byref(nm), vp(g), vp(mk), vp(oo),
                                   ctypes.byref(n), ctypes.byref(best), None, None, None, None, None)

    assert call2(fm3d.AlignOpts(16, 0, 0.01, 0.0, 0)) == 0
    assert call2(fm3d.AlignOpts(16, 0, 0.01, 0.0, 0), descA=None) == inv
    assert call2(fm3d.AlignOpts(16, 0, 0.01, 0.0, 0), nrmA=A) == inv
    assert call2(fm3d.AlignOpts(0, 0, 0.01, 0.0, 0)) == inv and call2(fm3d.AlignOpts(16, 0, -0.01, 0.0, 0)) == inv
    assert call2(fm3d.AlignOpts(16, 17, 0.01, 0.0, 0)) == inv and call2(fm3d.AlignOpts(16, 0, 0.01, 2.0, 0)) == inv
    assert call2(fm3d.AlignOpts((1 << 20) + 1, 0, 0.01, 0.0, 0)) == uns
