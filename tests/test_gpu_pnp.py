"""2D-3D localisation on the GPU: fm3d_localize_points and fm3d_localize_model against the
plain-Python restatement (tests/pnp_pyref.py) -- every hypothesis's model and count, the best, the
rounds of the refit, the final pose, its mask and the compacted inliers, bit for bit -- over the
shapes at which the kernels take another path, the edge cases of the predicate and the argument rules.
No case provokes a fault: every index is validated on the host, and the NaN cases are data."""
import ctypes
import math

import numpy as np
import pytest

import pnp_pyref as ref

pytestmark = pytest.mark.gpu

MAX_PX = 2.0


def make_ctx(fm3d, cam):
    s = fm3d.Settings.default()
    s.set_camera(cam)
    return fm3d.Context(s, device=0)


@pytest.fixture(scope="module")
def big():
    """the quality recipe at 1,800 points: the shapes' inputs"""
    return ref.scene(N=1800)


@pytest.fixture(scope="module")
def ctx(fm3d, big):
    c = make_ctx(fm3d, big["cam"])
    yield c
    c.close()


def run_both(fm3d, orc, ctx, p, m, samples, seed, refine=0, normals=False, min_cos=0.5, max_px=MAX_PX):
    """(the library's debug result, the restatement's) on the same inputs"""
    n = p["n"] if normals else None
    got = fm3d.ModelLocalizer(ctx).localize(p["X"], p["kpts"], m, max_px, n, min_cos, samples=samples, seed=seed,
                                            refine=refine, debug=True)
    return got, ref.localize(orc, p["cam"], p["X"], p["kpts"], m, max_px, samples, seed, refine, n, min_cos)


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
@pytest.mark.parametrize("samples", [1, 5, 16, 17, 65])
def test_shapes(fm3d, orc, ctx, big, M, samples, normals):
    """no model (M = 2), the minimum, partial waves, blocks and tiles; one sample to several chunks of 64
    hypotheses (16 samples fill one, 17 cross it); both instances of the scoring kernel"""
    m = big["matches"][:M]
    got, want = run_both(fm3d, orc, ctx, big, m, samples, 0, normals=normals)
    assert_same(fm3d, got, want, m)
    assert got[4].shape == (4 * samples,) and got[5].shape == (4 * samples, 12)
    if M < 3:
        assert got[3] == -1 and not got[0].any() and not got[1].any() and len(got[2]) == 0 and (got[4] == -1).all()
    if M >= 257 and samples >= 16:  # (0.343 of the samples are clean: the consensus is found; the caps are the quality case's)
        assert got[3] >= 0 and got[1][big["true"][:M]].sum() > 0.5 * big["true"][:M].sum()
        assert np.array_equal(got[0][3], [0, 0, 0, 1])


def test_normals_are_a_second_test(fm3d, orc, ctx, big):
    """the scene's normals lie along the viewing rays; a model whose normals face the other way keeps
    no match, one with a third of them turned keeps the others"""
    m = big["matches"][:1025]
    p = dict(big)
    p["n"] = big["n"].copy()
    p["n"][::3] = -p["n"][::3]
    plain, want0 = run_both(fm3d, orc, ctx, p, m, 64, 0)
    both, want1 = run_both(fm3d, orc, ctx, p, m, 64, 0, normals=True, min_cos=0.9)
    assert_same(fm3d, plain, want0, m)
    assert_same(fm3d, both, want1, m)
    turned = (m["trainIdx"] % 3) == 0
    assert plain[1][turned].any() and not both[1][turned].any()
    assert both[3] >= 0 and np.array_equal(both[1][~turned], plain[1][~turned])


# ---------------------------------------------------------------- the predicate's edges
UNIT = ref.Cam(1.0, 1.0, 0.0, 0.0)


def clean_scene(n, seed=9):
    """n exact matches under the unit camera (keypoints are normalised coordinates, tau = max_px): points
    in front of a camera at a random pose, keypoints rounded to float32"""
    rng = np.random.default_rng(seed)
    R, t = ref.rodrigues(rng.normal(size=3), 0.3), rng.uniform(-0.3, 0.3, 3)
    Xc = np.stack([rng.uniform(-0.8, 0.8, n), rng.uniform(-0.6, 0.6, n), rng.uniform(1.6, 2.3, n)], axis=1)
    m = np.zeros(n, dtype=ref.DMATCH)
    m["queryIdx"] = m["trainIdx"] = np.arange(n)
    return dict(cam=UNIT, X=(Xc - t) @ R, n=None, kpts=(Xc[:, :2] / Xc[:, 2:3]).astype(np.float32), R=R, t=t, matches=m)


def boundary_case(orc):
    """200 clean matches and three more of one extra point, under the unit camera.  With (x, y, z) the
    extra point under the best model in the contract's order and its keypoint (u, v) about 2^-8 from
    the projection, max_px is the double next to |(x - u z, y - v z)| / z for which tau^2 z^2 equals
    (x - u z)^2 + (y - v z)^2 exactly as the predicate computes them: at the threshold; the keypoints one
    float32 ulp of u nearer and farther lie inside and outside"""
    p = clean_scene(201)
    kp = np.concatenate([p["kpts"][:200], np.full((3, 2), 50.0, dtype=np.float32)])  # far off: in no winning sample
    m = np.zeros(203, dtype=ref.DMATCH)
    m["queryIdx"], m["trainIdx"] = np.arange(203), np.minimum(np.arange(203), 200)
    p["kpts"] = kp
    tau0 = 2.0 ** -8
    # one sample: its true slot keeps the 200, and no other model is near enough for the extras to matter
    r = ref.localize(orc, UNIT, p["X"], kp, m, tau0, 1, 0)
    assert r["best"] >= 0 and max(r["ransac"]["samples"][0]) < 200 and r["counts"][r["best"]] == 200
    assert sorted(r["counts"])[-2] < 100
    mod = [float(v) for v in r["model"]]
    X = [float(v) for v in p["X"][200]]
    x, y, z = [ref._rot_row(mod, k, X[0], X[1], X[2]) + mod[9 + k] for k in range(3)]
    u, v = np.float32(x / z - tau0), np.float32(y / z)
    ex, ey = x - float(u) * z, y - float(v) * z
    e, zz = ex * ex + ey * ey, z * z
    tau = math.sqrt(e / zz)
    for _ in range(8):
        tau = np.nextafter(tau, 0.0)
    for _ in range(17):
        if (tau * tau) * zz == e:
            break
        tau = float(np.nextafter(tau, 1.0))
    assert (tau * tau) * zz == e and abs(tau - tau0) < 1e-4 * tau0
    kp[200] = [u, v]
    kp[201] = [np.nextafter(u, np.float32(1.0)), v]   # towards the projection: inside
    kp[202] = [np.nextafter(u, np.float32(-1.0)), v]  # away from it: outside
    return p, m, float(tau), r["model"]


def test_match_exactly_at_the_threshold(fm3d, orc):
    p, m, tau, model = boundary_case(orc)
    c = make_ctx(fm3d, UNIT)
    try:
        assert ref.tau_of(UNIT, tau) == tau
        got, want = run_both(fm3d, orc, c, p, m, 1, 0, max_px=tau)
        assert np.array_equal(want["model"], model)  # the three matches did not change the best model
        assert list(want["mask"][200:]) == [True, True, False]
        assert_same(fm3d, got, want, m)
        assert list(got[1][200:]) == [True, True, False] and got[1][:200].all()
    finally:
        c.close()


def test_nan_and_behind_the_camera(fm3d, orc, ctx, big):
    """a NaN point, keypoint or normal is never an inlier; neither is a point behind the camera whose
    line through the centre meets the keypoint"""
    p = dict(big)
    p["X"], p["kpts"], p["n"] = big["X"].copy(), big["kpts"].copy(), big["n"].copy()
    m = big["matches"][:300]
    true = np.nonzero(big["true"][:300])[0]
    ia, ib, ic, idd = true[:4]
    p["X"][m["trainIdx"][ia], 1] = math.nan
    p["kpts"][m["queryIdx"][ib], 0] = math.nan
    p["n"][m["trainIdx"][ic], 0] = math.nan
    # mirrored through the camera centre: Xc -> -Xc, i.e. X -> R^T (-(R X + t) - t)
    Xd = p["X"][m["trainIdx"][idd]]
    p["X"][m["trainIdx"][idd]] = big["R"].T @ (-(big["R"] @ Xd + big["t"]) - big["t"])
    for normals in (False, True):
        got, want = run_both(fm3d, orc, ctx, p, m, 64, 0, normals=normals, refine=2)
        assert_same(fm3d, got, want, m)
        assert got[3] >= 0 and not got[1][ia] and not got[1][ib] and not got[1][idd] and got[1][ic] == (not normals)
        assert np.isfinite(got[0]).all() and got[1][true[4:]].all()


def test_coplanar_model_localises(fm3d, orc, big):
    """every model point on one exact plane (no six-point DLT has a solution there): the pose comes out"""
    p = ref.scene(N=1025, relief=False)
    c = make_ctx(fm3d, p["cam"])
    try:
        got, want = run_both(fm3d, orc, c, p, p["matches"], 64, 0, refine=4)
        assert_same(fm3d, got, want, p["matches"])
        true = p["true"]
        assert got[3] >= 0 and got[1][true].sum() >= 0.99 * true.sum() and got[1][~true].sum() <= 0.01 * (~true).sum()
        assert ref.rot_err_deg(got[0][:3, :3], p["R"]) < 0.1
    finally:
        c.close()


def test_duplicate_matches(fm3d, orc, ctx, big):
    """every match three times over: some samples hold one match twice (a zero side: no model), and every
    copy is counted and kept"""
    m = np.repeat(big["matches"][:100], 3)
    got, want = run_both(fm3d, orc, ctx, big, m, 65, 0, refine=1)
    assert_same(fm3d, got, want, m)
    twice = [h for h, s in enumerate(want["ransac"]["samples"]) if len({i // 3 for i in s}) < 3]
    assert twice and got[3] >= 0 and (got[4].reshape(-1, 4)[twice] == -1).all()
    assert np.array_equal(got[1][0::3], got[1][1::3]) and np.array_equal(got[1][0::3], got[1][2::3])


def test_seed_determinism(fm3d, ctx, big):
    loc = fm3d.ModelLocalizer(ctx)
    m = big["matches"]
    runs = [loc.localize(big["X"], big["kpts"], m, MAX_PX, samples=65, seed=s, refine=2, debug=True) for s in (3, 3, 4)]
    for x, y in zip(runs[0], runs[1]):
        assert np.asarray(x).tobytes() == np.asarray(y).tobytes()
    assert not np.array_equal(runs[0][5], runs[2][5])


# ---------------------------------------------------------------- refinement
@pytest.mark.parametrize("normals", [False, True])
@pytest.mark.parametrize("refine", [1, 4, 16])
def test_refine_rounds(fm3d, orc, ctx, big, refine, normals):
    """1,800 matches (two tiles): every round's model and count; codes >= 0 adopted or rejected, -2 not run"""
    m = big["matches"]
    got, want = run_both(fm3d, orc, ctx, big, m, 16, 0, refine=refine, normals=normals)
    assert_same(fm3d, got, want, m)
    rc, rm, adopted = got[6:]
    assert rc.shape == (refine + 1,) and rm.shape == (refine, 12) and 1 <= adopted <= refine
    assert rc[0] == got[4][got[3]] and (rc[1:1 + adopted] >= rc[0]).all()
    ran = int((rc[1:] != -2).sum())
    assert ran in (adopted, adopted + 1) and (rc[1 + ran:] == -2).all() and not rm[ran:].any()
    assert int(got[1].sum()) == rc[adopted]


def test_refine_zero_is_the_unrefined_call(fm3d, ctx, big):
    """refineIters == 0 with the rounds' outputs given: byte for byte what the RANSAC alone gives, and
    the rounds' outputs say that none ran"""
    m = big["matches"][:1025]
    loc = fm3d.ModelLocalizer(ctx)
    plain = loc.localize(big["X"], big["kpts"], m, MAX_PX, samples=16, seed=1, debug=True)
    L, o = fm3d.lib(), fm3d.LocalizeOpts(16, 0, MAX_PX, 0.0, 1)
    g, mask, out = np.zeros(16), np.zeros(len(m), dtype=np.uint8), np.zeros(len(m), dtype=fm3d.DMATCH)
    n, best, adopted = ctypes.c_int(0), ctypes.c_int(0), ctypes.c_int(99)
    rc = np.full(1, 77, dtype=np.int32)
    vp = lambda a: ctypes.c_void_p(a.ctypes.data)
    mm, X, kp = np.ascontiguousarray(m), np.ascontiguousarray(big["X"]), np.ascontiguousarray(big["kpts"])
    assert L.fm3d_localize_points(ctx.handle, vp(X), None, len(X), vp(kp), len(kp), vp(mm), len(mm), ctypes.byref(o), vp(g),
                                  vp(mask), vp(out), ctypes.byref(n), ctypes.byref(best), None, None, vp(rc), None,
                                  ctypes.byref(adopted)) == 0
    assert np.array_equal(g.reshape(4, 4), plain[0]) and np.array_equal(mask.astype(bool), plain[1])
    assert out[:n.value].tobytes() == plain[2].tobytes() and best.value == plain[3]
    assert adopted.value == 0 and rc[0] == n.value == plain[4][plain[3]]


def test_refine_without_a_model(fm3d, orc, ctx, big):
    """every hypothesis invalid (all matches name one pair): best -1, c_0 = -1, no round runs"""
    m = np.repeat(big["matches"][:1], 10)
    got, want = run_both(fm3d, orc, ctx, big, m, 5, 0, refine=3)
    assert_same(fm3d, got, want, m)
    assert got[3] == -1 and not got[0].any() and list(got[6]) == [-1, -2, -2, -2] and got[8] == 0


# ---------------------------------------------------------------- quality
# twice what the restatement alone is off (tests/test_pnp_host.py), relief and planar
ROT_BOUND_DEG = {(True, 0): 2 * 0.1894, (True, 3): 2 * 0.1058, (True, 7): 2 * 0.1209,
                 (False, 0): 2 * 0.1481, (False, 3): 2 * 0.1752, (False, 7): 2 * 0.2448}
ROT_BOUND_REFINED_DEG = {True: 2 * 0.0179, False: 2 * 0.0058}


@pytest.mark.parametrize("relief", [True, False])
@pytest.mark.parametrize("seed", [0, 3, 7])
def test_quality_case(fm3d, orc, ctx, seed, relief):
    p, r = ref.quality_case(orc, seed, relief)
    _, r4 = ref.quality_case(orc, seed, relief, refine=4)
    loc = fm3d.ModelLocalizer(ctx)
    got = loc.localize(p["X"], p["kpts"], p["matches"], MAX_PX, samples=256, seed=seed, debug=True)
    got4 = loc.localize(p["X"], p["kpts"], p["matches"], MAX_PX, samples=256, seed=seed, refine=4, debug=True)
    assert_same(fm3d, got, r, p["matches"])
    assert_same(fm3d, got4, r4, p["matches"])
    true = p["true"]
    for g in (got, got4):
        kt, kw = int((g[1] & true).sum()), int((g[1] & ~true).sum())
        print("seed", seed, ": kept", kt, "of", int(true.sum()), "true matches and", kw, "of", int((~true).sum()), "wrong")
        assert kt >= 0.99 * true.sum() and kw <= 0.01 * (~true).sum()
    e0, e4 = ref.rot_err_deg(got[0][:3, :3], p["R"]), ref.rot_err_deg(got4[0][:3, :3], p["R"])
    print("rotation error %.4f deg, refined %.4f deg" % (e0, e4))
    assert e4 <= e0 and e0 <= ROT_BOUND_DEG[relief, seed] and e4 <= ROT_BOUND_REFINED_DEG[relief]


def test_loop_closing(fm3d, synth, orc):
    """a model in camera 1's frame (a synthetic pair's points) localised against image 2 returns the
    pair's g12, the pose fm3d_set_g12 installs, within the quality table's error; the keypoints are exact
    projections rounded to float32 (zero distortion, as §3.1d's end-to-end case: the five-step
    undistortion is no exact inverse of the projection)"""
    cam = synth.Camera.reference(640)
    pair = synth.make_frame_pair(400, seed=2, cam=synth.Camera(cam.fx, cam.fy, cam.cx, cam.cy, (0.0,) * 5))
    q = np.nonzero(pair.true_train >= 0)[0]
    m = np.zeros(q.size, dtype=ref.DMATCH)
    m["queryIdx"], m["trainIdx"] = pair.true_train[q], q
    rng = np.random.default_rng(1)
    wrong = rng.random(q.size) < 0.3
    m["queryIdx"][wrong] = rng.integers(0, pair.kp2.shape[0], int(wrong.sum()))
    true = m["queryIdx"] == pair.true_train[q]
    assert (np.einsum("ij,ij->i", pair.normals, pair.points) > 0).all()  # away from camera 1: the predicate's sign
    c = make_ctx(fm3d, pair.cam)
    try:
        p = dict(cam=pair.cam, X=pair.points, n=pair.normals, kpts=pair.kp2)
        for normals in (False, True):
            got, want = run_both(fm3d, orc, c, p, m, 64, 0, refine=4, normals=normals, min_cos=0.0)
            assert_same(fm3d, got, want, m)
            g = got[0]
            assert got[3] >= 0 and got[1][true].sum() >= 0.99 * true.sum() and not got[1][~true].any()
            assert ref.rot_err_deg(g[:3, :3], pair.g12[:3, :3]) <= min(ROT_BOUND_REFINED_DEG.values())
            assert np.abs(g[:3, 3] - pair.g12[:3, 3]).max() < 1e-3
    finally:
        c.close()


def test_distorted_camera(fm3d, orc):
    """a camera with all five distortion coefficients: the gather kernel's undistortion is the
    oracle's, so everything behind it still equals the restatement (the scene was drawn without
    distortion: fewer matches agree, which is beside the point)"""
    cam = ref.Cam(k=(-0.02, 0.004, 0.0005, -0.0003, 0.001))
    p = ref.scene(N=257, cam=cam)
    c = make_ctx(fm3d, cam)
    try:
        got, want = run_both(fm3d, orc, c, p, p["matches"], 17, 0, refine=2, normals=True)
        assert_same(fm3d, got, want, p["matches"])
        assert got[3] >= 0 and got[1].sum() >= 20
    finally:
        c.close()


# ---------------------------------------------------------------- the matcher in front
def described_scene(binary):
    """300 model points with one descriptor row each; the image's rows are the model's, permuted with
    the keypoints and lightly disturbed, a fifth of them replaced by noise (those queries fail the ratio
    test or match wrongly)"""
    p = ref.scene(N=300, wrong_frac=0.0)
    rng = np.random.default_rng(2)
    perm = p["matches"]["queryIdx"]
    if binary:
        dm = rng.integers(0, 256, (300, 32), dtype=np.uint8)
        flip = (rng.random((300, 32, 8)) < 0.03)
        rows = dm ^ np.packbits(flip, axis=2).reshape(300, 32)
    else:
        dm = rng.integers(0, 256, (300, 128), dtype=np.uint8)
        rows = np.clip(dm.astype(np.int32) + rng.integers(-6, 7, dm.shape), 0, 255).astype(np.uint8)
    lost = rng.random(300) < 0.2
    rows[lost] = rng.integers(0, 256, (int(lost.sum()), dm.shape[1]), dtype=np.uint8)
    di = np.zeros_like(dm)
    di[perm] = rows
    return p, di, dm


@pytest.mark.parametrize("cross", [0, 1])
@pytest.mark.parametrize("binary", [False, True])
def test_match_and_localize_equals_the_two_calls(fm3d, binary, cross):
    p, di, dm = described_scene(binary)
    s = fm3d.Settings.default()
    s.set_camera(p["cam"])
    s.crossCheck = cross
    c = fm3d.Context(s, device=0)
    try:
        mt, loc = fm3d.DescriptorsMatcher(c, binary=binary), fm3d.ModelLocalizer(c)
        m = mt.compareWithNNDRMutual(0.8, di, dm, mode=1) if cross else mt.compareWithNNDR(0.8, di, dm)
        assert 150 <= len(m) <= 300
        for normals, refine in ((False, 0), (True, 3)):
            n = p["n"] if normals else None
            two = loc.localize(p["X"], p["kpts"], m, MAX_PX, n, 0.5, samples=16, seed=2, refine=refine, debug=True)
            one = loc.match_and_localize(di, p["kpts"], dm, p["X"], 0.8, MAX_PX, n, 0.5, samples=16, seed=2, refine=refine,
                                         debug=True, binary=binary)
            assert one[0].tobytes() == m.tobytes()
            assert len(one) == 1 + len(two)
            for x, y in zip(one[1:], two):
                assert np.asarray(x).tobytes() == np.asarray(y).tobytes()
            assert two[3] >= 0 and two[1].sum() >= 0.9 * len(m)
    finally:
        c.close()


def test_match_and_localize_few_matches(fm3d, ctx):
    """unrelated random rows: fewer than three queries pass the ratio test, so no model, FM3D_OK"""
    p = ref.scene(N=8, wrong_frac=0.0)
    rng = np.random.default_rng(6)
    di, dm = rng.integers(0, 256, (8, 128), dtype=np.uint8), rng.integers(0, 256, (8, 128), dtype=np.uint8)
    m = fm3d.DescriptorsMatcher(ctx).compareWithNNDR(0.5, di, dm)
    assert len(m) < 3
    out = fm3d.ModelLocalizer(ctx).match_and_localize(di, p["kpts"], dm, p["X"], 0.5, MAX_PX, samples=5, refine=2, debug=True)
    assert out[0].tobytes() == m.tobytes() and out[4] == -1 and not out[1].any() and not out[2].any()
    assert len(out[3]) == 0 and (out[5] == -1).all() and not out[6].any() and list(out[7]) == [-1, -2, -2] and out[9] == 0


# ---------------------------------------------------------------- refusals
def test_refusals(fm3d, ctx, big):
    """every refusal with its code, before any launch (the Python mirror's own checks are bypassed)"""
    L = fm3d.lib()
    X, kp = np.ascontiguousarray(big["X"][:50]), np.ascontiguousarray(big["kpts"][:40])
    m = np.zeros(10, dtype=fm3d.DMATCH)
    m["queryIdx"] = m["trainIdx"] = np.arange(10)
    g, mask, out = np.zeros(16), np.zeros(10, dtype=np.uint8), np.zeros(10, dtype=fm3d.DMATCH)
    n, best = ctypes.c_int(0), ctypes.c_int(0)
    vp = lambda a: ctypes.c_void_p(a.ctypes.data) if a is not None else None
    LO = fm3d.LocalizeOpts

    def call(o=None, pts=X, nrm=None, kpts=kp, mm=m, gg=g, mk=mask, oo=out, pn=ctypes.byref(n), pb=ctypes.byref(best),
             nP=50, nK=40, opts=True):
        o = o or LO(16, 0, 1.0, 0.0, 0)
        return L.fm3d_localize_points(ctx.handle, vp(pts), vp(nrm), nP, vp(kpts), nK, vp(mm), len(mm),
                                      ctypes.byref(o) if opts else None, vp(gg), vp(mk), vp(oo), pn, pb, None, None, None,
                                      None, None)

    inv, uns = fm3d.ERR_INVALID, fm3d.ERR_UNSUPPORTED
    assert call() == 0 and call(nrm=X) == 0
    assert call(pts=None) == inv and call(kpts=None) == inv and call(gg=None) == inv and call(mk=None) == inv
    assert call(oo=None) == inv and call(pn=None) == inv and call(pb=None) == inv and call(opts=False) == inv
    assert call(mm=m[:0], mk=None, oo=None) == 0  # no matches: nothing to write
    assert call(nP=-1) == inv and call(nK=-1) == inv
    assert call(LO(0, 0, 1.0, 0.0, 0)) == inv and call(LO(-5, 0, 1.0, 0.0, 0)) == inv
    for bad in (0.0, -1.0, math.nan, math.inf):
        assert call(LO(16, 0, bad, 0.0, 0)) == inv
    for bad in (1.0000001, -0.01, math.nan):
        assert call(LO(16, 0, 1.0, bad, 0)) == inv
    assert call(LO(16, 0, 1.0, 0.0, 0)) == 0 and call(LO(16, 0, 1.0, 1.0, 0)) == 0
    assert call(LO(16, -1, 1.0, 0.0, 0)) == inv and call(LO(16, 17, 1.0, 0.0, 0)) == inv
    assert call(LO(16, 16, 1.0, 0.0, 0)) == 0
    assert call(LO((1 << 18) + 1, 0, 1.0, 0.0, 0)) == uns
    for field, bad in (("queryIdx", -1), ("queryIdx", 40), ("trainIdx", -1), ("trainIdx", 50)):
        mb = m.copy()
        mb[field][7] = bad
        assert call(mm=mb) == inv
        assert b"index" in L.fm3d_last_error(ctx.handle)
    # the one-call form: the same rules
    di, dm = np.zeros((40, 128), dtype=np.uint8), np.zeros((50, 128), dtype=np.uint8)
    mo = np.zeros(40, dtype=fm3d.DMATCH)
    mk, oo, nm = np.zeros(40, dtype=np.uint8), np.zeros(40, dtype=fm3d.DMATCH), ctypes.c_int(0)

    def call2(o, descImg=di, kpts=kp, pts=X):
        return L.fm3d_localize_model(ctx.handle, vp(descImg), vp(kpts), 40, vp(dm), vp(pts), None, 50, 128, fm3d.DESC_U8,
                                     ctypes.c_double(0.8), ctypes.byref(o), vp(mo), ctypes.byref(nm), vp(g), vp(mk), vp(oo),
                                     ctypes.byref(n), ctypes.byref(best), None, None, None, None, None)

    assert call2(LO(16, 0, 1.0, 0.0, 0)) == 0
    assert call2(LO(16, 0, 1.0, 0.0, 0), descImg=None) == inv and call2(LO(16, 0, 1.0, 0.0, 0), kpts=None) == inv
    assert call2(LO(16, 0, 1.0, 0.0, 0), pts=None) == inv
    assert call2(LO(0, 0, 1.0, 0.0, 0)) == inv and call2(LO(16, 0, -1.0, 0.0, 0)) == inv
    assert call2(LO(16, 17, 1.0, 0.0, 0)) == inv and call2(LO(16, 0, 1.0, 2.0, 0)) == inv
    assert call2(LO((1 << 18) + 1, 0, 1.0, 0.0, 0)) == uns
