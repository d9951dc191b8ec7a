"""Geometric verification on the GPU: fm3d_verify_matches against the plain-Python
restatement (tests/verify_pyref.py) -- every hypothesis's model and count, the best, its mask and the
compacted inliers, bit for bit -- over the shapes at which the kernels take another path, the edge
cases of the predicate, the end-to-end use and the argument rules."""
import ctypes
import math

import numpy as np
import pytest

import verify_pyref as ref

pytestmark = pytest.mark.gpu


def make_ctx(fm3d, cam):
    s = fm3d.Settings.default()
    s.set_camera(cam)
    return fm3d.Context(s, device=0)


@pytest.fixture(scope="module")
def case(synth, orc):
    return ref.reference_case(synth, orc)


@pytest.fixture(scope="module")
def ctx(fm3d, case):
    """the end-to-end case's camera: the reference's at width 640 with zero distortion"""
    c = make_ctx(fm3d, case["pair"].cam)
    yield c
    c.close()


def run_both(fm3d, orc, ctx, cam, kp1, kp2, m, max_px, H, seed):
    """(the library's debug result, the restatement's) on the same inputs"""
    got = fm3d.SingleCameraTriangulator(ctx).verifyMatches(kp1, kp2, m, max_px, hypotheses=H, seed=seed, debug=True)
    x1, x2 = ref.coords(orc, cam, kp1, kp2, m)
    return got, ref.ransac(orc, x1, x2, H, ref.tau_of(cam, max_px), seed), (x1, x2)


def assert_same(fm3d, got, want, m, xy=None, seed=0):
    E, mask, inl, best, counts, models = got
    assert np.array_equal(counts, want["counts"])
    assert np.array_equal(models, want["models"])
    assert best == want["best"]
    assert np.array_equal(E, want["E"])
    assert np.array_equal(mask, want["mask"])
    assert inl.tobytes() == np.ascontiguousarray(m[want["mask"]], dtype=fm3d.DMATCH).tobytes()
    if xy is not None:  # the models are the host's epipolar_from8 on ransac_sample's samples
        for h in range(len(counts)):
            idx, ok = fm3d.ransac_sample(seed, h, len(m))
            Eh, okh = fm3d.epipolar_from8(xy[0][idx], xy[1][idx]) if ok else (np.zeros((3, 3)), False)
            assert np.array_equal(models[h], Eh) and (counts[h] >= 0) == okh


# ---------------------------------------------------------------- shapes
@pytest.mark.parametrize("M", [7, 8, 9, 63, 64, 65, 257, 1800])
@pytest.mark.parametrize("H", [1, 5, 64, 257, 512])
def test_shapes(fm3d, orc, ctx, case, M, H):
    """no model (M = 7), the minimum, partial waves and blocks; one hypothesis to several chunks"""
    pair, m = case["pair"], case["matches"][:M]
    got, want, xy = run_both(fm3d, orc, ctx, pair.cam, pair.kp1, pair.kp2, m, 1.0, H, 0)
    assert_same(fm3d, got, want, m, xy)
    if M < 8:
        assert got[3] == -1 and not got[0].any() and not got[1].any() and len(got[2]) == 0 and (got[4] == -1).all()
    if (M, H) == (1800, 512):
        assert want is case["ref"] or np.array_equal(want["counts"], case["ref"]["counts"])
        assert got[1][case["true"]].sum() >= 0.99 * case["true"].sum()


def test_large_shape_takes_the_wide_paths(fm3d, orc, ctx, case):
    """20,000 matches (the compaction's multi-launch scan above 16,384 items) and 3,400 hypotheses: 20
    tiles x 54 chunks of 64 hypotheses, the last one partial"""
    pair = case["pair"]
    rng = np.random.default_rng(3)
    m = case["matches"][rng.integers(0, len(case["matches"]), 20000)]
    got, want, _ = run_both(fm3d, orc, ctx, pair.cam, pair.kp1, pair.kp2, m, 1.0, 3400, 9)
    assert_same(fm3d, got, want, m)
    assert want["best"] >= 0 and want["mask"].sum() > 10000


# ---------------------------------------------------------------- edge cases
def boundary_tau(E, x1, x2):
    """the smallest double t with r^2 <= (t t) den for the one pair (x1, x2)"""
    t = float(np.sqrt(sampson2(E, x1, x2)))
    while not ref.inliers(E, x1, x2, t)[0]:
        t = float(np.nextafter(t, math.inf))
    while ref.inliers(E, x1, x2, float(np.nextafter(t, 0.0)))[0]:
        t = float(np.nextafter(t, 0.0))
    return t


def sampson2(E, x1, x2):
    a, b, c, d = float(x1[0]), float(x1[1]), float(x2[0]), float(x2[1])
    l = [(E[k, 0] * a + E[k, 1] * b) + E[k, 2] for k in range(3)]
    m0 = (E[0, 0] * c + E[1, 0] * d) + E[2, 0]
    m1 = (E[0, 1] * c + E[1, 1] * d) + E[2, 1]
    r = (c * l[0] + d * l[1]) + l[2]
    return r * r / (((l[0] * l[0] + l[1] * l[1]) + m0 * m0) + m1 * m1)


def test_boundary(fm3d, synth, orc, case):
    """Fx = Fy = 1, Cx = Cy = 0, no distortion: tau == maxPx and the keypoints are the coordinates.
    maxPx at r^2 == tau^2 den of one pair keeps it, the next double towards 0 drops it."""
    cam = synth.Camera(1.0, 1.0, 0.0, 0.0, (0.0, 0.0, 0.0, 0.0, 0.0))
    c = make_ctx(fm3d, cam)
    try:
        M, H = 300, 64
        k1 = case["x1"][:M].astype(np.float32)
        k2 = case["x2"][:M].astype(np.float32)
        m = np.zeros(M, dtype=fm3d.DMATCH)
        m["queryIdx"] = m["trainIdx"] = np.arange(M)
        x1, x2 = ref.coords(orc, cam, k1, k2, m)
        assert np.array_equal(x1, k1.astype(np.float64))
        t0 = case["tau"]
        first = ref.ransac(orc, x1, x2, H, t0, 0)
        assert first["best"] >= 0
        d2 = np.array([sampson2(first["E"], x1[i], x2[i]) for i in range(M)])
        out = np.nonzero(~first["mask"])[0]
        p = int(out[np.argmin(d2[out])])  # the nearest pair outside the best model
        tb = boundary_tau(first["E"], x1[p], x2[p])
        assert tb > t0
        for max_px, inside in ((tb, True), (float(np.nextafter(tb, 0.0)), False)):
            assert ref.tau_of(cam, max_px) == max_px
            got, want, _ = run_both(fm3d, orc, c, cam, k1, k2, m, max_px, H, 0)
            assert want["best"] == first["best"]  # the same model: only the threshold moved
            assert bool(want["mask"][p]) == inside
            assert_same(fm3d, got, want, m)
            assert bool(got[1][p]) == inside
    finally:
        c.close()


def test_nan_keypoint_is_never_an_inlier(fm3d, orc, ctx, case):
    pair, m = case["pair"], case["matches"][:257]
    kp1 = pair.kp1.copy()
    q = int(m["queryIdx"][10])
    kp1[q, 0] = np.nan
    H = 257
    got, want, _ = run_both(fm3d, orc, ctx, pair.cam, kp1, pair.kp2, m, 1.0, H, 0)
    assert_same(fm3d, got, want, m)
    assert not got[1][10] and got[3] >= 0
    # some hypothesis drew the NaN match (10 of 257, eight draws, 257 hypotheses): it is invalid
    drew = [h for h in range(H) if 10 in want["samples"][h]]
    assert drew and all(got[4][h] == -1 for h in drew)


def test_duplicate_matches(fm3d, orc, ctx, case):
    """every match twice: a sample that draws both copies has rank <= 7"""
    pair = case["pair"]
    m = np.concatenate([case["matches"][:40], case["matches"][:40]])
    got, want, xy = run_both(fm3d, orc, ctx, pair.cam, pair.kp1, pair.kp2, m, 1.0, 64, 2)
    assert_same(fm3d, got, want, m, xy, seed=2)
    assert np.array_equal(got[1][:40], got[1][40:])


def test_tie_takes_the_lowest_hypothesis(fm3d, orc, ctx, case):
    """eight true pairs: every hypothesis draws the same eight in another order, the models differ in
    their last bits and their counts tie"""
    pair = case["pair"]
    m = case["matches"][np.nonzero(case["true"])[0][::150][:8]]
    assert len(m) == 8
    got, want, _ = run_both(fm3d, orc, ctx, pair.cam, pair.kp1, pair.kp2, m, 1.0, 64, 0)
    assert_same(fm3d, got, want, m)
    counts = got[4]
    top = np.nonzero(counts == counts.max())[0]
    assert len(top) >= 2 and got[3] == top[0]
    assert len({got[5][h].tobytes() for h in top}) >= 2


# ---------------------------------------------------------------- determinism
def test_determinism(fm3d, ctx, case):
    pair, m = case["pair"], case["matches"]
    sct = fm3d.SingleCameraTriangulator(ctx)
    a = sct.verifyMatches(pair.kp1, pair.kp2, m, 1.0, hypotheses=512, seed=5, debug=True)
    b = sct.verifyMatches(pair.kp1, pair.kp2, m, 1.0, hypotheses=512, seed=5, debug=True)
    for u, v in zip(a, b):
        assert np.asarray(u).tobytes() == np.asarray(v).tobytes()
    c = sct.verifyMatches(pair.kp1, pair.kp2, m, 1.0, hypotheses=512, seed=6, debug=True)
    assert not np.array_equal(a[5], c[5])  # other samples
    assert c[3] >= 0 and c[1][case["true"]].sum() >= 0.99 * case["true"].sum()
    # without the debug outputs: the same result
    d = sct.verifyMatches(pair.kp1, pair.kp2, m, 1.0, hypotheses=512, seed=5)
    assert len(d) == 4 and all(np.asarray(u).tobytes() == np.asarray(v).tobytes() for u, v in zip(a[:4], d))


# ---------------------------------------------------------------- end to end
def test_end_to_end(fm3d, orc, ctx, case):
    """matches from compareWithNNDR at epsilon 1.0 (the distractors get through), verified, the pose
    taken from the model, and the rest of the path run on it"""
    pair, true_train = case["pair"], case["pair"].true_train
    m = fm3d.DescriptorsMatcher(ctx).compareWithNNDR(1.0, pair.desc1, pair.desc2)
    is_true = true_train[m["queryIdx"]] == m["trainIdx"]
    assert len(m) == 2000 and 1700 <= is_true.sum() < len(m)
    sct = fm3d.SingleCameraTriangulator(ctx)
    E, mask, inl, best = sct.verifyMatches(pair.kp1, pair.kp2, m, 1.0, hypotheses=512, seed=0)
    x1, x2 = ref.coords(orc, pair.cam, pair.kp1, pair.kp2, m)
    want = ref.ransac(orc, x1, x2, 512, ref.tau_of(pair.cam, 1.0), 0)
    assert best == want["best"] and np.array_equal(E, want["E"]) and np.array_equal(mask, want["mask"])
    print("kept", int((mask & is_true).sum()), "of", int(is_true.sum()), "true and", int((mask & ~is_true).sum()), "of",
          int((~is_true).sum()), "wrong")
    assert (mask & is_true).sum() >= 0.99 * is_true.sum()
    assert inl.tobytes() == m[mask].tobytes()
    base = float(np.linalg.norm(pair.g12[:3, 3]))
    g, votes, ok = fm3d.pose_from_epipolar(E, x1[mask], x2[mask], base)
    assert ok and votes.max() >= 0.99 * mask.sum()
    sct.set_g12(g)
    sct.setKeypoints(pair.kp1, pair.kp2, inl)
    pts, tmask = sct.triangulate()
    print("triangulated", len(pts), "of", len(inl))
    assert len(pts) > 0 and len(pts) == tmask.sum() and np.isfinite(pts).all()


# ---------------------------------------------------------------- interface
def test_invalid_arguments(fm3d, ctx, case):
    L = fm3d.lib()
    pair = case["pair"]
    k1 = np.ascontiguousarray(pair.kp1, dtype=np.float32)
    k2 = np.ascontiguousarray(pair.kp2, dtype=np.float32)
    m = np.ascontiguousarray(case["matches"][:64], dtype=fm3d.DMATCH)
    E = np.zeros(9)
    mask = np.zeros(64, dtype=np.uint8)
    out = np.zeros(64, dtype=fm3d.DMATCH)
    n, best = ctypes.c_int(0), ctypes.c_int(0)
    vp = lambda a: ctypes.c_void_p(a.ctypes.data) if a is not None else None

    def call(k1=k1, k2=k2, m=m, K=64, H=16, px=1.0, E=E, mask=mask, out=out, n=ctypes.byref(n), best=ctypes.byref(best),
             n1=len(k1), n2=len(k2)):
        return L.fm3d_verify_matches(ctx.handle, vp(k1), n1, vp(k2), n2, vp(m), K, H, ctypes.c_double(px),
                                     ctypes.c_uint64(0), vp(E), vp(mask), vp(out), n, best, None, None)

    assert call() == fm3d.FM3D_OK and best.value >= 0
    for kw in (dict(E=None), dict(n=None), dict(best=None), dict(k1=None), dict(k2=None), dict(m=None),
               dict(mask=None), dict(out=None), dict(K=-1), dict(H=0), dict(H=-3), dict(px=0.0), dict(px=-1.0),
               dict(px=math.nan), dict(px=math.inf)):
        assert call(**kw) == fm3d.ERR_INVALID, kw
    for field, bad in (("queryIdx", -1), ("queryIdx", len(k1)), ("trainIdx", -1), ("trainIdx", len(k2))):
        mb = m.copy()
        mb[field][63] = bad
        assert call(m=mb) == fm3d.ERR_INVALID, (field, bad)
    assert call(H=(1 << 20) + 1) == fm3d.ERR_UNSUPPORTED
    assert call(K=0, m=None, mask=None, out=None) == fm3d.FM3D_OK and best.value == -1 and n.value == 0
    assert call() == fm3d.FM3D_OK and best.value >= 0  # the context is still usable
