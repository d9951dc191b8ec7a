"""The refit on the inliers on the GPU ("Refinement"): fm3d_verify_matches_refined
against the plain-Python restatement (tests/verify_refit_pyref.py) -- every round's count and
candidate, the rounds adopted, the final model, its mask and the compacted inliers, bit for bit -- over
the tile shapes, both outcomes of the adoption rule, the invalid refit, the predicate's edge cases, the
quality on noisy keypoints and the end-to-end use."""
import ctypes

import numpy as np
import pytest

import verify_pyref as ref
import verify_refit_pyref as rr

pytestmark = pytest.mark.gpu

H = 64


def make_ctx(fm3d, cam):
    s = fm3d.Settings.default()
    s.set_camera(cam)
    return fm3d.Context(s, device=0)


@pytest.fixture(scope="module")
def case(synth, orc):
    return ref.reference_case(synth, orc)


@pytest.fixture(scope="module")
def ctx(fm3d, case):
    c = make_ctx(fm3d, case["pair"].cam)
    yield c
    c.close()


_RANSAC = {}


def ransac_of(orc, key, x1, x2, hyps, tau, seed):
    """the restatement's RANSAC, once per input (the refine levels share it)"""
    if key not in _RANSAC:
        _RANSAC[key] = ref.ransac(orc, x1, x2, hyps, tau, seed)
    return _RANSAC[key]


def run_both(fm3d, orc, ctx, cam, kp1, kp2, m, max_px, seed, refine, key=None, hyps=H):
    got = fm3d.SingleCameraTriangulator(ctx).verifyMatches(kp1, kp2, m, max_px, hypotheses=hyps, seed=seed, debug=True,
                                                           refine=refine)
    x1, x2 = ref.coords(orc, cam, kp1, kp2, m)
    tau = ref.tau_of(cam, max_px)
    ran = ransac_of(orc, key, x1, x2, hyps, tau, seed) if key else ref.ransac(orc, x1, x2, hyps, tau, seed)
    return got, ran, rr.refined(orc, ran, x1, x2, tau, refine)


def assert_same(fm3d, got, ran, want, m, refine):
    E, mask, inl, best, counts, models = got[:6]
    assert np.array_equal(counts, ran["counts"]) and np.array_equal(models, ran["models"]) and best == ran["best"]
    if refine:
        rc, rm, adopted = got[6:]
        assert np.array_equal(rc, want["roundCounts"]), (rc, want["roundCounts"])
        assert np.array_equal(rm, want["roundModels"])
        assert adopted == want["adopted"]
    else:
        assert len(got) == 6
    assert np.array_equal(E, want["E"])
    assert np.array_equal(mask, want["mask"])
    assert inl.tobytes() == np.ascontiguousarray(m[want["mask"]], dtype=fm3d.DMATCH).tobytes()


# ---------------------------------------------------------------- shapes
def shape_matches(case, M):
    if M <= len(case["matches"]):
        return case["matches"][:M]
    rng = np.random.default_rng(3)
    return case["matches"][rng.integers(0, len(case["matches"]), M)]


@pytest.mark.parametrize("refine", [0, 1, 3])
@pytest.mark.parametrize("M", [7, 8, 9, 257, 1024, 1025, 1800, 2049, 20000])
def test_shapes(fm3d, orc, ctx, case, M, refine):
    """no model (7), the minimum, one / two / three / twenty tiles with full and partial last tiles, the
    compaction's multi-launch scan (20,000); 0, 1 and 3 rounds"""
    pair, m = case["pair"], shape_matches(case, M)
    got, ran, want = run_both(fm3d, orc, ctx, pair.cam, pair.kp1, pair.kp2, m, 1.0, 0, refine, key=("shape", M))
    assert_same(fm3d, got, ran, want, m, refine)
    if M < 8 and refine:
        assert got[3] == -1 and got[6][0] == -1 and (got[6][1:] == -2).all() and not got[7].any() and got[8] == 0
    if refine == 0:  # byte for byte the unrefined call
        plain = fm3d.SingleCameraTriangulator(ctx).verifyMatches(pair.kp1, pair.kp2, m, 1.0, hypotheses=H, seed=0,
                                                                 debug=True)
        assert len(plain) == len(got)
        for u, v in zip(plain, got):
            assert np.asarray(u).tobytes() == np.asarray(v).tobytes()


# ---------------------------------------------------------------- the rule
def test_round_adopted(fm3d, orc, ctx, case):
    """seed 0 at 1 px: 1250 -> 1250 -> 1251 -> 1251, every round adopted (a tie is adopted)"""
    pair, m = case["pair"], case["matches"]
    got, ran, want = run_both(fm3d, orc, ctx, pair.cam, pair.kp1, pair.kp2, m, 1.0, 0, 3)
    assert list(want["roundCounts"]) == [1250, 1250, 1251, 1251] and want["adopted"] == 3
    assert_same(fm3d, got, ran, want, m, 3)
    assert np.array_equal(got[0], got[7][2]) and not np.array_equal(got[0], ran["E"])
    assert got[1].sum() == 1251


def test_round_refused(fm3d, orc, ctx, case):
    """seed 1 at 1 px: the refit keeps 1249 of the best model's 1252, so E_0 stays and the later rounds
    do not run"""
    pair, m = case["pair"], case["matches"]
    got, ran, want = run_both(fm3d, orc, ctx, pair.cam, pair.kp1, pair.kp2, m, 1.0, 1, 3)
    assert list(want["roundCounts"]) == [1252, 1249, -2, -2] and want["adopted"] == 0
    assert_same(fm3d, got, ran, want, m, 3)
    assert np.array_equal(got[0], ran["E"]) and got[7][0].any() and not got[7][1:].any()
    assert got[1].sum() == 1252


def test_too_few_inliers_is_invalid(fm3d, orc, ctx, case):
    """a threshold so small that the best model keeps fewer than 8 matches: no refit, E_0 kept"""
    pair, m = case["pair"], case["matches"][:257]
    got, ran, want = run_both(fm3d, orc, ctx, pair.cam, pair.kp1, pair.kp2, m, 1e-7, 0, 3)
    assert ran["best"] >= 0 and 0 <= ran["counts"][ran["best"]] < 8
    assert list(want["roundCounts"][1:]) == [-1, -2, -2] and want["adopted"] == 0
    assert_same(fm3d, got, ran, want, m, 3)
    assert np.array_equal(got[0], ran["E"]) and not got[7].any()


# ---------------------------------------------------------------- edge cases
def test_nan_keypoint_adds_nothing(fm3d, orc, ctx, case):
    """a NaN keypoint is never in, and its NaN products never reach the sums: the rounds' models are
    those of the same matches without it (its slot is +0.0 either way)"""
    pair, m = case["pair"], case["matches"][:1025]
    kp1 = pair.kp1.copy()
    q = int(m["queryIdx"][10])
    assert (m["queryIdx"] == q).sum() == 1
    kp1[q, 0] = np.nan
    got, ran, want = run_both(fm3d, orc, ctx, pair.cam, kp1, pair.kp2, m, 1.0, 0, 3)
    assert_same(fm3d, got, ran, want, m, 3)
    assert got[8] >= 1 and np.isfinite(got[7]).all() and got[7][0].any() and not got[1][10]
    # the same slots with match 10 replaced by a pair no model accepts in another way: a wrong pair
    x1, x2 = ref.coords(orc, pair.cam, kp1, pair.kp2, m)
    tau = ref.tau_of(pair.cam, 1.0)
    E1, ok = rr.refit(orc, ran["E"], x1, x2, tau)
    y1, y2 = x1.copy(), x2.copy()
    y1[10], y2[10] = (0.9, -0.9), (-0.9, 0.9)
    assert not ref.inliers(ran["E"], y1, y2, tau)[10]
    E2, ok2 = rr.refit(orc, ran["E"], y1, y2, tau)
    assert ok and ok2 and np.array_equal(E1, E2) and np.array_equal(got[7][0], E1)


def test_duplicate_matches(fm3d, orc, ctx, case):
    """every match twice: the normal matrix doubles, whatever the restatement gives, bit for bit"""
    pair = case["pair"]
    m = np.concatenate([case["matches"][:600], case["matches"][:600]])
    got, ran, want = run_both(fm3d, orc, ctx, pair.cam, pair.kp1, pair.kp2, m, 1.0, 2, 3)
    assert_same(fm3d, got, ran, want, m, 3)
    assert ran["best"] >= 0 and want["roundCounts"][1] != -2
    assert np.array_equal(got[1][:600], got[1][600:])


def test_determinism(fm3d, ctx, case):
    pair, m = case["pair"], case["matches"]
    sct = fm3d.SingleCameraTriangulator(ctx)
    a = sct.verifyMatches(pair.kp1, pair.kp2, m, 1.0, hypotheses=H, seed=5, debug=True, refine=3)
    b = sct.verifyMatches(pair.kp1, pair.kp2, m, 1.0, hypotheses=H, seed=5, debug=True, refine=3)
    assert len(a) == 9
    for u, v in zip(a, b):
        assert np.asarray(u).tobytes() == np.asarray(v).tobytes()
    d = sct.verifyMatches(pair.kp1, pair.kp2, m, 1.0, hypotheses=H, seed=5, refine=3)
    assert len(d) == 4 and all(np.asarray(u).tobytes() == np.asarray(v).tobytes() for u, v in zip(a[:4], d))


# ---------------------------------------------------------------- quality
@pytest.mark.parametrize("M", [300, 1800])
def test_quality_on_noisy_keypoints(fm3d, synth, orc, ctx, M):
    """sigma = 0.5 px on both keypoint sets, 256 hypotheses, seeds 0..7 at 1 and 2 px, three rounds: the
    final count is never below c_0, and in at least 12 of the 16 runs the rotation error against the
    true pose is strictly lower than the unrefined model's (the restatement on the CPU: 16 of 16 at
    M = 300, 15 of 16 at M = 1800; tests/test_verify_refit_host.py)"""
    pair, kp1, kp2, m = rr.noisy_inputs(synth, M)
    x1, x2 = ref.coords(orc, pair.cam, kp1, kp2, m)
    sct = fm3d.SingleCameraTriangulator(ctx)
    better = 0
    for px in (1.0, 2.0):
        for seed in range(8):
            E0, mask0, _, best0 = sct.verifyMatches(kp1, kp2, m, px, hypotheses=256, seed=seed)
            E, mask, _, best, _, _, rc, _, adopted = sct.verifyMatches(kp1, kp2, m, px, hypotheses=256, seed=seed,
                                                                        debug=True, refine=3)
            assert best == best0 >= 0 and rc[0] == mask0.sum()
            assert mask.sum() >= rc[0] and mask.sum() == max(c for c in rc if c >= 0)
            err = []
            for Ek, mk in ((E0, mask0), (E, mask)):
                g, _, ok = fm3d.pose_from_epipolar(Ek, x1[mk], x2[mk])
                assert ok
                err.append(rr.rot_err_deg(g[:3, :3], pair.g12[:3, :3]))
            print("M %d, %g px, seed %d: %s adopted %d, rotation %.3f -> %.3f deg" % (M, px, seed, list(rc), adopted,
                                                                                     err[0], err[1]))
            better += err[1] < err[0]
    print("M", M, "better in", better, "of 16")
    assert better >= 12


# ---------------------------------------------------------------- end to end
def test_end_to_end(fm3d, orc, ctx, case):
    """tests/test_gpu_verify.py's path with the refined model: matches from compareWithNNDR at epsilon
    1.0, verified and refined, the pose from the final model, then the triangulation on it"""
    pair, true_train = case["pair"], case["pair"].true_train
    m = fm3d.DescriptorsMatcher(ctx).compareWithNNDR(1.0, pair.desc1, pair.desc2)
    is_true = true_train[m["queryIdx"]] == m["trainIdx"]
    sct = fm3d.SingleCameraTriangulator(ctx)
    E, mask, inl, best = sct.verifyMatches(pair.kp1, pair.kp2, m, 1.0, hypotheses=512, seed=0, refine=3)
    x1, x2 = ref.coords(orc, pair.cam, pair.kp1, pair.kp2, m)
    tau = ref.tau_of(pair.cam, 1.0)
    ran = ref.ransac(orc, x1, x2, 512, tau, 0)
    want = rr.refined(orc, ran, x1, x2, tau, 3)
    assert best == ran["best"] and np.array_equal(E, want["E"]) and np.array_equal(mask, want["mask"])
    assert (mask & is_true).sum() >= 0.99 * is_true.sum()
    assert inl.tobytes() == m[mask].tobytes()
    base = float(np.linalg.norm(pair.g12[:3, 3]))
    g, votes, ok = fm3d.pose_from_epipolar(E, x1[mask], x2[mask], base)
    assert ok and votes.max() >= 0.99 * mask.sum()
    sct.set_g12(g)
    sct.setKeypoints(pair.kp1, pair.kp2, inl)
    pts, tmask = sct.triangulate()
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
    n, best, adopted = ctypes.c_int(0), ctypes.c_int(0), ctypes.c_int(0)
    rc = np.zeros(17, dtype=np.int32)
    vp = lambda a: ctypes.c_void_p(a.ctypes.data) if a is not None else None

    def call(R, E=E, n=ctypes.byref(n), rc=rc):
        return L.fm3d_verify_matches_refined(ctx.handle, vp(k1), len(k1), vp(k2), len(k2), vp(m), 64, 16,
                                             ctypes.c_double(1.0), ctypes.c_uint64(0), R, vp(E), vp(mask), vp(out), n,
                                             ctypes.byref(best), None, None, vp(rc), None, ctypes.byref(adopted))

    for R in (0, 1, 16):
        assert call(R) == fm3d.FM3D_OK and best.value >= 0 and rc[0] >= 8
    for R in (-1, 17):
        assert call(R) == fm3d.ERR_INVALID
    assert call(1, E=None) == fm3d.ERR_INVALID and call(1, n=None) == fm3d.ERR_INVALID
    assert call(2, rc=None) == fm3d.FM3D_OK  # the round outputs are optional
