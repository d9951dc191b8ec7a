"""The staged pipeline on verified matches (DESIGN.md §3.1d "In the pipeline"):
fm3d_pipeline_run_verified and fm3d_pipeline_run_dlt_verified against the composition of the public
calls they replace -- compareWithNNDR, verifyMatches, pose_from_epipolar, set_g12, triangulate,
computeOptimizedNormals -- bit for bit.  The pair is verify_pyref.verify_inputs': 2,000 keypoints, the
last 200 of them distractors, the zero-distortion camera; pixelsRay = 16 and nndrEpsilon = 1.0, so every
query keeps its match (K = nA) and the distractors' wrong ones reach the verification."""
import ctypes

import numpy as np
import pytest

import verify_pyref as ref

pytestmark = pytest.mark.gpu

MAX_PX = 1.0


@pytest.fixture(scope="module")
def pair(synth):
    return ref.verify_inputs(synth)[0]


@pytest.fixture(scope="module")
def base(pair):
    return float(np.linalg.norm(pair.g12[:3, 3]))


def make_ctx(fm3d, pair, g12=None, **fields):
    s = fm3d.Settings.default()
    s.set_camera(pair.cam)
    s.pixelsRay = 16
    s.nndrEpsilon = 1.0
    for k, v in fields.items():
        setattr(s, k, v)
    c = fm3d.Context(s, device=0)
    if g12 is not None:
        fm3d.SingleCameraTriangulator(c).set_g12(g12)
    return c


def upload(fm3d, c, pair, nA=None, images=True, **kw):
    nA = len(pair.desc1) if nA is None else nA
    pipe = fm3d.Pipeline(c)
    pipe.upload(pair.desc1[:nA], pair.desc2, pair.kp1[:nA], pair.kp2, pair.img1 if images else None,
                pair.img2 if images else None, **kw)
    return pipe


def composed(fm3d, orc, c, pair, nA, H, seed=0, refine=0, baseline=None, g12=None, max_px=MAX_PX, normals=False):
    """The calls the verified run replaces, on the context c (not the one under test): match, verify,
    the pose from the model (or the given g12), triangulate and, when asked, the LM -> dict."""
    kp1, d1 = pair.kp1[:nA], pair.desc1[:nA]
    m = fm3d.DescriptorsMatcher(c).compareWithNNDR(1.0, d1, pair.desc2)
    sct = fm3d.SingleCameraTriangulator(c)
    E, mask, inl, best = sct.verifyMatches(kp1, pair.kp2, m, max_px, hypotheses=H, seed=seed, refine=refine)
    out = dict(m=m, E=E, mask=mask, inl=inl, best=best, ok=best >= 0, votes=np.zeros(4, dtype=np.int32), g12=None)
    if best < 0:
        return out
    if g12 is None:
        x1, x2 = ref.coords(orc, pair.cam, kp1, pair.kp2, m)
        g12, votes, ok = fm3d.pose_from_epipolar(E, x1[mask], x2[mask], baseline)
        out.update(votes=votes, ok=ok)
        if not ok:
            return out
    out["g12"] = g12
    sct.set_g12(g12)
    sct.setKeypoints(kp1, pair.kp2, inl)
    pts, tmask = sct.triangulate()
    out.update(pts=pts, tmask=tmask)
    if normals:
        no = fm3d.NormalOptimizer(c, sct)
        no.setImages(pair.img1, pair.img2)
        _, nrm = no.computeOptimizedNormals(pts)
        keep = no.last_status == fm3d.ST_OK
        src = inl[tmask][keep]
        rec = np.zeros(int(keep.sum()), dtype=fm3d.RECORD)
        rec["queryIdx"], rec["trainIdx"], rec["distance"] = src["queryIdx"], src["trainIdx"], src["distance"]
        rec["status"] = fm3d.ST_OK
        rec["point"], rec["normal"] = pts[keep], nrm
        out["records"] = rec
    return out


def same_report(rep, want):
    assert rep["matches"] == len(want["m"])
    assert rep["best"] == want["best"]
    assert rep["verified"] == int(want["mask"].sum())
    assert rep["E"].tobytes() == want["E"].tobytes()
    assert np.array_equal(rep["votes"], want["votes"])
    assert rep["poseInstalled"] == 1 and rep["g12"].tobytes() == want["g12"].tobytes()


# ---------------------------------------------------------------- 1. the DLT leg over the shapes
@pytest.mark.parametrize("nA", [7, 8, 9, 1024, 1025, 2000])
def test_dlt_leg_shapes(fm3d, orc, pair, base, nA):
    """no model (7), the minimum (8, 9), one full tile of 1,024 matches, a second tile of one match, a
    ragged second tile with the distractors in it"""
    c, c2 = make_ctx(fm3d, pair), make_ctx(fm3d, pair)
    try:
        pipe = upload(fm3d, c, pair, nA, images=False)
        sct = fm3d.SingleCameraTriangulator(c)
        R0, t0 = sct.camera2()
        P, st, rep = pipe.run_dlt_verified(MAX_PX, hypotheses=64, seed=0, pose_from_model=True, baseline=base)
        want = composed(fm3d, orc, c2, pair, nA, 64, baseline=base)
        assert len(want["m"]) == nA
        R1, t1 = sct.camera2()
        if nA < 8:
            assert want["best"] == -1
            assert (rep["matches"], rep["verified"], rep["best"], rep["roundsAdopted"], rep["poseInstalled"]) == \
                (nA, 0, -1, 0, 0)
            assert not rep["E"].any() and not rep["votes"].any()
            assert P == 0 and st["matches"] == 0 and st["inliers"] == 0 and st["queries"] == nA
            assert R0.tobytes() == R1.tobytes() and t0.tobytes() == t1.tobytes()
            R, t = fm3d.camera2_from_g12(rep["g12"])
            assert R.tobytes() == R0.tobytes() and t.tobytes() == t0.tobytes()
            m, pts, _ = pipe.dlt_results(st["matches"], P)
            assert len(m) == 0 and len(pts) == 0
            return
        assert want["best"] >= 0 and want["ok"] and len(want["pts"]) >= 1  # the reference itself is not empty
        same_report(rep, want)
        assert st["matches"] == rep["verified"] and P == st["inliers"] == len(want["pts"])
        m, pts, src = pipe.dlt_results(st["matches"], P)
        assert m.tobytes() == want["inl"].tobytes()
        assert pts.tobytes() == want["pts"].tobytes()
        assert np.array_equal(src, np.nonzero(want["tmask"])[0])
        R, t = fm3d.camera2_from_g12(want["g12"])  # installed, and it stays
        assert R.tobytes() == R1.tobytes() and t.tobytes() == t1.tobytes()
    finally:
        c.close()
        c2.close()


# ---------------------------------------------------------------- 2. the full run without a pose
@pytest.mark.parametrize("refine", [0, 3])
def test_full_run_pose_free(fm3d, orc, pair, base, refine):
    c, c2 = make_ctx(fm3d, pair), make_ctx(fm3d, pair)
    try:
        pipe = upload(fm3d, c, pair)
        n, st, rep = pipe.run_verified(MAX_PX, hypotheses=512, seed=0, refine=refine, pose_from_model=True, baseline=base)
        rec = pipe.records(n).copy()
        want = composed(fm3d, orc, c2, pair, len(pair.desc1), 512, refine=refine, baseline=base, normals=True)
        same_report(rep, want)
        print("verified", rep["verified"], "of", rep["matches"], "rounds adopted", rep["roundsAdopted"], "votes",
              rep["votes"], "records", n, "verify_ms %.3f" % rep["verify_ms"])
        assert st["matches"] == rep["verified"] and st["inliers"] == len(want["pts"]) and st["kept"] == n
        assert n == len(want["records"]) and n > 100
        assert rec.tobytes() == want["records"].tobytes()
        m = want["m"]
        is_true = pair.true_train[m["queryIdx"]] == m["trainIdx"]
        assert 1700 <= is_true.sum() < len(m)
        assert (want["mask"] & is_true).sum() >= 0.99 * is_true.sum()
        # the pose stays installed
        R1, t1 = fm3d.SingleCameraTriangulator(c).camera2()
        R, t = fm3d.camera2_from_g12(rep["g12"])
        assert R.tobytes() == R1.tobytes() and t.tobytes() == t1.tobytes()
        # again, on the inputs as they lie: the same bytes
        n2, st2, rep2 = pipe.run_verified(MAX_PX, hypotheses=512, seed=0, refine=refine, pose_from_model=True,
                                          baseline=base)
        assert n2 == n and pipe.records(n2).tobytes() == rec.tobytes()
        for k in ("matches", "verified", "best", "roundsAdopted", "poseInstalled"):
            assert rep2[k] == rep[k]
        for k in ("votes", "E", "g12"):
            assert rep2[k].tobytes() == rep[k].tobytes()
    finally:
        c.close()
        c2.close()


# ---------------------------------------------------------------- 3., 4. under the known pose
@pytest.fixture(scope="module")
def plain(fm3d, pair):
    """fm3d_pipeline_run under the true pose, on a context of its own"""
    c = make_ctx(fm3d, pair, pair.g12)
    try:
        pipe = upload(fm3d, c, pair)
        n, st = pipe.run()
        return pipe.records(n).copy(), st
    finally:
        c.close()


def test_filter_mode(fm3d, orc, pair, plain):
    """pose_from_model = False: the plain run's records of the verified matches, byte for byte (a
    point's result does not depend on the others), and the pose untouched"""
    rec0, st0 = plain
    c, c2 = make_ctx(fm3d, pair, pair.g12), make_ctx(fm3d, pair)
    try:
        pipe = upload(fm3d, c, pair)
        sct = fm3d.SingleCameraTriangulator(c)
        R0, t0 = sct.camera2()
        n, st, rep = pipe.run_verified(MAX_PX, hypotheses=512, seed=0)
        rec = pipe.records(n)
        want = composed(fm3d, orc, c2, pair, len(pair.desc1), 512, g12=pair.g12)
        assert want["best"] >= 0 and 0 < want["mask"].sum() < len(want["m"])
        assert rep["matches"] == st0["matches"] == len(want["m"]) and rep["best"] == want["best"]
        assert rep["verified"] == st["matches"] == int(want["mask"].sum())
        assert rep["E"].tobytes() == want["E"].tobytes()
        assert rep["poseInstalled"] == 0 and not rep["votes"].any()
        assert rep["g12"].tobytes() == np.ascontiguousarray(pair.g12, dtype=np.float64).tobytes()
        pairs = set(zip(want["inl"]["queryIdx"].tolist(), want["inl"]["trainIdx"].tolist()))
        keep = np.array([(q, t) in pairs for q, t in zip(rec0["queryIdx"].tolist(), rec0["trainIdx"].tolist())])
        assert 0 < keep.sum() < len(rec0)
        assert n == keep.sum() and rec.tobytes() == rec0[keep].tobytes()
        m, pts, _ = pipe.dlt_results(st["matches"], st["inliers"])
        assert m.tobytes() == want["inl"].tobytes() and pts.tobytes() == want["pts"].tobytes()
        R1, t1 = sct.camera2()
        assert R0.tobytes() == R1.tobytes() and t0.tobytes() == t1.tobytes()
    finally:
        c.close()
        c2.close()


def test_gate_that_rejects_nothing(fm3d, pair, plain):
    rec0, st0 = plain
    c = make_ctx(fm3d, pair, pair.g12)
    try:
        pipe = upload(fm3d, c, pair)
        n, st, rep = pipe.run_verified(1e6, hypotheses=64, seed=0)
        assert rep["best"] >= 0 and rep["verified"] == rep["matches"] == st0["matches"]
        assert st["matches"] == st0["matches"] and st["inliers"] == st0["inliers"]
        assert n == len(rec0) and pipe.records(n).tobytes() == rec0.tobytes()
    finally:
        c.close()


# ---------------------------------------------------------------- 5. with the matcher's options, and the rules
def test_cross_check_filter_mode(fm3d, orc, pair):
    c, c2 = make_ctx(fm3d, pair, pair.g12, crossCheck=1), make_ctx(fm3d, pair)
    try:
        pipe = upload(fm3d, c, pair, images=False)
        P, st, rep = pipe.run_dlt_verified(MAX_PX, hypotheses=512, seed=0)
        mutual = fm3d.DescriptorsMatcher(c2).compareWithNNDRMutual(1.0, pair.desc1, pair.desc2, mode=1)
        assert rep["matches"] == len(mutual) and 8 <= rep["verified"] <= len(mutual)
        m, _, _ = pipe.dlt_results(st["matches"], P)
        assert len(m) == rep["verified"]
        sct = fm3d.SingleCameraTriangulator(c2)
        E, mask, inl, best = sct.verifyMatches(pair.kp1, pair.kp2, mutual, MAX_PX, hypotheses=512, seed=0)
        assert m.tobytes() == inl.tobytes() and rep["best"] == best and rep["E"].tobytes() == E.tobytes()
        have = set(zip(mutual["queryIdx"].tolist(), mutual["trainIdx"].tolist()))
        assert all((q, t) in have for q, t in zip(m["queryIdx"].tolist(), m["trainIdx"].tolist()))
    finally:
        c.close()
        c2.close()


def test_guided_match(fm3d, pair, base):
    c = make_ctx(fm3d, pair, pair.g12, guidedMatchPx=2.0)
    try:
        pipe = upload(fm3d, c, pair, images=False)
        K = pipe.run_dlt()[1]["matches"]
        P, st, rep = pipe.run_dlt_verified(MAX_PX, hypotheses=128, seed=0)
        assert rep["matches"] == K and rep["best"] >= 0 and 8 <= rep["verified"] <= K and P > 0
        with pytest.raises(fm3d.Fm3dError) as e:
            pipe.run_dlt_verified(MAX_PX, hypotheses=128, seed=0, pose_from_model=True, baseline=base)
        assert e.value.code == fm3d.ERR_INVALID and "guidedMatchPx" in str(e.value)
        with pytest.raises(fm3d.Fm3dError) as e:
            pipe.run_verified(MAX_PX, hypotheses=128, seed=0, pose_from_model=True, baseline=base)
        assert e.value.code == fm3d.ERR_INVALID and "guidedMatchPx" in str(e.value)
    finally:
        c.close()


def test_argument_rules(fm3d, pair, base):
    L = fm3d.lib()
    c = make_ctx(fm3d, pair, pair.g12)
    try:
        n, st, rep = ctypes.c_int(0), fm3d.PipelineStats(), fm3d.VerifyReport()

        def call(ctx=c.handle, rep=rep, null_opts=False, **kw):
            f = dict(hypotheses=64, refineIters=0, maxPx=1.0, seed=0, poseFromModel=0, reserved=0, baseline=base)
            f.update(kw)
            o = fm3d.VerifyOpts(**f)
            po = None if null_opts else ctypes.byref(o)
            pr = None if rep is None else ctypes.byref(rep)
            a = L.fm3d_pipeline_run_dlt_verified(ctx, po, ctypes.byref(n), ctypes.byref(st), pr)
            b = L.fm3d_pipeline_run_verified(ctx, po, None, ctypes.byref(n), ctypes.byref(st), pr)
            assert a == b
            return a

        assert call() == fm3d.ERR_INVALID  # nothing staged
        pipe = upload(fm3d, c, pair, 300, images=True)
        R0, t0 = fm3d.SingleCameraTriangulator(c).camera2()
        assert call() == fm3d.FM3D_OK and rep.best >= 0
        for kw in (dict(null_opts=True), dict(rep=None), dict(hypotheses=0), dict(hypotheses=-1), dict(refineIters=-1),
                   dict(refineIters=17), dict(maxPx=0.0), dict(maxPx=-1.0), dict(maxPx=float("nan")),
                   dict(maxPx=float("inf")), dict(reserved=1), dict(poseFromModel=2), dict(poseFromModel=-1),
                   dict(poseFromModel=1, baseline=0.0), dict(poseFromModel=1, baseline=float("nan")),
                   dict(poseFromModel=1, baseline=float("inf")), dict(poseFromModel=1, baseline=-1.0)):
            assert call(**kw) == fm3d.ERR_INVALID, kw
        assert call(hypotheses=(1 << 20) + 1) == fm3d.ERR_UNSUPPORTED
        assert call(poseFromModel=0, baseline=float("nan")) == fm3d.FM3D_OK  # the baseline is read only with the pose
        R1, t1 = fm3d.SingleCameraTriangulator(c).camera2()
        assert R0.tobytes() == R1.tobytes() and t0.tobytes() == t1.tobytes()
        # a share of the queries sees only its own matches
        pipe = upload(fm3d, c, pair, 300, images=True, query_offset=5)
        assert call() == fm3d.ERR_UNSUPPORTED
        assert b"queryOffset" in L.fm3d_last_error(c.handle)
        # a pending submit
        pipe = upload(fm3d, c, pair, 300, images=True)
        pipe.submit_dlt()
        assert call() == fm3d.ERR_INVALID
        P, _ = pipe.wait_dlt()
        assert P > 0 and call() == fm3d.FM3D_OK
    finally:
        c.close()


# ---------------------------------------------------------------- 6. nothing else moved
def test_plain_run_after_a_verified_run(fm3d, pair, base, plain):
    """the verified run leaves its pose, the swapped match buffer and its working memory behind: a
    fresh upload, the true pose and fm3d_pipeline_run give a fresh context's records"""
    rec0, st0 = plain
    c = make_ctx(fm3d, pair)
    try:
        pipe = upload(fm3d, c, pair)
        n, st, rep = pipe.run_verified(MAX_PX, hypotheses=128, seed=3, refine=2, pose_from_model=True, baseline=base)
        assert rep["poseInstalled"] == 1 and n > 0
        pipe.upload(pair.desc1, pair.desc2, pair.kp1, pair.kp2, pair.img1, pair.img2)
        fm3d.SingleCameraTriangulator(c).set_g12(pair.g12)
        n, st = pipe.run()
        assert st["matches"] == st0["matches"] and st["inliers"] == st0["inliers"]
        assert n == len(rec0) and pipe.records(n).tobytes() == rec0.tobytes()
        P, st = pipe.run_dlt()
        assert st["matches"] == st0["matches"] and P == st0["inliers"]
    finally:
        c.close()
