"""The verified runs as submit / wait (DESIGN.md §3.1d "Submit / wait"): fm3d_pipeline_submit_verified /
_wait_verified and fm3d_pipeline_submit_dlt_verified / _wait_dlt_verified against the synchronous
fm3d_pipeline_run_verified / _run_dlt_verified on a second context, byte for byte.  The submit forms
size every launch of the verification by the staged nA and read the match count K on the device; the
synchronous call sizes them by K.  The pair and the contexts are test_gpu_pipeline_verified.py's
(verify_pyref.verify_inputs: 2,000 keypoints, the last 200 distractors; pixelsRay = 16, nndrEpsilon =
1.0 unless a case sets it), filter mode throughout."""
import ctypes

import numpy as np
import pytest

import verify_pyref as ref

pytestmark = pytest.mark.gpu

MAX_PX = 1.0
REP_INTS = ("matches", "verified", "best", "roundsAdopted", "poseInstalled")
REP_ARRAYS = ("votes", "E", "g12")
STAT_KEYS = ("queries", "trains", "matches", "inliers", "kept")


@pytest.fixture(scope="module")
def pair(synth):
    return ref.verify_inputs(synth)[0]


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


def result(n, st, rep, pipe, records=None):
    """everything the contract names, as comparable values"""
    out = {k: rep[k] for k in REP_INTS}
    out.update({k: rep[k].tobytes() for k in REP_ARRAYS})
    out.update({"st_" + k: st[k] for k in STAT_KEYS})
    out["n"] = n
    m, pts, src = pipe.dlt_results(st["matches"], st["inliers"])
    out.update(m=m.tobytes(), pts=pts.tobytes(), src=src.tobytes())
    if records is not None:
        out["records"] = records.tobytes()
    return out


def same(got, want):
    bad = [k for k in want if got[k] != want[k]]
    assert not bad and got.keys() == want.keys(), bad


_SYNC = {}


def sync_dlt(fm3d, pair, nA, H, refine, g12=None, **fields):
    """fm3d_pipeline_run_dlt_verified on a context of its own (once per case)"""
    key = ("dlt", nA, H, refine, g12 is not None, tuple(sorted(fields.items())))
    if key not in _SYNC:
        c = make_ctx(fm3d, pair, g12, **fields)
        try:
            pipe = upload(fm3d, c, pair, nA, images=False)
            P, st, rep = pipe.run_dlt_verified(MAX_PX, hypotheses=H, seed=0, refine=refine)
            _SYNC[key] = result(P, st, rep, pipe)
        finally:
            c.close()
    return _SYNC[key]


def sync_full(fm3d, pair, nA, H, refine, g12=None, **fields):
    """fm3d_pipeline_run_verified on a context of its own (once per case)"""
    key = ("full", nA, H, refine, g12 is not None, tuple(sorted(fields.items())))
    if key not in _SYNC:
        c = make_ctx(fm3d, pair, g12, **fields)
        try:
            pipe = upload(fm3d, c, pair, nA)
            n, st, rep = pipe.run_verified(MAX_PX, hypotheses=H, seed=0, refine=refine)
            _SYNC[key] = result(n, st, rep, pipe, pipe.records(n).copy())
        finally:
            c.close()
    return _SYNC[key]


def queued_dlt(fm3d, pair, nA, H, refine, g12=None, **fields):
    c = make_ctx(fm3d, pair, g12, **fields)
    try:
        pipe = upload(fm3d, c, pair, nA, images=False)
        pipe.submit_dlt_verified(MAX_PX, hypotheses=H, seed=0, refine=refine)
        P, st, rep = pipe.wait_dlt_verified()
        return result(P, st, rep, pipe)
    finally:
        c.close()


def submit_full(pipe, pair, nA, H, refine):
    pipe.submit_verified(pair.desc1[:nA], pair.desc2, pair.kp1[:nA], pair.kp2, pair.img1, pair.img2, MAX_PX,
                         hypotheses=H, seed=0, refine=refine)


def wait_full(pipe):
    rec, st, rep = pipe.wait_verified()
    return result(len(rec), st, rep, pipe, rec)


# ---------------------------------------------------------------- 1. the DLT leg over the shapes, K = nA
@pytest.mark.parametrize("nA, refine", [(7, 0), (8, 0), (9, 0), (1024, 0), (1025, 0), (2000, 0), (1025, 3), (2000, 3)])
def test_dlt_leg_shapes(fm3d, pair, nA, refine):
    """no model (7), the minimum (8, 9), one full tile of 1,024 matches, a second tile of one match, a
    ragged second tile with the distractors in it"""
    want = sync_dlt(fm3d, pair, nA, 64, refine)
    got = queued_dlt(fm3d, pair, nA, 64, refine)
    print(nA, refine, {k: got[k] for k in REP_INTS}, got["st_inliers"])
    assert want["matches"] == nA and want["st_queries"] == nA
    if nA < 8:
        assert (want["verified"], want["best"], want["n"], want["st_matches"], want["st_inliers"]) == (0, -1, 0, 0, 0)
        assert got["E"] == np.zeros(9).tobytes()
    else:
        assert want["best"] >= 0 and want["verified"] >= 8 and want["n"] >= 1  # the twin itself is not empty
    same(got, want)


# ---------------------------------------------------------------- 2. K < nA, with whole tiles past K
@pytest.mark.parametrize("fields, lo, hi", [(dict(nndrEpsilon=0.17), 8, 1024), (dict(nndrEpsilon=0.5), 1025, 1999),
                                            (dict(crossCheck=1), 1025, 1999)],
                         ids=["nndr0.17", "nndr0.5", "crosscheck"])
def test_count_below_the_bound(fm3d, pair, fields, lo, hi):
    """nA = 2000 sizes two tiles; the oracle's matcher keeps 714 matches at nndrEpsilon 0.17 (one tile,
    a second one all pad, a trailing tile for the solve), 1,800 at 0.5 and 1,802 mutual ones"""
    want = sync_dlt(fm3d, pair, 2000, 64, 3, **fields)
    assert lo <= want["matches"] <= hi and want["best"] >= 0 and want["verified"] >= 8 and want["n"] >= 1
    got = queued_dlt(fm3d, pair, 2000, 64, 3, **fields)
    print(fields, {k: got[k] for k in REP_INTS}, got["st_inliers"])
    same(got, want)


def test_oracle_counts_of_the_settings(orc, pair):
    """the K of case 2's settings by the oracle's matcher"""
    idx, dist = orc.knn2(pair.desc1, pair.desc2, orc.U8)
    assert [len(orc.nndr(idx, dist, e)[0]) for e in (0.17, 0.5)] == [714, 1800]


# ---------------------------------------------------------------- 3. the full path under the true pose
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


@pytest.mark.parametrize("refine", [0, 3])
def test_full_path(fm3d, pair, plain, refine):
    rec0, st0 = plain
    want = sync_full(fm3d, pair, 2000, 512, refine, g12=pair.g12)
    c = make_ctx(fm3d, pair, pair.g12)
    try:
        pipe = fm3d.Pipeline(c)
        sct = fm3d.SingleCameraTriangulator(c)
        R0, t0 = sct.camera2()
        submit_full(pipe, pair, 2000, 512, refine)
        rec, st, rep = pipe.wait_verified()
        got = result(len(rec), st, rep, pipe, rec)
        print("verified", rep["verified"], "of", rep["matches"], "rounds adopted", rep["roundsAdopted"], "records",
              len(rec), "verify_ms %.3f" % rep["verify_ms"], "total_ms %.3f" % st["total_ms"])
        same(got, want)
        assert len(rec) > 100 and rep["matches"] == st0["matches"] and 0 < rep["verified"] < rep["matches"]
        assert rep["verify_ms"] > 0 and st["total_ms"] > rep["verify_ms"]
        # the plain run's records of the verified matches (a point's result does not depend on the others)
        m, _, _ = pipe.dlt_results(st["matches"], st["inliers"])
        pairs = set(zip(m["queryIdx"].tolist(), m["trainIdx"].tolist()))
        keep = np.array([(q, t) in pairs for q, t in zip(rec0["queryIdx"].tolist(), rec0["trainIdx"].tolist())])
        assert 0 < keep.sum() < len(rec0)
        assert len(rec) == keep.sum() and rec.tobytes() == rec0[keep].tobytes()
        R1, t1 = sct.camera2()
        assert R0.tobytes() == R1.tobytes() and t0.tobytes() == t1.tobytes()
        assert rep["g12"].tobytes() == np.ascontiguousarray(pair.g12, dtype=np.float64).tobytes()
    finally:
        c.close()


# ---------------------------------------------------------------- 4. two contexts in flight, sizes swapped
def test_two_contexts_in_flight(fm3d, pair):
    """both submits before either wait; then the same contexts with the sizes swapped: the context that
    had 2,000 queries gets 1,025, so its pool holds an older pair's partials and flags past the new
    count"""
    want = {nA: sync_full(fm3d, pair, nA, 64, 3, g12=pair.g12) for nA in (1025, 2000)}
    a, b = make_ctx(fm3d, pair, pair.g12), make_ctx(fm3d, pair, pair.g12)
    try:
        pa, pb = fm3d.Pipeline(a), fm3d.Pipeline(b)
        for na, nb in ((1025, 2000), (2000, 1025), (1025, 2000)):
            submit_full(pa, pair, na, 64, 3)
            submit_full(pb, pair, nb, 64, 3)
            ga, gb = wait_full(pa), wait_full(pb)
            same(ga, want[na])
            same(gb, want[nb])
        # the DLT leg on the same contexts, a smaller count still: K = 714 of nA = 2000 needs settings of
        # its own, so here the staged size shrinks instead
        for pipe, nA in ((pa, 9), (pb, 1024)):
            pipe.upload(pair.desc1[:nA], pair.desc2, pair.kp1[:nA], pair.kp2, None, None)
        pa.submit_dlt_verified(MAX_PX, hypotheses=64, seed=0, refine=3)
        pb.submit_dlt_verified(MAX_PX, hypotheses=64, seed=0, refine=3)
        for pipe, nA in ((pb, 1024), (pa, 9)):
            P, st, rep = pipe.wait_dlt_verified()
            same(result(P, st, rep, pipe), sync_dlt(fm3d, pair, nA, 64, 3, g12=pair.g12))
    finally:
        a.close()
        b.close()


# ---------------------------------------------------------------- 5. the rules
INV, UNSUP = -1, -3
PENDING = (INV, "a submitted frame pair is pending: fm3d_pipeline_wait first")
LINK_PENDING = (INV, "a submitted frame pair is pending")
IS_VER = (INV, "a verified frame pair is pending: fm3d_pipeline_wait_verified")
IS_DLT_VER = (INV, "a verified front half is pending: fm3d_pipeline_wait_dlt_verified")
NO_VER = (INV, "no verified frame pair submitted (fm3d_pipeline_submit_verified)")
NO_DLT_VER = (INV, "no verified front half submitted (fm3d_pipeline_submit_dlt_verified)")
UPLOAD = (INV, "fm3d_pipeline_upload not called")
NEEDS_IDLE = ("upload", "run", "submit", "run_dlt", "submit_dlt", "submit_dlt_pair", "run_verified", "run_dlt_verified",
              "submit_verified", "submit_dlt_verified", "submit_ncc", "run_ncc", "ncc_results", "dlt_results")
N_RULES = 300


def refusal(fm3d, f):
    try:
        f()
    except fm3d.Fm3dError as e:
        return e.code, str(e).split(": ", 1)[1]
    return "accepted"


def call(fm3d, pipe, pair, col, others):
    nA = N_RULES
    full = (pair.desc1[:nA], pair.desc2, pair.kp1[:nA], pair.kp2, pair.img1, pair.img2)
    if col in ("upload", "submit"):
        return getattr(pipe, col)(*full)
    if col == "submit_verified":
        return pipe.submit_verified(*full, MAX_PX, hypotheses=64)
    if col == "submit_dlt_pair":
        return pipe.submit_dlt_pair(*full[:4])
    if col == "link":
        others.append(make_ctx(fm3d, pair, pair.g12))
        return pipe.link(fm3d.Pipeline(others[-1]))
    if col in ("run_verified", "run_dlt_verified", "submit_dlt_verified"):
        return getattr(pipe, col)(MAX_PX, hypotheses=64)
    if col == "ncc_results":
        return pipe.ncc_results(0, 16)
    if col == "dlt_results":
        return pipe.dlt_results(0, 0)
    return getattr(pipe, col)()


@pytest.mark.parametrize("kind", ["verified", "dlt_verified"])
def test_pending_state(fm3d, pair, kind):
    """every other pipeline call is refused while a verified pair is pending, the wrong waits with a
    message that names the right one; none of them disturbs the pending pair"""
    c, others = make_ctx(fm3d, pair, pair.g12), []
    try:
        pipe = fm3d.Pipeline(c)
        wrong = []
        for col, want in (("wait_verified", NO_VER), ("wait_dlt_verified", NO_DLT_VER),
                          ("submit_dlt_verified", UPLOAD)):  # fresh: nothing staged, nothing pending
            got = refusal(fm3d, lambda: call(fm3d, pipe, pair, col, others))
            if got != want:
                wrong.append(("fresh", col, got, want))
        if kind == "verified":
            submit_full(pipe, pair, N_RULES, 64, 3)
            want = sync_full(fm3d, pair, N_RULES, 64, 3, g12=pair.g12)
            table = {"wait": IS_VER, "wait_dlt": IS_VER, "wait_ncc": IS_VER, "wait_dlt_verified": IS_VER}
        else:
            pipe = upload(fm3d, c, pair, N_RULES, images=False)
            pipe.submit_dlt_verified(MAX_PX, hypotheses=64, seed=0, refine=3)
            want = sync_dlt(fm3d, pair, N_RULES, 64, 3, g12=pair.g12)
            table = {"wait": IS_DLT_VER, "wait_dlt": IS_DLT_VER, "wait_ncc": IS_DLT_VER, "wait_verified": IS_DLT_VER}
        table.update({col: PENDING for col in NEEDS_IDLE})
        table["link"] = LINK_PENDING
        for col, expect in table.items():
            got = refusal(fm3d, lambda: call(fm3d, pipe, pair, col, others))
            if got != expect:
                wrong.append((col, got, expect))
        print(kind, wrong)
        assert not wrong
        if kind == "verified":
            same(wait_full(pipe), want)
        else:
            P, st, rep = pipe.wait_dlt_verified()
            same(result(P, st, rep, pipe), want)
        # idle again: the waits have nothing, and a null report is refused before the state is looked at
        assert refusal(fm3d, pipe.wait_verified) == NO_VER and refusal(fm3d, pipe.wait_dlt_verified) == NO_DLT_VER
        L, n, st = fm3d.lib(), ctypes.c_int(0), fm3d.PipelineStats()
        assert L.fm3d_pipeline_wait_verified(c.handle, None, 0, ctypes.byref(n), ctypes.byref(st), None) == INV
        assert L.fm3d_pipeline_wait_dlt_verified(c.handle, ctypes.byref(n), ctypes.byref(st), None) == INV
    finally:
        c.close()
        for o in others:
            o.close()


def test_argument_rules(fm3d, pair):
    L = fm3d.lib()
    c, lead, memb = (make_ctx(fm3d, pair, pair.g12) for _ in range(3))
    vp = lambda a: ctypes.c_void_p(a.ctypes.data)
    nA = N_RULES
    d1, k1 = np.ascontiguousarray(pair.desc1[:nA]), np.ascontiguousarray(pair.kp1[:nA], dtype=np.float32)
    d2, k2 = np.ascontiguousarray(pair.desc2), np.ascontiguousarray(pair.kp2, dtype=np.float32)
    i1, i2 = np.ascontiguousarray(pair.img1), np.ascontiguousarray(pair.img2)
    h, w = i1.shape
    try:
        pipe = upload(fm3d, c, pair, nA)
        R0, t0 = fm3d.SingleCameraTriangulator(c).camera2()

        def call(ctx=c, null_opts=False, **kw):
            """both submits with the same options -> their common code; an accepted pair is waited for"""
            f = dict(hypotheses=64, refineIters=0, maxPx=1.0, seed=0, poseFromModel=0, reserved=0, baseline=1.0)
            f.update(kw)
            o = fm3d.VerifyOpts(**f)
            po = None if null_opts else ctypes.byref(o)
            n, st, rep = ctypes.c_int(0), fm3d.PipelineStats(), fm3d.VerifyReport()
            a = L.fm3d_pipeline_submit_dlt_verified(ctx.handle, po)
            if a == fm3d.FM3D_OK:
                assert L.fm3d_pipeline_wait_dlt_verified(ctx.handle, ctypes.byref(n), ctypes.byref(st),
                                                         ctypes.byref(rep)) == fm3d.FM3D_OK
            b = L.fm3d_pipeline_submit_verified(ctx.handle, po, vp(d1), nA, vp(d2), len(d2), 128, fm3d.DESC_U8, vp(k1),
                                                vp(k2), vp(i1), vp(i2), w, h)
            if b == fm3d.FM3D_OK:
                assert L.fm3d_pipeline_wait_verified(ctx.handle, None, 0, ctypes.byref(n), ctypes.byref(st),
                                                     ctypes.byref(rep)) == fm3d.FM3D_OK
                assert rep.best >= 0 and n.value > 0
            assert a == b
            return a, L.fm3d_last_error(ctx.handle).decode()

        assert call()[0] == fm3d.FM3D_OK
        for kw in (dict(null_opts=True), dict(hypotheses=0), dict(hypotheses=-1), dict(refineIters=-1),
                   dict(refineIters=17), dict(maxPx=0.0), dict(maxPx=-1.0), dict(maxPx=float("nan")),
                   dict(maxPx=float("inf")), dict(reserved=1), dict(poseFromModel=2), dict(poseFromModel=-1),
                   dict(poseFromModel=1, baseline=0.0), dict(poseFromModel=1, baseline=float("nan"))):
            assert call(**kw)[0] == INV, kw
        assert call(hypotheses=(1 << 20) + 1)[0] == UNSUP
        code, msg = call(poseFromModel=1, baseline=1.0)
        assert code == UNSUP and "synchronous" in msg and "fm3d_pipeline_run_verified" in msg
        assert call(poseFromModel=0, baseline=float("nan"))[0] == fm3d.FM3D_OK
        # every refusal left the context idle, and nothing moved the pose
        assert call()[0] == fm3d.FM3D_OK
        R1, t1 = fm3d.SingleCameraTriangulator(c).camera2()
        assert R0.tobytes() == R1.tobytes() and t0.tobytes() == t1.tobytes()
        # linked contexts: a member and a leader with a member
        upload(fm3d, lead, pair, nA)
        upload(fm3d, memb, pair, nA)
        fm3d.Pipeline(memb).link(fm3d.Pipeline(lead))
        for ctx in (memb, lead):
            code, msg = call(ctx=ctx)
            assert code == UNSUP and "fm3d_pipeline_link" in msg
        # a share of the queries sees only its own matches: the staged pair of submit_dlt_verified
        upload(fm3d, c, pair, nA, query_offset=5)
        o = fm3d.VerifyOpts(64, 0, 1.0, 0, 0, 0, 1.0)
        assert L.fm3d_pipeline_submit_dlt_verified(c.handle, ctypes.byref(o)) == UNSUP
        assert b"queryOffset" in L.fm3d_last_error(c.handle)
        assert refusal(fm3d, fm3d.Pipeline(c).wait_dlt_verified) == NO_DLT_VER  # nothing is pending
        # with guidedMatchPx the pose rule of the synchronous call comes first, as there
        g = make_ctx(fm3d, pair, pair.g12, guidedMatchPx=2.0)
        try:
            upload(fm3d, g, pair, nA)
            code, msg = call(ctx=g, poseFromModel=1)
            assert code == INV and "guidedMatchPx" in msg
        finally:
            g.close()
    finally:
        for x in (c, lead, memb):
            x.close()


def test_failed_submit_leaves_idle(fm3d, pair, plain):
    """a submit on a context that never got images: the LM refuses after the match half and the
    verification are queued.  Nothing is pending afterwards; a fresh upload and run give a fresh
    context's records, as after any verified submit / wait"""
    rec0, st0 = plain
    c = make_ctx(fm3d, pair, pair.g12)
    vp = lambda a: ctypes.c_void_p(a.ctypes.data)
    try:
        o = fm3d.VerifyOpts(64, 2, 1.0, 0, 0, 0, 1.0)
        rc = fm3d.lib().fm3d_pipeline_submit_verified(c.handle, ctypes.byref(o), vp(pair.desc1), 2000, vp(pair.desc2), 2000,
                                                      128, fm3d.DESC_U8, vp(pair.kp1), vp(pair.kp2), None, None, 0, 0)
        assert rc == INV
        assert fm3d.lib().fm3d_last_error(c.handle) == b"fm3d_set_images (NormalOptimizer::setImages) not called"
        pipe = fm3d.Pipeline(c)
        assert refusal(fm3d, pipe.wait_verified) == NO_VER
        submit_full(pipe, pair, 2000, 128, 2)
        rec, st, rep = pipe.wait_verified()
        assert rep["best"] >= 0 and 0 < len(rec) < len(rec0)
        pipe.upload(pair.desc1, pair.desc2, pair.kp1, pair.kp2, pair.img1, pair.img2)
        n, st = pipe.run()
        assert st["matches"] == st0["matches"] and st["inliers"] == st0["inliers"]
        assert n == len(rec0) and pipe.records(n).tobytes() == rec0.tobytes()
        P, st = pipe.run_dlt()
        assert st["matches"] == st0["matches"] and P == st0["inliers"]
    finally:
        c.close()


# ---------------------------------------------------------------- 6. with the epipolar gate
def test_guided_match(fm3d, pair):
    want = sync_dlt(fm3d, pair, 2000, 128, 0, g12=pair.g12, guidedMatchPx=2.0)
    assert want["best"] >= 0 and 8 <= want["verified"] <= want["matches"] <= 2000 and want["n"] > 0
    same(queued_dlt(fm3d, pair, 2000, 128, 0, g12=pair.g12, guidedMatchPx=2.0), want)
