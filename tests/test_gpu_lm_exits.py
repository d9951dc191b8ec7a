"""The LM kernel on the exit and border scenes of tests/golden/lm_exits.npz (tests/test_lm_exits.py pins
the oracle to that fixture on the CPU): every status 0..6, lmdif info 0..5, aborts below the coarsest
level, neighbourhoods of 1..3 pixels, the 157 x 119 pair whose coarse levels gather column w_L and
row h_L.  Bit for bit against the DETMATH oracle on the same inputs (the tree oracle for
lmReduction = 1), and code for code against the scipy fixture; plus plane_to_image2 and nccHypotheses
on the same scenes and a queue of mostly immediate exits."""
import os

import numpy as np
import pytest

from conftest import oracle_threads
from test_lm_exits import GOLDEN, SCENES, Cam, scene

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def fx():
    with np.load(os.path.join(GOLDEN, "lm_exits.npz"), allow_pickle=False) as z:
        return {k: z[k] for k in z.files}


def _g12(R2, t2):
    g = np.eye(4)
    g[:3, :3] = R2
    g[:3, 3] = t2
    return g


class _Session:
    """a context with the scene's settings, pose and images"""

    def __init__(self, fm3d, fx, s, **kw):
        st = fm3d.Settings.default()
        st.set_camera(Cam(s.get("cam", fx["cam"])))
        st.pixelsRay, st.pyramids = int(s["ray"]), int(s.get("levels", 2))
        st.boundWidth, st.boundHeight = int(s["bound"][0]), int(s["bound"][1])
        for k, v in kw.items():
            setattr(st, k, v)
        self.ctx = fm3d.Context(st)
        try:
            self.sct = fm3d.SingleCameraTriangulator(self.ctx)
            self.sct.set_g12(_g12(s["R2"], s["t2"]))
            self.R2, self.t2 = self.sct.camera2()
            self.no = fm3d.NormalOptimizer(self.ctx, self.sct)
            self.no.setImages(s["img1"], s["img2"])
        except Exception:
            self.ctx.close()
            raise

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.ctx.close()


def _lm_vs_oracle(fm3d, orc, fx, s, P, tree):
    cam = Cam(s.get("cam", fx["cam"]))
    L = int(s["levels"]) + 1
    with _Session(fm3d, fx, s, lmReduction=1 if tree else 0) as g:
        kept, normals = g.no.computeOptimizedNormals(P)
        st, info, nfev = g.no.last_status, g.no.last_info, g.no.last_nfev
        R2, t2 = g.R2, g.t2
    ref = orc.optimize_normals(cam, R2, t2, s["img1"], s["img2"], L - 1, P, int(s["ray"]), int(s["bound"][0]),
                               int(s["bound"][1]), mode=orc.DETMATH | (orc.TREE | orc.GRAM if tree else 0),
                               nthreads=oracle_threads())
    assert np.array_equal(st, ref["status"])
    assert np.array_equal(info[:, :L], ref["info"][:, :L])
    assert np.array_equal(nfev[:, :L], ref["nfev"][:, :L])
    ok = ref["status"] == 0
    assert np.array_equal(kept, np.asarray(P, float)[ok], equal_nan=True)
    assert np.array_equal(normals, ref["normals"][ok], equal_nan=True)
    return st, info[:, :L], nfev[:, :L]


@pytest.mark.parametrize("path", ["default", "safe", "tree"])
@pytest.mark.parametrize("name", SCENES)
def test_exit_scene_bitwise_vs_oracle(fm3d, orc, fx, name, path, monkeypatch):
    monkeypatch.setenv("FM3D_LM_SAFE", "1" if path == "safe" else "0")
    monkeypatch.setenv("FM3D_LM_MAX_SECONDS", "20")
    s = scene(fx, name)
    st, info, nfev = _lm_vs_oracle(fm3d, orc, fx, s, s["points"], path == "tree")
    assert np.array_equal(st, s["status"])    # the scipy fixture's codes
    assert np.array_equal(info, s["info"])
    if path != "tree":
        assert np.array_equal(nfev, s["nfev"])


def test_strict_nan_exit_fails_the_call(fm3d, fx, monkeypatch):
    """strictNanExit = 1: a NAN_PLANE point makes computeOptimizedNormals fail (the reference's
    exit(-6)); without it the point is dropped with status 5 (the nanplane case above)."""
    monkeypatch.setenv("FM3D_LM_MAX_SECONDS", "20")
    s = scene(fx, "nanplane")
    assert (s["status"] == 5).any()
    with _Session(fm3d, fx, s, strictNanExit=1) as g:
        with pytest.raises(fm3d.Fm3dError):
            g.no.computeOptimizedNormals(s["points"])
        kept, _ = g.no.computeOptimizedNormals(s["points"][s["status"] != 5])  # the context goes on working
        assert len(kept) == int((s["status"] == 0).sum())


@pytest.mark.parametrize("coop", [0, 1])
def test_queue_of_immediate_exits(fm3d, orc, fx, coop, monkeypatch):
    """5,000 points of which three quarters leave after one pass (NO_PIXELS, ABORT_PIX1 at the coarsest
    level, NAN_NORMAL), interleaved with points that run every level: the slots refetch from the queue
    after a single pass, with and without the tail help."""
    monkeypatch.setenv("FM3D_LM_COOP", str(coop))
    monkeypatch.setenv("FM3D_LM_MAX_SECONDS", "30")
    b, sp = scene(fx, "border"), scene(fx, "special")
    full = b["mdat"] == 113
    good = b["points"][(b["status"] == 0) & full]
    lists = [b["points"][b["status"] == 1], b["points"][(b["status"] == 3) & full], sp["points"][sp["status"] == 6]]
    assert len(good) >= 3 and all(len(v) >= 3 for v in lists)
    rng = np.random.default_rng(17)
    P = np.empty((5000, 3))
    for i in range(len(P)):
        src = good if i % 4 == 3 else lists[i % 4]
        P[i] = src[(i // 4) % len(src)]
        if i % 4 == 3:
            P[i] *= 1 + 1e-3 * rng.normal()
    st, info, nfev = _lm_vs_oracle(fm3d, orc, fx, b, P, False)
    quick = (st == 1) | (st == 6) | ((st == 3) & (nfev[:, -1] == 1))
    assert quick.mean() >= 0.74 and (st == 0).sum() > 500
    for code in (1, 3, 6):
        assert (st == code).sum() >= 1000


def test_plane_to_image2_codes(fm3d, orc, fx):
    p, b = scene(fx, "plane"), scene(fx, "border")
    s = dict(b, ray=p["ray"], bound=p["bound"])
    assert tuple(p["size"]) == b["img1"].shape[::-1]
    with _Session(fm3d, fx, s) as g:
        got = [g.sct.plane_to_image2(p["X"], n) for n in p["normals"]]
        R2, t2 = g.R2, g.t2
    for (xy, uv, st), n, fst in zip(got, p["normals"], p["status"]):
        assert np.array_equal(xy, p["pix"])
        ruv, rst = orc.plane_to_image2(Cam(fx["cam"]), R2, t2, p["X"], n, p["pix"], 2.4,
                                       size=tuple(int(v) for v in p["size"]))
        assert np.array_equal(st, rst) and np.array_equal(uv, ruv, equal_nan=True)
        assert np.array_equal(st, fst)  # the numpy restatement's codes


@pytest.mark.parametrize("name", ["flat_equal", "flat_diff", "flat_step", "flat_sat", "odd"])
def test_ncc_hypotheses_flat_and_odd(fm3d, orc, fx, name):
    s = scene(fx, name)
    with _Session(fm3d, fx, s) as g:
        sc, nb, b = g.no.nccHypotheses(s["points"], 4, 4, 0.4)
        R2, t2 = g.R2, g.t2
    rs, rn, rb = orc.ncc_hypotheses(Cam(fx["cam"]), R2, t2, s["img1"], s["img2"], s["points"], int(s["ray"]), 4, 4,
                                    0.4, bound=(int(s["bound"][0]), int(s["bound"][1])))
    assert np.array_equal(sc, rs) and np.array_equal(b, rb) and np.array_equal(nb, rn, equal_nan=True)
    if name == "odd":
        assert (b >= 0).sum() >= 3 and (sc == -2).any()  # scored patches, and ones that leave an image
    elif name != "flat_step":
        assert (sc == -2).all() and (b == -1).all()  # a flat patch has no variance: no score
