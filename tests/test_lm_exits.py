"""The exits and border paths of the LM normal refinement that the well-behaved golden scenes never
reach (tests/golden/lm_exits.npz, written by tests/golden/make_golden.py make_lm_exits from the numpy /
scipy.optimize.leastsq restatement): every status 0..6, lmdif info 0..5, aborts below the coarsest
level, neighbourhoods trimmed to 1..3 pixels, an odd image size, a NaN plane point.  CPU only: the
oracle in its three modes against the fixture.  lmdif's info 6, 7, 8 cannot occur with ftol = xtol =
gtol = 30 eps: the tests for info 1 to 4 use the larger tolerance and fire first."""
import os

import numpy as np
import pytest

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
SCENES = ("border", "odd", "flat_equal", "flat_diff", "flat_step", "flat_sat", "noise", "special", "nanplane")


class Cam:
    def __init__(self, arr):
        self.fx, self.fy, self.cx, self.cy = arr[:4]
        self.k = tuple(arr[4:9])


@pytest.fixture(scope="module")
def fx():
    with np.load(os.path.join(GOLDEN, "lm_exits.npz"), allow_pickle=False) as z:
        return {k: z[k] for k in z.files}


def scene(fx, name):
    return {k[len(name) + 1:]: v for k, v in fx.items() if k.startswith(name + "_")}


def run_oracle(orc, fx, name, mode):
    s = scene(fx, name)
    cam = Cam(s.get("cam", fx["cam"]))  # the nanplane scene has a camera of its own
    return s, orc.optimize_normals(cam, s["R2"], s["t2"], s["img1"], s["img2"], int(s["levels"]), s["points"],
                                   int(s["ray"]), int(s["bound"][0]), int(s["bound"][1]), mode=mode, nthreads=2)


def ran_info(info, status):
    """lmdif's info of the levels that ran: every level of a kept point, the levels above the
    aborting one of an aborted point (NO_PIXELS runs none)"""
    out = []
    for i, code in zip(info, status):
        out += list(i) if code == 0 else list(i[int(np.nonzero(i < 0)[0][0]) + 1:]) if code > 1 else []
    return np.array(out)


def test_fixture_reaches_every_exit(fx):
    """The generator's reach conditions on the committed file: every scene is needed by one of them."""
    st = np.concatenate([fx[f"{s}_status"] for s in SCENES])
    assert (np.bincount(np.concatenate([st, fx["plane_status"].ravel()]), minlength=7)[:7] >= 3).all()
    assert (np.bincount(st, minlength=7) >= 3).all()  # and through the LM
    info = np.concatenate([ran_info(fx[f"{s}_info"], fx[f"{s}_status"]) for s in SCENES])
    for code in range(6):
        assert (info == code).sum() >= 3, code
    assert not np.isin(info, (6, 7, 8)).any()
    st, inf, nf, m = (fx[f"border_{k}"] for k in ("status", "info", "nfev", "mdat"))
    assert ((st == 3) & (inf[:, -1] == -3) & (nf[:, -1] == 1)).sum() >= 3   # PIX1 at the coarsest level
    assert (st == 1).sum() >= 3 and (m[st == 1] == 0).all()                   # NO_PIXELS
    m1 = m == 1                                                               # m < n: info 0, no evaluation, kept
    assert m1.sum() >= 2 and (st[m1] == 0).all() and (inf[m1] == 0).all() and (nf[m1] == 0).all()
    assert (m == 2).any() and (m == 3).any()
    st, inf, nf = (fx[f"odd_{k}"] for k in ("status", "info", "nfev"))
    fine = (st == 3) & (inf[:, 0] == -3) & (inf[:, 1:] > 0).all(1) & (nf[:, 1:] > 2).all(1)
    assert fine.sum() >= 3                                                    # PIX1 at level 0 only
    assert (st == 0).sum() >= 3
    for s in ("flat_equal", "flat_diff", "flat_step", "flat_sat"):
        assert (fx[f"{s}_info"] == 4).sum() >= 3, s
    assert ((fx["noise_info"] == 5) & (fx["noise_nfev"] >= 300)).sum() >= 3   # maxfev
    assert (fx["special_status"] == 6).sum() >= 3 and (fx["special_status"] == 2).sum() >= 2
    assert (fx["nanplane_status"] == 5).sum() >= 3
    for code in (0, 2, 5):
        assert (fx["plane_status"] == code).sum() >= 3, code
    total = sum(len(fx[f"{s}_status"]) for s in SCENES)
    assert total < 400


def assert_normals(r, s, tol):
    """normals of the kept points, and the carried normal of a point that aborted below the
    coarsest level (where the fixture holds one), within tol"""
    have = ~np.isnan(s["normals"]).any(1)
    sel = have & ((s["status"] == 0) | (s["info"][:, -1] > 0))
    if sel.any():
        assert np.abs(r["normals"][sel] - s["normals"][sel]).max() < tol
    kept_nan = (s["status"] == 0) & ~have
    assert np.isnan(r["normals"][kept_nan]).any(1).all()


@pytest.mark.parametrize("name", SCENES)
def test_oracle_strict_vs_scipy(orc, fx, name):
    s, r = run_oracle(orc, fx, name, orc.STRICT)
    L = int(s["levels"]) + 1
    assert np.array_equal(r["status"], s["status"])
    assert np.array_equal(r["info"][:, :L], s["info"])
    assert np.array_equal(r["nfev"][:, :L], s["nfev"])
    assert np.array_equal(r["mdat"], s["mdat"])
    assert_normals(r, s, 1e-12)


@pytest.mark.parametrize("name", SCENES)
def test_oracle_detmath_and_tree_vs_scipy(orc, fx, name):
    """DETMATH (the GPU contract) keeps status, info, nfev and, within 1e-12, the normals; the tree mode
    keeps status and info (its normals' distance is printed, not bounded)."""
    s, det = run_oracle(orc, fx, name, orc.DETMATH)
    _, tree = run_oracle(orc, fx, name, orc.DETMATH | orc.TREE | orc.GRAM)
    L = int(s["levels"]) + 1
    for r in (det, tree):
        assert np.array_equal(r["status"], s["status"])
        assert np.array_equal(r["info"][:, :L], s["info"])
    assert np.array_equal(det["nfev"][:, :L], s["nfev"])
    assert_normals(det, s, 1e-12)
    ok = (s["status"] == 0) & ~np.isnan(s["normals"]).any(1)
    if ok.any():
        print(f"{name}: tree mode max |n - n_scipy| {np.abs(tree['normals'][ok] - s['normals'][ok]).max():.3g}")


def test_noise_scene_modes_agree(orc, fx):
    """A condition on the noise scene's seed and points, not a tolerance: libm's and the correctly
    rounded transcendentals take the same path through all 300 evaluations, code for code."""
    _, a = run_oracle(orc, fx, "noise", orc.STRICT)
    _, b = run_oracle(orc, fx, "noise", orc.DETMATH)
    for k in ("status", "info", "nfev"):
        assert np.array_equal(a[k], b[k]), k


def test_plane_to_image2_codes_vs_numpy(orc, fx):
    """orc_plane_to_image2 on the in-plane normals: the centre ray's 0/0 is NAN_PLANE, every other
    pixel leaves the bounding box; a fourth plane leaves it on one side only.  Codes and uv equal the
    numpy restatement's (the same operations in the same order)."""
    p = scene(fx, "plane")
    cam = Cam(fx["cam"])
    pix = orc.neighborhood(cam, p["X"], int(p["ray"]), int(p["bound"][0]), int(p["bound"][1]))
    assert np.array_equal(pix, p["pix"])
    for n, uv, st in zip(p["normals"], p["uv"], p["status"]):
        ruv, rst = orc.plane_to_image2(cam, fx["border_R2"], fx["border_t2"], p["X"], n, pix, 2.4,
                                       size=tuple(int(v) for v in p["size"]))
        assert np.array_equal(rst, st)
        assert np.array_equal(ruv, uv, equal_nan=True)  # the same operations in the same order
