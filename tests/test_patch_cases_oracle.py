"""Stage 4 on its rare branches, CPU side: the oracle's patch export (orc_features_frames,
orc_frame_camera's cvRodrigues2 round trip, orc_project1, the border rule) on every case of
tests/patch_cases.py against tests/patch_pyref.py, an independent 50-digit restatement.  The GPU side
(tests/test_gpu_patch_cases.py) then holds csrc/fm3d_patch.hip to the oracle bit for bit on the same
table, so a branch that is wrong in both the same way -- the kernel and the oracle restate one
OpenCV function -- is caught here.

Bounds (tests/patch_cases.py has the reasoning): image points within 1e-9 px, the figure
test_features_frames_and_patches_vs_numpy uses; 1e-6 px within 1e-5 rad of a half turn.  A wrong sign
or a wrong branch moves points by whole pixels.  Rank-deficient and non-finite frames have no unique
polar factor: for them only the two oracle modes' NaN pattern is compared.

Measured oracle-against-pyref maxima (px, the larger of the two modes), per branch: identity snap
5.7e-14 (R = I exactly on both sides; the rest is the projection's own rounding), generic 4.7e-11
(small_angle_1.1e-05, where acos near +1 is at its worst; 5.7e-14 for the 1.1 rad rotation), half
turn without the flip 3.5e-9 (pi_minus_1e-07; 5.7e-14 for the exact half turns), half turn with the
flip 4.4e-8 (half_yz_flip: the double polar factor leaves R00 + 1 = 1e-16 where it is 0, an axis
tilted by 1e-8 rad).
"""
import numpy as np
import pytest

import patch_cases as pc
import patch_pyref

pytest.importorskip("mpmath")

CASES = pc.all_cases()
BY_NAME = {c.name: c for c in CASES}


@pytest.fixture(scope="module")
def table(orc):
    """per group: the cases, their frames (frame cases through orc.features_frames with g = (0, -1, 0))
    and the oracle's patches and image points in both modes"""
    pair = pc.frame_pair()
    assert pair.img1.shape == (pc.HEIGHT, pc.WIDTH) and pair.img1.min() > 0
    out = {}
    for group, (_, eps, cmpp, size) in pc.GROUPS.items():
        cases = [c for c in CASES if c.group == group]
        assert orc.patch_size(eps, cmpp) == size
        pts, nrm = pc.case_normals(cases, pc.GRAVITY)
        ff = orc.features_frames(pts, nrm, pc.GRAVITY) if len(pts) else np.zeros((0, 4, 4))
        frames = pc.frames_of(cases, ff)
        cam = pc.group_camera(group, pair)
        res = {m: orc.export_patches(cam, pair.img1, frames, eps, cmpp, mode=m, image_points=True)
               for m in (orc.STRICT, orc.DETMATH)}
        out[group] = dict(cases=cases, frames=frames, cam=cam, res=res, eps=eps, cmpp=cmpp, size=size)
    return out


def _of(table, name):
    c = BY_NAME[name]
    g = table[c.group]
    k = [x.name for x in g["cases"]].index(name)
    return c, g, k


def test_table_names_unique_and_complete():
    assert len(BY_NAME) == len(CASES)
    assert {c.group for c in CASES} == set(pc.GROUPS)
    # each rare condition has its cases: the half turn with the flip, a zero singular value, a patch
    # straddling each border and corner, samples exactly on the border
    assert BY_NAME["half_yz_flip"].branch == patch_pyref.HALF_FLIP
    assert {c.name for c in CASES if c.zero_sv} >= {"n_gravity", "n_2.5_gravity", "n_minus_gravity", "n_zero",
                                                    "n_1e-200", "n_below_eps"}
    assert sum(c.border for c in CASES) == 8 and sum(bool(c.exact) for c in CASES) == 3
    assert {c.tol for c in CASES} == {1e-9, 1e-6}
    for c in CASES:  # the looser bound: half-turn branch only (within 1e-5 rad of pi), and at eps <= 0.02 only
        assert c.tol == 1e-9 or (c.branch in (patch_pyref.HALF, patch_pyref.HALF_FLIP)
                                 and pc.GROUPS[c.group][1] <= 0.02), c.name
    assert BY_NAME["pi_minus_1.1e-05"].tol == 1e-9 and BY_NAME["small_angle_1.1e-05"].tol == 1e-9


def test_normalize_threshold_both_sides():
    """the two normals built to straddle normalize3's s > DBL_EPSILON do"""
    below = pc.gravity_cross_norm(pc.GRAVITY, BY_NAME["n_below_eps"].normal(pc.GRAVITY))
    above = pc.gravity_cross_norm(pc.GRAVITY, BY_NAME["n_above_eps"].normal(pc.GRAVITY))
    assert 0 < below < pc.DBL_EPSILON < above < 1.5 * pc.DBL_EPSILON, (below, above)


@pytest.mark.parametrize("name", [c.name for c in CASES if c.rank == pc.FULL])
def test_oracle_vs_pyref(orc, table, name):
    c, g, k = _of(table, name)
    size = g["size"]
    # the whole 16 x 16 or 8 x 8 grid; of a 128 x 128 one every 37th point and the four corners
    index = list(range(size * size)) if size <= 16 else sorted(set(range(0, size * size, 37)) |
                                                                {0, size - 1, size * (size - 1), size * size - 1})
    ref, branch = patch_pyref.image_points(g["cam"], g["frames"][k], g["eps"], g["cmpp"], size, index)
    assert branch == c.branch, (name, branch)
    assert np.isfinite(ref).all()
    worst = 0.0
    for mode in (orc.STRICT, orc.DETMATH):
        got = g["res"][mode][1][k][index]
        worst = max(worst, float(np.abs(got - ref).max()))
    print(f"{name}: branch {branch}, oracle - pyref max {worst:.3g} px (bound {c.tol:g})")
    assert worst <= c.tol, (name, worst)
    # STRICT against DETMATH patches: at most one level (a truncation flip of the float sample)
    d = np.abs(g["res"][orc.STRICT][0][k].astype(int) - g["res"][orc.DETMATH][0][k].astype(int))
    assert d.max() <= 1


@pytest.mark.parametrize("name", [c.name for c in CASES if c.rank != pc.FULL])
def test_degenerate_cases_end_and_modes_agree(orc, table, name):
    """no unique SVD, nothing to hold the values to: the run ended (the table fixture returned) and
    both oracle modes put their NaNs in the same places"""
    c, g, k = _of(table, name)
    a, b = g["res"][orc.STRICT][1][k], g["res"][orc.DETMATH][1][k]
    assert np.array_equal(np.isnan(a), np.isnan(b))
    F = g["frames"][k]
    if c.rank == pc.NONFINITE:
        assert np.isnan(a).any()
        # a NaN pixel is never good: its patch byte is 0
        for mode in (orc.STRICT, orc.DETMATH):
            p, pts = g["res"][mode][0][k], g["res"][mode][1][k]
            bad = np.isnan(pts).any(axis=1).reshape(g["size"], g["size"])  # point (i, j) -> patch[j, i]
            assert (p.T[bad] == 0).all()
    if c.zero_sv:
        assert np.isfinite(F).all()
        w, _, _ = orc.cv_svd(F[:3, :3])
        assert w.min() <= pc.DBL_MIN, (name, w)
    elif c.rank == pc.DEFICIENT:
        pytest.fail("a rank-deficient case must say how")


def test_r6_overflow_case_overflows_r6_only(orc, table):
    """the case built for cvProjectPoints2's icdist2 = NaN: NaNs exactly in grid row j = 8, off the
    column X = 0 (where x = 0 and the point is the principal point)"""
    c, g, k = _of(table, "r6_overflow")
    size = g["size"]
    nan = np.isnan(g["res"][orc.DETMATH][1][k]).any(axis=1).reshape(size, size)  # [i, j]
    want = np.zeros((size, size), bool)
    want[:, 8] = True
    want[8, 8] = False
    assert np.array_equal(nan, want)


def test_plane_through_centre_has_z_zero_samples(orc, table):
    """z == 0 exactly in row j = 8 of plane_through_centre: project1's z ? 1/z : 1 gives u = fx X + cx"""
    c, g, k = _of(table, "plane_through_centre")
    size, cam = g["size"], g["cam"]
    pts = g["res"][orc.DETMATH][1][k].reshape(size, size, 2)
    X = -g["eps"] + g["cmpp"] * 0.01 * np.arange(size)
    assert np.array_equal(pts[:, 8, 0], X * cam.fx + cam.cx)


@pytest.mark.parametrize("name", [c.name for c in CASES if c.border])
def test_border_cases_straddle(orc, table, name):
    c, g, k = _of(table, name)
    share = float(pc.inside(g["res"][orc.DETMATH][1][k]).mean())
    print(f"{name}: inside share {share:.3f}")
    assert 0.1 <= share <= 0.9, (name, share)


def test_distorted_camera_cannot_reach_left_border_or_corners(orc):
    """why the left border and the corners use the camera without distortion: up to the radius where
    the synthetic camera's distorted radius r (1 + k1 r^2 + k2 r^4 + k3 r^6) peaks and the projection
    folds back, no point projects onto or past the left border, nor past two borders at once"""
    cam = pc.frame_pair().cam
    k1, k2, _, _, k3 = cam.k
    r = np.linspace(0.0, 2.0, 20001)
    rd = r * (1 + k1 * r ** 2 + k2 * r ** 4 + k3 * r ** 6)
    peak = int(np.argmax(rd))
    assert 0 < peak < len(r) - 1 and (np.diff(rd[:peak + 1]) > 0).all()  # monotone up to an inner peak
    assert abs(rd[peak] - 0.949) < 1e-3 and 339 < rd[peak] * cam.fx < 341
    x, y = np.meshgrid(np.arange(-r[peak], r[peak], 0.004), np.arange(-r[peak], r[peak], 0.004))
    keep = x * x + y * y <= r[peak] ** 2
    P = np.stack([x[keep], y[keep], np.ones(int(keep.sum()))], axis=1)
    uv = orc.project(cam, np.eye(3), np.zeros(3), P)
    u, v = uv[:, 0], uv[:, 1]
    print(f"distorted camera: peak radius {rd[peak] * cam.fx:.1f} px, leftmost u {u.min():.2f}")
    assert u.min() > 1.0  # the left border stays more than a pixel away (the grid's step is 1.4 px)
    assert not (((u <= 0) | (u >= pc.WIDTH)) & ((v <= 0) | (v >= pc.HEIGHT))).any()  # no corner
    assert (u >= pc.WIDTH).any() and (v <= 0).any() and (v >= pc.HEIGHT).any()  # the other three borders are reached


@pytest.mark.parametrize("name", [c.name for c in CASES if c.exact])
def test_exact_border_cases_sit_on_the_border(orc, table, name):
    c, g, k = _of(table, name)
    for mode in (orc.STRICT, orc.DETMATH):
        pts = g["res"][mode][1][k]
        for axis, value in c.exact:
            col = pts[:, 0 if axis == "u" else 1]
            assert (col == value).any(), (name, axis, value)
        assert np.array_equal(pts, np.round(pts / 32) * 32)  # no rounding anywhere: multiples of 32
    # a sample on u == cols or v == rows is good, and reads zeros past the image: v == rows gives 0
    p, pts = g["res"][orc.DETMATH]
    on_bottom = (pts[k][:, 1] == float(pc.HEIGHT)).reshape(g["size"], g["size"])
    if on_bottom.any():
        assert (p[k].T[on_bottom] == 0).all()


def test_frame_cases_fronto_parallel_is_the_exact_half_turn(orc, table):
    """gravity (0, -1, 0) and the fronto-parallel normal give diag(-1, -1, 1): the half-turn branch is
    no corner case"""
    c, g, k = _of(table, "n_fronto")
    assert np.array_equal(g["frames"][k][:3, :3], np.diag([-1.0, -1.0, 1.0]))
