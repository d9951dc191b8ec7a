"""Stage 4 on its rare branches, GPU side: csrc/fm3d_patch.hip (frames, the cvRodrigues2 round trip,
the patch export, square and circular neighbourhoods) against the oracle, bit for bit, on the case
table of tests/patch_cases.py -- both sides of every Rodrigues threshold, the half turn with and
without its sign flip, zero singular values, NaN / inf normals, z == 0, r^6 overflow, patches across
every border and samples exactly on it -- plus more frames than one grid.y holds, the zero guard after
the image on a context shrank, circular neighbourhoods with a normal in the image plane, and the
argument checks.  tests/test_patch_cases_oracle.py holds the oracle itself to a 50-digit restatement
on the same table; the rank-deficient and non-finite cases have no such reference and are pinned here
oracle-against-GPU only.

Every degenerate frame runs through the oracle on the CPU before it goes to the device: polar3 is one
shared header, so a frame whose zero-singular-value loop ends there ends in the kernel too.
"""
import numpy as np
import pytest

import patch_cases as pc

pytestmark = pytest.mark.gpu

CASES = pc.all_cases()


def _settings(fm3d, cam, **kw):
    s = fm3d.Settings.default()
    s.set_camera(cam)
    s.rodriguesIC = pc.RODRIGUES_IC
    for k, v in kw.items():
        setattr(s, k, v)
    return s


@pytest.fixture(scope="module")
def pair():
    p = pc.frame_pair()
    assert p.img1.shape == (pc.HEIGHT, pc.WIDTH) and p.img1.min() > 0
    return p


def _export_both_ways(fm3d, ctx, s, frames):
    sct = fm3d.SingleCameraTriangulator(ctx)
    ref_nbhd = fm3d.NeighborhoodsGenerator(s).getReferenceSquaredNeighborhood()
    patches, ipts = sct.projectReferencePointsToImageWithFrames(ref_nbhd, frames, image_points=True)
    alone = sct.projectReferencePointsToImageWithFrames(ref_nbhd, frames)
    assert alone.tobytes() == patches.tobytes()  # the imagePoints == nullptr launch
    return patches, ipts


@pytest.mark.parametrize("group", list(pc.GROUPS))
def test_case_table_bitwise(fm3d, orc, pair, group):
    """every case of the group in one context: computeFeaturesFrames of the frame cases, then the
    export of all frames, against the oracle's deterministic-math mode"""
    _, eps, cmpp, size = pc.GROUPS[group]
    cases = [c for c in CASES if c.group == group]
    cam = pc.group_camera(group, pair)
    s = _settings(fm3d, cam, neighEpsilon=eps, cmPerPixel=cmpp)
    ctx = fm3d.Context(s)
    try:
        no = fm3d.NormalOptimizer(ctx)
        no.setImages(pair.img1, pair.img2)
        g = no.getGravity()
        assert np.array_equal(g, orc.gravity(list(pc.RODRIGUES_IC)))
        assert g[0] == 0 and g[1] == -1 and abs(g[2]) < 1e-16  # the conditions of the CPU test's (0, -1, 0)
        pts, nrm = pc.case_normals(cases, g)
        if len(pts):
            row = {c.name: k for k, c in enumerate(c for c in cases if c.frame is None)}
            below = pc.gravity_cross_norm(g, nrm[row["n_below_eps"]])
            above = pc.gravity_cross_norm(g, nrm[row["n_above_eps"]])
            assert 0 < below < pc.DBL_EPSILON < above
            ref_ff = orc.features_frames(pts, nrm, g)
            ff = no.computeFeaturesFrames(pts, nrm)
            assert np.array_equal(ff, ref_ff, equal_nan=True)
            assert np.isnan(ff).any() and np.array_equal(ff[0, :3, :3], np.diag([-1.0, -1.0, 1.0]))
        else:
            ref_ff = np.zeros((0, 4, 4))
        frames = pc.frames_of(cases, ref_ff)
        ref_p, ref_pts = orc.export_patches(cam, pair.img1, frames, eps, cmpp, mode=orc.DETMATH, image_points=True)
        patches, ipts = _export_both_ways(fm3d, ctx, s, frames)
    finally:
        ctx.close()
    assert patches.shape == (len(cases), size, size)
    for k, c in enumerate(cases):
        assert np.array_equal(ipts[k], ref_pts[k], equal_nan=True), c.name
        assert patches[k].tobytes() == ref_p[k].tobytes(), c.name
    assert (patches > 0).any()


def _random_frames(n, seed):
    rng = np.random.default_rng(seed)
    a = rng.normal(size=(n, 3))
    a /= np.linalg.norm(a, axis=1, keepdims=True)
    th = rng.uniform(0, np.pi, n)
    K = np.zeros((n, 3, 3))
    K[:, 0, 1], K[:, 0, 2], K[:, 1, 0], K[:, 1, 2], K[:, 2, 0], K[:, 2, 1] = (-a[:, 2], a[:, 1], a[:, 2], -a[:, 0],
                                                                            -a[:, 1], a[:, 0])
    c, s = np.cos(th)[:, None, None], np.sin(th)[:, None, None]
    F = np.zeros((n, 4, 4))
    F[:, :3, :3] = c * np.eye(3) + (1 - c) * a[:, :, None] * a[:, None, :] + s * K
    F[:, :3, 3] = np.stack([rng.uniform(-0.6, 0.6, n), rng.uniform(-0.4, 0.4, n), rng.uniform(1.6, 2.3, n)], 1)
    F[:, 3, 3] = 1
    return F


def test_more_frames_than_one_grid_y(fm3d, orc, pair):
    """65,600 frames of 2 x 2 patches: launch_export_patches walks them in chunks of 65,535 (grid.y),
    the frames on either side of the seam take the rare branches (identity snap, half turn with the
    flip, exact half turn, a rank-1 frame); the same frames through the square neighbourhoods (4 points
    a frame, 64 frames a block)"""
    P, eps, cmpp = 65600, 0.015, 1.0
    frames = _random_frames(P, 5)
    frames[65534:65538] = pc.branch_frames()[[0, 1, 2, 4]]
    assert orc.patch_size(eps, cmpp) == 2
    ref_p, ref_pts = orc.export_patches(pair.cam, pair.img1, frames, eps, cmpp, mode=orc.DETMATH, image_points=True)
    ref_sq = orc.square_neighborhoods(frames, eps, cmpp)
    s = _settings(fm3d, pair.cam, neighEpsilon=eps, cmPerPixel=cmpp)
    ctx = fm3d.Context(s)
    try:
        fm3d.NormalOptimizer(ctx).setImages(pair.img1, pair.img2)
        patches, ipts = _export_both_ways(fm3d, ctx, s, frames)
        sq = fm3d.NeighborhoodsGenerator(s).computeSquareNeighborhoodsByNormals(ctx, frames)
    finally:
        ctx.close()
    assert (ref_p > 0).mean() > 0.5
    same_pts = (ipts == ref_pts) | (np.isnan(ipts) & np.isnan(ref_pts))
    bad = np.flatnonzero((patches != ref_p).any(axis=(1, 2)) | ~same_pts.all(axis=(1, 2)))
    assert bad.size == 0, bad[:8]  # the first frames that differ: 65535 and on if the seam is wrong
    assert np.array_equal(ipts, ref_pts, equal_nan=True)
    assert sq.shape == (P, 4, 3) and np.array_equal(sq, ref_sq)


# (first image, second image, camera of the exact-border cases at the second size): fx = fy and the
# principal point chosen so that the 8 x 8 grid of step 0.25 about the cases' translations lands on
# u == cols and v == rows of the SECOND image exactly
def _shrink_runs(img):
    half = np.ascontiguousarray(img[:240, :320])
    tall = np.ascontiguousarray(img.T)  # 480 wide, 640 high: the same area, another width
    return [
        ("shrink", img, [half], pc.pinhole(128.0, 128.0, 160.0, 120.0)),
        ("same_size_twice", img, [half, half], pc.pinhole(128.0, 128.0, 160.0, 120.0)),
        ("same_area_other_width", img, [tall], pc.pinhole(256.0, 256.0, 160.0, 400.0)),
    ]


@pytest.mark.parametrize("run", [0, 1, 2])
def test_guard_is_zero_after_the_image_changed_size(fm3d, orc, pair, run):
    """isPixelGood admits u == cols and v == rows, and the bilinear taps then read one column and one
    row past the image.  In a continuous cv::Mat followed by zeros (the oracle) a tap in column `cols`
    is the next row's first pixel, except in the last row, where it lies past the image like every tap
    of rows `rows` and `rows + 1`: those read zero.  The level buffers keep their size when the image
    shrinks, so the old image's pixels lie exactly where the new image's guard is; set_images_impl
    clears it when the size changed and relies on it staying clear when it did not."""
    name, first, then, cam = _shrink_runs(pair.img1)[run]
    eps, cmpp = 1.0, 25.0
    frames = np.array([pc.frame(np.eye(3), t) for t in pc.EXACT_T])
    s = _settings(fm3d, cam, neighEpsilon=eps, cmPerPixel=cmpp)
    ctx = fm3d.Context(s)
    try:
        no = fm3d.NormalOptimizer(ctx)
        no.setImages(first, first)
        got = []
        for img in then:
            no.setImages(img, img)
            got.append(_export_both_ways(fm3d, ctx, s, frames))
    finally:
        ctx.close()
    img = then[-1]
    h, w = img.shape
    ref_p, ref_pts = orc.export_patches(cam, img, frames, eps, cmpp, mode=orc.DETMATH, image_points=True)
    # the cases sit on the far borders of this image, and the taps past it read zero in the oracle
    assert (ref_pts[..., 0] == float(w)).any() and (ref_pts[..., 1] == float(h)).any()
    on_bottom = ref_pts[..., 1] == float(h)  # [frame, i*size + j]
    ref_by_point = np.transpose(ref_p, (0, 2, 1)).reshape(len(frames), -1)
    assert (ref_by_point[on_bottom] == 0).all()
    # u == cols above the last row: the next row's first pixel (x - floor(x) = 0: only the left taps count)
    on_right = (ref_pts[..., 0] == float(w)) & (ref_pts[..., 1] >= 0) & (ref_pts[..., 1] < h - 1)
    assert on_right.any()
    rows = ref_pts[..., 1][on_right].astype(int)  # the cases' v are integers
    assert np.array_equal(ref_by_point[on_right], img[rows + 1, 0])
    assert (ref_p > 0).any()
    for patches, ipts in got:
        assert np.array_equal(ipts, ref_pts), name
        assert patches.tobytes() == ref_p.tobytes(), name


CIRC_NORMALS = np.array([[1.0, 0.0, 0.0], [0.0, 1.0, 0.0], [0.0, 1.0, -0.0], [0.6, 0.8, 1e-300], [0.0, 0.0, 1.0]])
CIRC_EMPTY_POINTS = np.array([[0.0, 0.0, 0.0], [1.0, 1.0, 0.0]])


@pytest.mark.parametrize("thetas,rays", [(1, 1), (7, 3), (15, 5)])
def test_circular_neighborhoods_normal_in_the_image_plane(fm3d, orc, pair, thetas, rays):
    """the spanner is (0, 1, -n1/n2): n2 == 0, -0.0 or 1e-300 gives 0/0, +-inf or 1e300 there.  Given
    normals, and the empty-normals branch n = X/|X| with X = 0 and X in the plane z = 0; one point a
    call and 257 points (two blocks of samples and more)."""
    rng = np.random.default_rng(9)
    X = np.stack([rng.uniform(-0.6, 0.6, 257), rng.uniform(-0.4, 0.4, 257), rng.uniform(1.6, 2.3, 257)], 1)
    N = CIRC_NORMALS[np.arange(257) % len(CIRC_NORMALS)]
    Xe = X.copy()
    Xe[::3] = CIRC_EMPTY_POINTS[0]
    Xe[1::3] = CIRC_EMPTY_POINTS[1]
    s = _settings(fm3d, pair.cam, neighMethod=1, neighThetas=thetas, neighRays=rays)
    ctx = fm3d.Context(s)
    try:
        ng = fm3d.NeighborhoodsGenerator(s)
        runs = [(X, N), (Xe, None)] + [(X[k:k + 1], N[k:k + 1]) for k in range(len(CIRC_NORMALS))] + \
               [(Xe[k:k + 1], None) for k in range(3)]
        for pts, nrm in runs:
            ref = orc.circular_neighborhoods(pts, nrm, s.neighEpsilon, thetas, rays)
            got = ng.computeCircularNeighborhoodsByNormals(ctx, pts, nrm)
            assert got.shape == (len(pts), thetas * rays, 3)
            assert np.array_equal(np.isnan(got).any(axis=(1, 2)), np.isnan(ref).any(axis=(1, 2)))
            assert np.array_equal(got, ref, equal_nan=True)
            if len(pts) == 257:  # both kinds of row are there
                nan_rows = np.isnan(ref).any(axis=(1, 2))
                assert nan_rows.any() and not nan_rows.all()
    finally:
        ctx.close()


def test_empty_inputs_return_empty(fm3d, pair):
    s = _settings(fm3d, pair.cam, neighEpsilon=0.02, cmPerPixel=0.25, neighMethod=1)
    ctx = fm3d.Context(s)
    try:
        no = fm3d.NormalOptimizer(ctx)
        no.setImages(pair.img1, pair.img2)
        ng = fm3d.NeighborhoodsGenerator(s)
        assert no.computeFeaturesFrames(np.zeros((0, 3)), np.zeros((0, 3))).shape == (0, 4, 4)
        p, ip = fm3d.SingleCameraTriangulator(ctx).projectReferencePointsToImageWithFrames(
            None, np.zeros((0, 4, 4)), image_points=True)
        assert p.shape == (0, 16, 16) and ip.shape == (0, 256, 2)
        assert ng.computeSquareNeighborhoodsByNormals(ctx, np.zeros((0, 4, 4))).shape == (0, 256, 3)
        S = s.neighThetas * s.neighRays
        assert ng.computeCircularNeighborhoodsByNormals(ctx, np.zeros((0, 3))).shape == (0, S, 3)
    finally:
        ctx.close()


def test_export_before_set_images_is_an_error(fm3d, pair):
    s = _settings(fm3d, pair.cam, neighEpsilon=0.02, cmPerPixel=0.25)
    ctx = fm3d.Context(s)
    try:
        with pytest.raises(fm3d.Fm3dError) as e:
            fm3d.SingleCameraTriangulator(ctx).projectReferencePointsToImageWithFrames(None, [pc.frame(np.eye(3))])
        assert e.value.code == fm3d.ERR_INVALID
    finally:
        ctx.close()


def test_patch_size_zero_is_refused(fm3d, pair):
    s = _settings(fm3d, pair.cam, neighEpsilon=0.001, cmPerPixel=0.25)  # 2 * floor(0.4) = 0
    assert fm3d.NeighborhoodsGenerator(s).size() == 0
    ctx = fm3d.Context(s)
    try:
        fm3d.NormalOptimizer(ctx).setImages(pair.img1, pair.img2)
        for call in (lambda: fm3d.SingleCameraTriangulator(ctx).projectReferencePointsToImageWithFrames(
                         None, [pc.frame(np.eye(3))]),
                     lambda: fm3d.NeighborhoodsGenerator(s).computeSquareNeighborhoodsByNormals(
                         ctx, [pc.frame(np.eye(3))])):
            with pytest.raises(fm3d.Fm3dError) as e:
                call()
            assert e.value.code == fm3d.ERR_INVALID
    finally:
        ctx.close()
