"""Cross-check matching on the GPU: mutual nearest neighbours (mode 1) and the
symmetric ratio test (mode 2) on top of NNDR, for every descriptor type and shape class, with and
without the epipolar gate, through the entry points, the pipeline and fm3d_mgpu.

The reference of every check is built here from the oracle: fwd = knn2(A, B), rev = knn2(B, A) (with
a gate: per row over the pairs the gate admits, `mask` forwards and `mask.T` backwards) and the
oracle's NNDR rule.  Every comparison is array_equal on queryIdx, trainIdx and distance."""
import ctypes

import numpy as np
import pytest

import f32_prefilter_pyref as pf
from conftest import oracle_threads

pytestmark = pytest.mark.gpu


# ---------------------------------------------------------------- the numpy restatement of the gate
# (tests/test_guided_match.py's helpers, restated)
def undistort_gpu(fm3d, ctx, kp):
    xy = np.ascontiguousarray(kp, dtype=np.float32).reshape(-1, 2).astype(np.float64)
    out = np.zeros_like(xy)
    if len(xy):
        p = ctypes.POINTER(ctypes.c_double)
        ctx.check(fm3d.lib().fm3d_undistort(ctx.handle, xy.ctypes.data_as(p), len(xy), out.ctypes.data_as(p)))
    return out


def essential_np(R2, t2):
    tx, ty, tz = (float(v) for v in t2)
    T = [[0.0, -tz, ty], [tz, 0.0, -tx], [-ty, tx, 0.0]]
    E = np.zeros((3, 3))
    for r in range(3):
        for c in range(3):
            E[r, c] = (T[r][0] * float(R2[0, c]) + T[r][1] * float(R2[1, c])) + T[r][2] * float(R2[2, c])
    return E


def lines_np(E, xy):
    x, y = xy[:, 0], xy[:, 1]
    with np.errstate(all="ignore"):
        l = [(E[k, 0] * x + E[k, 1] * y) + E[k, 2] for k in range(3)]
        n = np.sqrt(l[0] * l[0] + l[1] * l[1])
        abc = np.stack([l[0] / n, l[1] / n, l[2] / n], axis=1).astype(np.float32)
    out = np.zeros((len(xy), 4), dtype=np.float32)
    out[:, :3] = abc
    bad = (n == 0) | ~np.isfinite(abc).all(axis=1)
    out[bad] = (0, 0, np.inf, 0)
    return out


def gate_np(lines, uv32, tau):
    """(d, d <= tau): d = |((double)a*u + (double)b*v) + (double)c|, NaN fails"""
    a, b, c = (lines[:, k].astype(np.float64)[:, None] for k in range(3))
    u, v = (uv32[:, k].astype(np.float64)[None, :] for k in range(2))
    with np.errstate(all="ignore"):
        d = np.abs((a * u + b * v) + c)
        return d, d <= tau


def tau_of(settings, max_px):
    return max_px * 2.0 / (settings.Fx + settings.Fy)


def gate_of(fm3d, ctx, kp1, kp2, max_px):
    R2, t2 = fm3d.SingleCameraTriangulator(ctx).camera2()
    lines = lines_np(essential_np(R2, t2), undistort_gpu(fm3d, ctx, kp1))
    uv = undistort_gpu(fm3d, ctx, kp2).astype(np.float32)
    return gate_np(lines, uv, tau_of(ctx.settings, max_px))


def knn_ref(orc, A, B, typ, mask):
    """per query the oracle's knn2 over the rows inside the gate; (idx (nA, 2), dist (nA, 2))"""
    nA = A.shape[0]
    idx = np.full((nA, 2), -1, dtype=np.int32)
    dist = np.full((nA, 2), np.inf, dtype=np.float32)
    for i in range(nA):
        rows = np.flatnonzero(mask[i])
        if rows.size == 0:
            continue
        ii, dd = orc.knn2(A[i:i + 1], np.ascontiguousarray(B[rows]), typ, 1)
        ok = ii[0] >= 0
        idx[i, ok] = rows[ii[0][ok]]
        dist[i, ok] = dd[0][ok]
    return idx, dist


# ---------------------------------------------------------------- the cross-check's reference
def two_way(orc, A, B, typ, mask=None):
    """(fwd, rev): fwd[i] = query i's two nearest train rows, rev[j] = train row j's two nearest
    queries, both as (idx, dist) in the oracle's order (distance, index)"""
    if mask is None:
        t = oracle_threads()
        return orc.knn2(A, B, typ, t), orc.knn2(B, A, typ, t)
    return knn_ref(orc, A, B, typ, mask), knn_ref(orc, B, A, typ, np.ascontiguousarray(mask.T))


def mutual_ref(orc, fwd, rev, eps, mode):
    """fwd[i][0] is kept iff the forward NNDR rule holds, rev[train][0] is query i
    and (mode 2) rev[train] passes the same rule -> (queryIdx, trainIdx, distance) in query order"""
    q, t, d = orc.nndr(fwd[0], fwd[1], eps)
    keep = rev[0][t, 0] == q
    if mode == 2:
        rows, _, _ = orc.nndr(rev[0], rev[1], eps)  # the train rows whose own two neighbours pass
        keep &= np.isin(t, rows)
    return q[keep], t[keep], d[keep]


def assert_matches(out, ref):
    assert np.array_equal(out["queryIdx"], ref[0])
    assert np.array_equal(out["trainIdx"], ref[1])
    assert np.array_equal(out["distance"], ref[2])


MODES_EPS = [(1, 1.0), (2, 1.0), (1, 0.98), (2, 0.98)]

# ---------------------------------------------------------------- inputs
KINDS = {  # name -> (oracle type, dim, binary)
    "u8-128": (1, 128, False), "u8-64": (1, 64, False), "u8-100": (1, 100, False), "u8-256": (1, 256, False),
    "f32-128": (0, 128, False), "f32-64": (0, 64, False), "f32-36": (0, 36, False),
    "bits-32": (2, 32, True), "bits-64": (2, 64, True),
    # widths off the extractors' own: a 16-byte popcount scan, zero-padded binary rows, float rows with a
    # tail after FLANN's groups of four, byte rows padded to 256 (tests/test_gpu_match_widths.py)
    "bits-16": (2, 16, True), "bits-17": (2, 17, True), "bits-63": (2, 63, True),
    "f32-5": (0, 5, False), "f32-65": (0, 65, False), "u8-129": (1, 129, False), "u8-255": (1, 255, False),
}
SHAPES = [(1, 1), (1, 2), (2, 1), (33, 129), (129, 33), (300, 700), (700, 300), (300, 5000), (5000, 300)]
GUIDED_KINDS = ["u8-128", "u8-256", "f32-64", "f32-36", "bits-32", "bits-64"]
GUIDED_SHAPES = [(33, 129), (300, 700), (700, 300), (2000, 5000)]
WIDTH, HEIGHT = 640, 480


def descriptors(kind, nA, nB, seed):
    """rows over a 4-value alphabet of close values: few distinct distances, so equal ones are common
    on both sides and the lowest index must win them"""
    typ, dim, _ = KINDS[kind]
    rng = np.random.default_rng(seed)
    if typ == 1:
        alpha = np.array([100, 101, 102, 103], dtype=np.uint8)
    elif typ == 0:  # not integers: the rows stay on the float kernels (sums of sixteenths are exact)
        alpha = np.array([0.25, 0.5, 0.75, 1.0], dtype=np.float32)
    else:
        alpha = np.array([0x00, 0x01, 0x03, 0x07], dtype=np.uint8)
    return alpha[rng.integers(0, 4, (nA, dim))], alpha[rng.integers(0, 4, (nB, dim))]


def keypoints(nA, nB, seed=5):
    rng = np.random.default_rng(1000 * nA + nB + seed)
    k1 = np.stack([rng.uniform(0, WIDTH, nA), rng.uniform(0, HEIGHT, nA)], axis=1).astype(np.float32)
    k2 = np.stack([rng.uniform(0, WIDTH, nB), rng.uniform(0, HEIGHT, nB)], axis=1).astype(np.float32)
    return k1, k2


def make_ctx(fm3d, cam=None, g12=None, **fields):
    s = fm3d.Settings.default()
    if cam is not None:
        s.set_camera(cam)
    for k, v in fields.items():
        setattr(s, k, v)
    ctx = fm3d.Context(s, device=0)
    if g12 is not None:
        fm3d.SingleCameraTriangulator(ctx).set_g12(g12)
    return ctx


@pytest.fixture(scope="module")
def ctx(fm3d, synth):
    """the reference camera (width 640, distorted) and the reference g12"""
    c = make_ctx(fm3d, synth.Camera.reference(WIDTH), synth.reference_g12())
    yield c
    c.close()


_GATES = {}


def shape_gate(fm3d, ctx, nA, nB, max_px):
    """keypoints of a shape and their reference gate, computed once and shared by the types"""
    key = (nA, nB, max_px)
    if key not in _GATES:
        k1, k2 = keypoints(nA, nB)
        _, mask = gate_of(fm3d, ctx, k1, k2, max_px)
        mask.setflags(write=False)
        _GATES[key] = (k1, k2, mask)
    return _GATES[key]


# ---------------------------------------------------------------- 1. types x shapes, ungated
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
@pytest.mark.parametrize("kind", list(KINDS))
def test_types_and_shapes(fm3d, orc, ctx, kind, shape):
    """the transposed shapes swap which side forms query blocks, ragged last tiles and train parts:
    (300, 5000) splits the forward search into parts, (5000, 300) the reverse one"""
    nA, nB = shape
    typ, _, binary = KINDS[kind]
    a, b = descriptors(kind, nA, nB, 7)
    fwd, rev = two_way(orc, a, b, typ)
    dm = fm3d.DescriptorsMatcher(ctx, binary=binary)
    if min(nA, nB) >= 300:  # the cross-check removes some of the forward matches, not all of them
        plain = orc.nndr(fwd[0], fwd[1], 1.0)
        assert 0 < len(mutual_ref(orc, fwd, rev, 1.0, 1)[0]) < len(plain[0])
    for mode, eps in MODES_EPS:
        assert_matches(dm.compareWithNNDRMutual(eps, a, b, mode=mode), mutual_ref(orc, fwd, rev, eps, mode))


@pytest.mark.parametrize("kind", ["f32-64", "f32-128"])
def test_float_prefilter_route(fm3d, orc, ctx, kind):
    """float rows at 2^22 pairs and more take the bf16 prefilter in fm3d_knn2; at (1500, 3000) the
    forward and the reverse search both do, and both must return the exact scan's lists"""
    typ, _, binary = KINDS[kind]
    a, b = descriptors(kind, 1500, 3000, 8)
    fwd, rev = two_way(orc, a, b, typ)
    dm = fm3d.DescriptorsMatcher(ctx, binary=binary)
    assert 0 < len(mutual_ref(orc, fwd, rev, 1.0, 1)[0]) < len(orc.nndr(fwd[0], fwd[1], 1.0)[0])
    for mode, eps in MODES_EPS:
        assert_matches(dm.compareWithNNDRMutual(eps, a, b, mode=mode), mutual_ref(orc, fwd, rev, eps, mode))


def test_float_prefilter_correlated_rounding(fm3d, orc, ctx):
    """the mutual check consumes the forward search's first neighbour.  Rows whose bf16 rounding errors
    all push one way (tests/f32_prefilter_pyref.py): each such query's nearest row is b*, whose own
    nearest query is a short ordinary one, so the pair is dropped -- while the decoy that a too
    tight prefilter bound returns instead has that query as its nearest, and the pair would be kept"""
    a, b, queries, rows = pf.correlated_rounding_case(128, 2048, 2051, 12, seed=128)
    fwd, rev = two_way(orc, a, b, orc.F32)
    ref = mutual_ref(orc, fwd, rev, 1.0, 1)
    assert len(ref[0]) > 1000 and not np.isin(queries, ref[0]).any()
    assert (rev[0][rows[:, 1], 0] == queries).sum() >= 10
    out = fm3d.DescriptorsMatcher(ctx).compareWithNNDRMutual(1.0, a, b, mode=1)
    assert_matches(out, ref)


# ---------------------------------------------------------------- 2. ties
@pytest.mark.parametrize("kind", ["u8-128", "f32-64", "bits-32", "bits-64"])
def test_ties(fm3d, orc, ctx, kind):
    """A holds every row twice (copies i and i + n): both copies have the same forward list, the
    train row's nearest query is the lower copy"""
    typ, _, binary = KINDS[kind]
    n, nB = 150, 400
    half, b = descriptors(kind, n, nB, 12)
    a = np.concatenate([half, half])
    fwd, rev = two_way(orc, a, b, typ)
    dm = fm3d.DescriptorsMatcher(ctx, binary=binary)
    for mode, eps in MODES_EPS:
        out = dm.compareWithNNDRMutual(eps, a, b, mode=mode)
        assert_matches(out, mutual_ref(orc, fwd, rev, eps, mode))
        assert np.all(out["queryIdx"] < n)  # only the lower-index copy of a duplicated query survives
        assert len(np.unique(out["trainIdx"])) == len(out)  # a train row keeps at most one query
    assert len(dm.compareWithNNDRMutual(1.0, a, b, mode=1)) > 0
    # several queries share a forward best row here, so the second property is not vacuous
    t = orc.nndr(fwd[0], fwd[1], 1.0)[1]
    assert len(np.unique(t)) < len(t)


# ---------------------------------------------------------------- 3. degenerate sizes
@pytest.mark.parametrize("kind", ["u8-128", "f32-36", "bits-32", "bits-64"])
def test_degenerate_sizes(fm3d, orc, ctx, kind):
    typ, dim, binary = KINDS[kind]
    dm = fm3d.DescriptorsMatcher(ctx, binary=binary)
    a, b = descriptors(kind, 5, 40, 3)
    # one query: the reverse search has no second neighbour, so mode 2 keeps nothing
    assert len(dm.compareWithNNDRMutual(1.0, a[:1], b, mode=2)) == 0
    # ... and mode 1 keeps it iff NNDR does (it is every row's nearest query)
    for eps in (1.0, 0.98, 0.5):
        fwd = orc.knn2(a[:1], b, typ, 1)
        assert_matches(dm.compareWithNNDRMutual(eps, a[:1], b, mode=1), orc.nndr(fwd[0], fwd[1], eps))
    assert len(dm.compareWithNNDRMutual(1.0, a[:1], b, mode=1)) == 1
    # one train row: no forward second neighbour
    for mode in (1, 2):
        assert len(dm.compareWithNNDRMutual(1.0, a, b[:1], mode=mode)) == 0
        # empty sides: 0 matches, no launch error
        assert len(dm.compareWithNNDRMutual(1.0, a[:0], b, mode=mode)) == 0
        assert len(dm.compareWithNNDRMutual(1.0, a, b[:0], mode=mode)) == 0
        assert len(dm.compareWithNNDRMutual(1.0, a[:0], b[:0], mode=mode)) == 0
    k1, k2 = keypoints(5, 40)
    for mode in (1, 2):
        assert len(dm.compareWithNNDRMutualGuided(1.0, a[:0], b, k1[:0], k2, 8.0, mode=mode)) == 0
        assert len(dm.compareWithNNDRMutualGuided(1.0, a, b[:0], k1, k2[:0], 8.0, mode=mode)) == 0
    # the context still works
    fwd, rev = two_way(orc, a, b, typ)
    assert_matches(dm.compareWithNNDRMutual(1.0, a, b, mode=1), mutual_ref(orc, fwd, rev, 1.0, 1))


# ---------------------------------------------------------------- 4. guided
@pytest.mark.parametrize("shape", GUIDED_SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
@pytest.mark.parametrize("kind", GUIDED_KINDS)
def test_guided_types_and_shapes(fm3d, orc, ctx, kind, shape):
    nA, nB = shape
    typ, _, binary = KINDS[kind]
    k1, k2, mask = shape_gate(fm3d, ctx, nA, nB, 8.0)
    a, b = descriptors(kind, nA, nB, 7)
    fwd, rev = two_way(orc, a, b, typ, mask)
    if nA >= 300:  # the gate is neither empty nor everything here
        assert 0 < mask.sum() < mask.size // 4 and (fwd[0][:, 1] >= 0).sum() > nA // 2
        assert len(mutual_ref(orc, fwd, rev, 1.0, 1)[0]) > 0
    dm = fm3d.DescriptorsMatcher(ctx, binary=binary)
    for mode, eps in MODES_EPS:
        out = dm.compareWithNNDRMutualGuided(eps, a, b, k1, k2, 8.0, mode=mode)
        assert_matches(out, mutual_ref(orc, fwd, rev, eps, mode))


@pytest.mark.parametrize("kind", ["u8-128", "u8-256", "f32-36", "bits-64", "bits-32"])
def test_guided_boundary(fm3d, synth, orc, kind):
    """Fx = Fy = 1, Cx = Cy = 0, no distortion: tau == maxPx exactly.  maxPx = d of the pair (i0, j0)
    admits it in both searches, the next double towards 0 in neither: the transposed gate computes
    the forward gate's bits.  Row j0 copies query i0 (distance 0), so the pair is mutual whenever
    both directions see it, and query i0 loses its best row when they do not."""
    typ, _, binary = KINDS[kind]
    cam = synth.Camera(1.0, 1.0, 0.0, 0.0, (0.0, 0.0, 0.0, 0.0, 0.0))
    c = make_ctx(fm3d, cam, synth.reference_g12())
    try:
        rng = np.random.default_rng(9)
        nA, nB, i0, j0 = 5, 9, 3, 6
        k1 = rng.uniform(-0.5, 0.5, (nA, 2)).astype(np.float32)
        k2 = rng.uniform(-0.5, 0.5, (nB, 2)).astype(np.float32)
        a, b = descriptors(kind, nA, nB, 2)
        b[j0] = a[i0]
        d, _ = gate_of(fm3d, c, k1, k2, 1.0)
        d0 = float(d[i0, j0])
        assert np.isfinite(d0) and d0 > 0
        dm = fm3d.DescriptorsMatcher(c, binary=binary)
        for max_px, inside in ((d0, True), (float(np.nextafter(d0, 0.0)), False)):
            assert tau_of(c.settings, max_px) == max_px
            mask = d <= max_px
            assert bool(mask[i0, j0]) == inside
            fwd, rev = two_way(orc, a, b, typ, mask)
            assert (fwd[0][i0, 0] == j0) == inside and (rev[0][j0, 0] == i0) == inside
            for mode in (1, 2):
                out = dm.compareWithNNDRMutualGuided(1.0, a, b, k1, k2, max_px, mode=mode)
                assert_matches(out, mutual_ref(orc, fwd, rev, 1.0, mode))
                pair = (out["queryIdx"] == i0) & (out["trainIdx"] == j0)
                if not inside:
                    assert not pair.any()
            # mode 1 at epsilon 1: inside, (i0, j0) is kept whenever query i0 has a second candidate
            if inside and fwd[0][i0, 1] >= 0:
                out = dm.compareWithNNDRMutualGuided(1.0, a, b, k1, k2, max_px, mode=1)
                assert ((out["queryIdx"] == i0) & (out["trainIdx"] == j0)).any()
    finally:
        c.close()


@pytest.mark.parametrize("kind", ["u8-128", "f32-64", "bits-32", "bits-64"])
def test_huge_gate_is_ungated(fm3d, ctx, kind):
    k1, k2 = keypoints(300, 700)
    a, b = descriptors(kind, 300, 700, 4)
    dm = fm3d.DescriptorsMatcher(ctx, binary=KINDS[kind][2])
    for mode in (1, 2):
        plain = dm.compareWithNNDRMutual(1.0, a, b, mode=mode)
        guided = dm.compareWithNNDRMutualGuided(1.0, a, b, k1, k2, 1e9, mode=mode)
        assert len(plain) > 0 and plain.tobytes() == guided.tobytes()


# ---------------------------------------------------------------- 5. identity pose
def test_identity_pose_keeps_nothing(fm3d, synth):
    c = make_ctx(fm3d, synth.Camera.reference(WIDTH), np.eye(4))  # E = 0: no line, no admissible pair
    try:
        k1, k2 = keypoints(300, 700)
        for kind in ("u8-128", "f32-36", "bits-32", "bits-64"):
            a, b = descriptors(kind, 300, 700, 1)
            dm = fm3d.DescriptorsMatcher(c, binary=KINDS[kind][2])
            for mode in (1, 2):
                assert len(dm.compareWithNNDRMutualGuided(1.0, a, b, k1, k2, 8.0, mode=mode)) == 0, kind
    finally:
        c.close()


# ---------------------------------------------------------------- 6. decoys
@pytest.fixture(scope="module")
def pair(synth):
    return synth.make_frame_pair(2000, seed=11)


@pytest.fixture(scope="module")
def pair_orb(synth):
    return synth.make_frame_pair(2000, seed=11, desc="orb")


@pytest.mark.parametrize("desc", ["sift", "orb"])
def test_decoys(fm3d, orc, ctx, pair, pair_orb, desc):
    """epsilon = 1.0 lets every distractor through the ratio test; the cross-check removes them"""
    fp, typ, binary = (pair, orc.U8, False) if desc == "sift" else (pair_orb, orc.BITS, True)
    fwd, rev = two_way(orc, fp.desc1, fp.desc2, typ)
    ref = mutual_ref(orc, fwd, rev, 1.0, 1)
    true = np.flatnonzero(fp.true_train >= 0)
    distract = np.flatnonzero(fp.true_train < 0)
    assert len(orc.nndr(fwd[0], fwd[1], 1.0)[0]) == 2000 and len(distract) == 200
    got = dict(zip(ref[0].tolist(), ref[1].tolist()))
    assert all(got.get(int(i)) == int(fp.true_train[i]) for i in true)  # every true pair is kept
    assert np.isin(ref[0], distract).sum() <= 10
    out = fm3d.DescriptorsMatcher(ctx, binary=binary).compareWithNNDRMutual(1.0, fp.desc1, fp.desc2, mode=1)
    assert_matches(out, ref)


# ---------------------------------------------------------------- 7. pipeline
def pipe_settings(fm3d, cam, cross, px=0.0):
    s = fm3d.Settings.default()
    s.set_camera(cam)
    s.pixelsRay = 16
    s.guidedMatchPx = px
    if cross is not None:
        s.crossCheck = cross
    return s


@pytest.mark.parametrize("px", [0.0, 2.0], ids=["plain", "guided"])
@pytest.mark.parametrize("cross", [1, 2])
@pytest.mark.parametrize("desc", ["sift", "orb"])
def test_pipeline_dlt(fm3d, orc, pair, pair_orb, desc, cross, px):
    """run_dlt under Fm3d.crossCheck: the matches are the entry point's, the points the oracle DLT's"""
    fp, binary = (pair, False) if desc == "sift" else (pair_orb, True)
    c = fm3d.Context(pipe_settings(fm3d, fp.cam, cross, px), device=0)
    try:
        s = c.settings
        fm3d.SingleCameraTriangulator(c).set_g12(fp.g12)
        dm = fm3d.DescriptorsMatcher(c, binary=binary)
        if px > 0:
            want = dm.compareWithNNDRMutualGuided(s.nndrEpsilon, fp.desc1, fp.desc2, fp.kp1, fp.kp2, px, mode=cross)
        else:
            want = dm.compareWithNNDRMutual(s.nndrEpsilon, fp.desc1, fp.desc2, mode=cross)
        pipe = fm3d.Pipeline(c)
        pipe.upload(fp.desc1, fp.desc2, fp.kp1, fp.kp2, None, None, binary=binary)
        P, st = pipe.run_dlt()
        m, pts, _ = pipe.dlt_results(st["matches"], P)
        assert len(want) > 100 and st["matches"] == len(want)
        assert_matches(m, (want["queryIdx"], want["trainIdx"], want["distance"]))
        ref_pts, _ = orc.triangulate(fp.cam, fp.g12, s.zThresholdMin, s.zThresholdMax, fp.kp1, fp.kp2, m["queryIdx"],
                                     m["trainIdx"])
        assert P == len(ref_pts) > 0 and np.array_equal(pts, ref_pts)
    finally:
        c.close()


def full_run(fm3d, fp, cross):
    c = fm3d.Context(pipe_settings(fm3d, fp.cam, cross), device=0)
    try:
        fm3d.SingleCameraTriangulator(c).set_g12(fp.g12)
        pipe = fm3d.Pipeline(c)
        pipe.upload(fp.desc1, fp.desc2, fp.kp1, fp.kp2, fp.img1, fp.img2)
        n, st = pipe.run()
        return pipe.records(n), st
    finally:
        c.close()


@pytest.fixture(scope="module")
def full_cross1(fm3d, pair):
    return full_run(fm3d, pair, 1)


def test_pipeline_full_run(fm3d, orc, pair, full_cross1):
    """a whole run with crossCheck = 1: repeatable, and every record is a mutual pair"""
    rec, st = full_cross1
    again, _ = full_run(fm3d, pair, 1)
    assert len(rec) > 100 and rec.tobytes() == again.tobytes()
    eps = fm3d.Settings.default().nndrEpsilon
    fwd, rev = two_way(orc, pair.desc1, pair.desc2, orc.U8)
    q, t, _ = mutual_ref(orc, fwd, rev, eps, 1)
    assert st["matches"] == len(q)
    mutual = set(zip(q.tolist(), t.tolist()))
    assert all((int(r["queryIdx"]), int(r["trainIdx"])) in mutual for r in rec)


def test_pipeline_off_is_untouched(fm3d, pair):
    """crossCheck = 0 gives the records of a context that never heard of the field"""
    off, _ = full_run(fm3d, pair, 0)
    never, _ = full_run(fm3d, pair, None)
    assert len(off) > 100 and off.tobytes() == never.tobytes()


@pytest.mark.parametrize("block", [None, 256], ids=["block-default", "block-256"])
def test_pipeline_mgpu_one_device(fm3d, pair, full_cross1, block):
    """one device holds every query in order, whatever the share count"""
    one, _ = full_cross1
    kw = {} if block is None else {"block": block}
    mg = fm3d.MultiGPU(pipe_settings(fm3d, pair.cam, 1), devices=(0,), shares=4, **kw)
    try:
        mg.set_g12(pair.g12)
        mg.upload(pair.desc1, pair.desc2, pair.kp1, pair.kp2, pair.img1, pair.img2)
        rec, _ = mg.run()
    finally:
        mg.close()
    assert len(one) > 100 and rec.tobytes() == one.tobytes()


# ---------------------------------------------------------------- 8. argument errors
def test_argument_errors(fm3d, synth, ctx):
    L = fm3d.lib()
    inv = fm3d.ERR_INVALID
    a, b = descriptors("u8-128", 4, 6, 1)
    k1, k2 = keypoints(4, 6)
    out = np.zeros(4, dtype=fm3d.DMATCH)
    n = ctypes.c_int(0)
    vp = lambda x: ctypes.c_void_p(x.ctypes.data)
    dbl = ctypes.c_double

    def plain(c, A, B, mode, o=vp(out), cnt=ctypes.byref(n)):
        return L.fm3d_match_mutual(c.handle, A, 4, B, 6, 128, 1, dbl(0.6), mode, o, cnt)

    def guided(c, A, B, mode, kp1=vp(k1), kp2=vp(k2), px=2.0, o=vp(out), cnt=ctypes.byref(n)):
        return L.fm3d_match_mutual_guided(c.handle, A, 4, B, 6, 128, 1, kp1, kp2, dbl(0.6), dbl(px), mode, o, cnt)

    for f in (plain, guided):
        assert f(ctx, vp(a), vp(b), 1) == fm3d.FM3D_OK and f(ctx, vp(a), vp(b), 2) == fm3d.FM3D_OK
        for bad in (0, 3, -1, 7):
            assert f(ctx, vp(a), vp(b), bad) == inv
        assert f(ctx, None, vp(b), 1) == inv and f(ctx, vp(a), None, 1) == inv
        assert f(ctx, vp(a), vp(b), 1, o=None) == inv and f(ctx, vp(a), vp(b), 1, cnt=None) == inv
    assert guided(ctx, vp(a), vp(b), 1, kp1=None) == inv and guided(ctx, vp(a), vp(b), 1, kp2=None) == inv
    for bad in (0.0, -1.0, float("nan"), float("inf")):
        assert guided(ctx, vp(a), vp(b), 1, px=bad) == inv
    fresh = make_ctx(fm3d, synth.Camera.reference(WIDTH))  # g12 not set
    try:
        assert guided(fresh, vp(a), vp(b), 1) == inv
        assert plain(fresh, vp(a), vp(b), 1) == fm3d.FM3D_OK  # the unguided form needs no pose
    finally:
        fresh.close()


NULL_ARG = "null argument"
NO_POSE = "g12 not set (SingleCameraTriangulator::setg12)"
BAD_PX = "maxPx must be finite and > 0"
BAD_MODE = "mode must be 1 (mutual nearest) or 2 (symmetric ratio)"
# call -> (its arguments after the context, by name; the refusals: {argument: bad value} -> message, in the
# order the call checks them).  Every refusal is FM3D_ERR_INVALID; "nopose": on a context without g12
ONE_SHOT = {
    "fm3d_knn2": ("A nA B nB dim type out",
                  [({"A": None}, NULL_ARG), ({"B": None}, NULL_ARG), ({"out": None}, NULL_ARG)]),
    "fm3d_match_nndr": ("A nA B nB dim type eps out cnt",
                        [({"cnt": None}, NULL_ARG), ({"A": None}, NULL_ARG), ({"B": None}, NULL_ARG),
                         ({"out": None}, NULL_ARG)]),
    "fm3d_knn2_guided": ("A nA B nB dim type k1 k2 px out",
                         [({"A": None}, NULL_ARG), ({"B": None}, NULL_ARG), ({"out": None}, NULL_ARG),
                          ({"k1": None}, NULL_ARG), ({"k2": None}, NULL_ARG), ({"nopose": 1}, NO_POSE),
                          ({"nopose": 1, "px": 0.0}, NO_POSE), ({"nopose": 1, "A": None}, NULL_ARG),
                          ({"px": 0.0}, BAD_PX), ({"px": -1.0}, BAD_PX), ({"px": float("nan")}, BAD_PX),
                          ({"px": float("inf")}, BAD_PX)]),
    "fm3d_match_nndr_guided": ("A nA B nB dim type k1 k2 eps px out cnt",
                               [({"cnt": None}, NULL_ARG), ({"A": None}, NULL_ARG), ({"B": None}, NULL_ARG),
                                ({"out": None}, NULL_ARG), ({"k1": None}, NULL_ARG), ({"k2": None}, NULL_ARG),
                                ({"nopose": 1}, NO_POSE), ({"nopose": 1, "px": 0.0}, NO_POSE),
                                ({"nopose": 1, "k2": None}, NULL_ARG), ({"px": 0.0}, BAD_PX), ({"px": -1.0}, BAD_PX),
                                ({"px": float("nan")}, BAD_PX), ({"px": float("inf")}, BAD_PX)]),
    "fm3d_match_mutual": ("A nA B nB dim type eps mode out cnt",
                          [({"cnt": None}, NULL_ARG), ({"A": None}, NULL_ARG), ({"B": None}, NULL_ARG),
                           ({"out": None}, NULL_ARG), ({"mode": 0}, BAD_MODE), ({"mode": 3}, BAD_MODE),
                           ({"mode": 0, "out": None}, NULL_ARG)]),
    "fm3d_match_mutual_guided": ("A nA B nB dim type k1 k2 eps px mode out cnt",
                                 [({"cnt": None}, NULL_ARG), ({"A": None}, NULL_ARG), ({"B": None}, NULL_ARG),
                                  ({"out": None}, NULL_ARG), ({"k1": None}, NULL_ARG), ({"k2": None}, NULL_ARG),
                                  ({"mode": 0}, BAD_MODE), ({"mode": 3}, BAD_MODE), ({"mode": 0, "k1": None}, NULL_ARG),
                                  ({"nopose": 1}, NO_POSE), ({"nopose": 1, "mode": 0}, BAD_MODE),
                                  ({"nopose": 1, "px": 0.0}, NO_POSE), ({"px": 0.0}, BAD_PX), ({"px": -1.0}, BAD_PX),
                                  ({"px": float("nan")}, BAD_PX), ({"px": float("inf")}, BAD_PX),
                                  ({"mode": 3, "px": 0.0}, BAD_MODE)]),
}


@pytest.mark.parametrize("call", list(ONE_SHOT))
def test_one_shot_argument_table(fm3d, synth, ctx, call):
    """every null / maxPx / mode / missing-pose refusal of the six one-shot matchers, by code and message,
    and which comes first where two apply"""
    L = fm3d.lib()
    a, b = descriptors("u8-128", 4, 6, 1)
    k1, k2 = keypoints(4, 6)
    out = np.zeros((4, 2), dtype=fm3d.DMATCH)
    n = ctypes.c_int(0)
    vp = lambda x: ctypes.c_void_p(x.ctypes.data)
    good = {"A": vp(a), "nA": 4, "B": vp(b), "nB": 6, "dim": 128, "type": 1, "k1": vp(k1), "k2": vp(k2), "eps": 0.6,
            "px": 2.0, "mode": 1, "out": vp(out), "cnt": ctypes.byref(n)}
    names, refusals = ONE_SHOT[call]

    def run(c, **bad):
        args = dict(good, **bad)
        vals = [ctypes.c_double(args[k]) if k in ("eps", "px") else args[k] for k in names.split()]
        return getattr(L, call)(c.handle, *vals), L.fm3d_last_error(c.handle).decode()

    fresh = make_ctx(fm3d, synth.Camera.reference(WIDTH))  # g12 not set
    try:
        assert run(ctx)[0] == fm3d.FM3D_OK
        for bad, msg in refusals:
            bad = dict(bad)
            c = fresh if bad.pop("nopose", 0) else ctx
            assert run(c, **bad) == (fm3d.ERR_INVALID, msg), (call, bad)
    finally:
        fresh.close()
