"""Epipolar-guided matching on the GPU: the lines, the gated knn2 of every
descriptor type and shape class, NNDR, the pipeline under Fm3d.guidedMatchPx and the argument rules.

The reference of every knn check: the gate matrix in numpy fp64 from fm3d_undistort's outputs and
the contract's formulas, then per query the oracle's knn2 over the rows that pass, indices mapped
back to frame 2 -- bit-exact distances for all three types with no new oracle code."""
import ctypes

import numpy as np
import pytest

pytestmark = pytest.mark.gpu


# ---------------------------------------------------------------- the numpy restatement
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
    return lines, gate_np(lines, uv, tau_of(ctx.settings, max_px))


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


def assert_knn(m, idx, dist):
    assert m.shape == idx.shape
    assert np.array_equal(m["queryIdx"], np.repeat(np.arange(len(idx), dtype=np.int32)[:, None], 2, axis=1))
    assert np.array_equal(m["trainIdx"], idx)
    have = idx >= 0
    assert np.array_equal(m["distance"][have], dist[have])


def assert_nndr(orc, out, idx, dist, eps):
    q, t, d = orc.nndr(idx, dist, eps)
    assert np.array_equal(out["queryIdx"], q)
    assert np.array_equal(out["trainIdx"], t)
    assert np.array_equal(out["distance"], d)


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
NEW_KINDS = ["bits-16", "bits-17", "bits-63", "f32-5", "f32-65", "u8-129", "u8-255"]
SHAPES = [(1, 2), (33, 129), (300, 700), (2000, 5000)]
# the new widths: the shapes up to (300, 700), and (300, 5000), where every gated kernel splits the train
# rows into parts (the reference of (2000, 5000) is a per-query oracle call, seconds per kind)
NEW_KIND_SHAPES = [(1, 2), (33, 129), (300, 700), (300, 5000)]
KIND_SHAPES = [(k, s) for k in KINDS for s in (NEW_KIND_SHAPES if k in NEW_KINDS else SHAPES)]
WIDTH, HEIGHT = 640, 480


def descriptors(kind, nA, nB, seed):
    """rows over a 4-value alphabet of close values: few distinct distances, so equal ones are common
    and the lowest index must win them"""
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
        _, (_, mask) = gate_of(fm3d, ctx, k1, k2, max_px)
        mask.setflags(write=False)
        _GATES[key] = (k1, k2, mask)
    return _GATES[key]


# ---------------------------------------------------------------- 1. lines
def test_lines_bitwise(fm3d, synth, ctx):
    rng = np.random.default_rng(3)
    kp1 = np.stack([rng.uniform(0, WIDTH, 1000), rng.uniform(0, HEIGHT, 1000)], axis=1).astype(np.float32)
    sct = fm3d.SingleCameraTriangulator(ctx)
    got = sct.epipolar_lines(kp1)
    R2, t2 = sct.camera2()
    assert np.array_equal(fm3d.epipolar_matrix(synth.reference_g12()), essential_np(R2, t2))
    ref = lines_np(essential_np(R2, t2), undistort_gpu(fm3d, ctx, kp1))
    assert got.dtype == np.float32 and got.shape == (1000, 4)
    assert np.array_equal(got.view(np.uint32), ref.view(np.uint32))
    n = np.hypot(got[:, 0].astype(np.float64), got[:, 1].astype(np.float64))
    assert np.abs(n - 1).max() < 1e-6 and np.all(got[:, 3] == 0)


def test_identity_pose_passes_nothing(fm3d, synth):
    c = make_ctx(fm3d, synth.Camera.reference(WIDTH), np.eye(4))
    try:
        k1, k2 = keypoints(300, 700)
        lines = fm3d.SingleCameraTriangulator(c).epipolar_lines(k1)
        assert np.array_equal(lines, np.tile(np.array([0, 0, np.inf, 0], dtype=np.float32), (300, 1)))
        for kind in ("u8-128", "f32-36", "bits-32", "bits-64"):
            a, b = descriptors(kind, 300, 700, 1)
            dm = fm3d.DescriptorsMatcher(c, binary=KINDS[kind][2])
            m = dm.knn_match_guided(a, b, k1, k2, 8.0)
            assert np.all(m["trainIdx"] == -1), kind
            assert len(dm.compareWithNNDRGuided(1.0, a, b, k1, k2, 8.0)) == 0, kind
    finally:
        c.close()


# ---------------------------------------------------------------- 2. types and shapes
@pytest.mark.parametrize("kind,shape", KIND_SHAPES, ids=[f"{k}-{s[0]}x{s[1]}" for k, s in KIND_SHAPES])
def test_types_and_shapes(fm3d, orc, ctx, kind, shape):
    nA, nB = shape
    typ, _, binary = KINDS[kind]
    k1, k2, mask = shape_gate(fm3d, ctx, nA, nB, 8.0)
    a, b = descriptors(kind, nA, nB, 7)
    m = fm3d.DescriptorsMatcher(ctx, binary=binary).knn_match_guided(a, b, k1, k2, 8.0)
    idx, dist = knn_ref(orc, a, b, typ, mask)
    if nA >= 300:  # the gate is neither empty nor everything here
        assert 0 < mask.sum() < mask.size // 4 and (idx[:, 1] >= 0).sum() > nA // 2
    assert_knn(m, idx, dist)


# ---------------------------------------------------------------- 3. decoys
def test_decoys(fm3d, synth, orc):
    ref = synth.Camera.reference(WIDTH)
    cam = synth.Camera(ref.fx, ref.fy, ref.cx, ref.cy, (0.0, 0.0, 0.0, 0.0, 0.0))
    g12 = synth.reference_g12()
    R, t = g12[:3, :3], g12[:3, 3]
    rng = np.random.default_rng(21)
    P = np.zeros((0, 3))
    while len(P) < 600:  # 600 points at depth 1.6 .. 2.3 m, visible in both views
        uv = np.stack([rng.uniform(0, WIDTH, 2000), rng.uniform(0, HEIGHT, 2000)], axis=1)
        z = rng.uniform(1.6, 2.3, 2000)
        X = np.stack([(uv[:, 0] - cam.cx) / cam.fx * z, (uv[:, 1] - cam.cy) / cam.fy * z, z], axis=1)
        uv2 = synth.project(cam, X, R, t)
        ok = (uv2[:, 0] >= 0) & (uv2[:, 0] < WIDTH) & (uv2[:, 1] >= 0) & (uv2[:, 1] < HEIGHT) & ((X @ R.T + t)[:, 2] > 0.1)
        P = np.concatenate([P, X[ok]])
    P = P[:600]
    kp1 = synth.project(cam, P).astype(np.float32)
    kp2_true = synth.project(cam, P, R, t).astype(np.float32)
    c = make_ctx(fm3d, cam, g12)
    try:
        lines, _ = gate_of(fm3d, c, kp1, kp2_true, 0.25)
        # decoys: 40 px from query i's line along its normal (pixel units)
        nrm = np.stack([lines[:, 0] / cam.fx, lines[:, 1] / cam.fy], axis=1).astype(np.float64)
        nrm /= np.linalg.norm(nrm, axis=1, keepdims=True)
        kp2 = np.concatenate([(kp2_true.astype(np.float64) + 40.0 * nrm).astype(np.float32), kp2_true])
        desc1 = np.minimum(255, np.abs(rng.normal(0, 40, (600, 128)))).astype(np.int32)
        noisy = np.clip(desc1 + rng.integers(-8, 9, (600, 128)), 0, 255)
        d1 = desc1.astype(np.uint8)
        d2 = np.concatenate([d1, noisy.astype(np.uint8)])
        _, (d, mask) = gate_of(fm3d, c, kp1, kp2, 0.25)
        px = d * (cam.fx + cam.fy) / 2
        i = np.arange(600)
        assert px[i, 600 + i].max() < 1e-3 and px[i, i].min() > 39.9  # 0.25 px separates them with room
        dm = fm3d.DescriptorsMatcher(c)
        plain = dm.knn_match(d1, d2)
        guided = dm.knn_match_guided(d1, d2, kp1, kp2, 0.25)
        assert np.array_equal(plain["trainIdx"][:, 0], i) and np.all(plain["distance"][:, 0] == 0)
        assert np.array_equal(guided["trainIdx"][:, 0], 600 + i)
        assert_knn(plain, *orc.knn2(d1, d2, orc.U8, 1))
        assert_knn(guided, *knn_ref(orc, d1, d2, orc.U8, mask))
    finally:
        c.close()


# ---------------------------------------------------------------- 4. boundary
@pytest.mark.parametrize("kind", ["u8-128", "f32-36", "bits-64", "bits-32"])
def test_boundary(fm3d, synth, orc, kind):
    """Fx = Fy = 1, Cx = Cy = 0, no distortion: tau == maxPx exactly.  maxPx = d of one pair includes
    its row, the next double towards 0 excludes it."""
    typ, _, binary = KINDS[kind]
    cam = synth.Camera(1.0, 1.0, 0.0, 0.0, (0.0, 0.0, 0.0, 0.0, 0.0))
    c = make_ctx(fm3d, cam, synth.reference_g12())
    try:
        rng = np.random.default_rng(9)
        nA, nB, i0, j0 = 5, 9, 3, 6
        k1 = rng.uniform(-0.5, 0.5, (nA, 2)).astype(np.float32)
        k2 = rng.uniform(-0.5, 0.5, (nB, 2)).astype(np.float32)
        a, b = descriptors(kind, nA, nB, 2)
        b[j0] = a[i0]  # distance 0: the best row of query i0 whenever the gate lets it in
        _, (d, _) = gate_of(fm3d, c, k1, k2, 1.0)
        d0 = float(d[i0, j0])
        assert np.isfinite(d0) and d0 > 0
        dm = fm3d.DescriptorsMatcher(c, binary=binary)
        for max_px, inside in ((d0, True), (float(np.nextafter(d0, 0.0)), False)):
            assert tau_of(c.settings, max_px) == max_px
            mask = d <= max_px
            assert bool(mask[i0, j0]) == inside
            m = dm.knn_match_guided(a, b, k1, k2, max_px)
            assert_knn(m, *knn_ref(orc, a, b, typ, mask))
            assert (m["trainIdx"][i0, 0] == j0) == inside
    finally:
        c.close()


# ---------------------------------------------------------------- 5. huge gate
@pytest.mark.parametrize("kind", ["u8-128", "f32-64", "bits-32"])
def test_huge_gate_is_ungated(fm3d, ctx, kind):
    k1, k2 = keypoints(300, 700)
    a, b = descriptors(kind, 300, 700, 4)
    dm = fm3d.DescriptorsMatcher(ctx, binary=KINDS[kind][2])
    plain, guided = dm.knn_match(a, b), dm.knn_match_guided(a, b, k1, k2, 1e9)
    assert plain.tobytes() == guided.tobytes()
    p2, g2 = dm.compareWithNNDR(0.95, a, b), dm.compareWithNNDRGuided(0.95, a, b, k1, k2, 1e9)
    assert len(p2) > 0 and p2.tobytes() == g2.tobytes()


# ---------------------------------------------------------------- 6. NNDR
@pytest.mark.parametrize("kind", ["u8-128", "f32-64", "bits-32", "bits-64"])
def test_nndr_guided(fm3d, orc, ctx, kind):
    typ, _, binary = KINDS[kind]
    max_px, eps = 0.5, 0.95
    k1, k2, mask = shape_gate(fm3d, ctx, 300, 700, max_px)
    a, b = descriptors(kind, 300, 700, 6)
    out = fm3d.DescriptorsMatcher(ctx, binary=binary).compareWithNNDRGuided(eps, a, b, k1, k2, max_px)
    idx, dist = knn_ref(orc, a, b, typ, mask)
    single = np.flatnonzero(mask.sum(axis=1) == 1)
    assert single.size > 0 and np.all(idx[single, 0] >= 0) and np.all(idx[single, 1] < 0)
    assert not np.isin(single, out["queryIdx"]).any()  # one candidate on the line: dropped
    assert len(out) > 0
    assert_nndr(orc, out, idx, dist, eps)


# ---------------------------------------------------------------- 7. pipeline
@pytest.fixture(scope="module")
def pair(synth):
    return synth.make_frame_pair(2000, seed=11)


def guided_settings(fm3d, cam, px):
    s = fm3d.Settings.default()
    s.set_camera(cam)
    s.pixelsRay = 16
    s.guidedMatchPx = px
    return s


def run_dlt_checked(fm3d, orc, fp, typ, binary):
    c = fm3d.Context(guided_settings(fm3d, fp.cam, 2.0), device=0)
    try:
        sct = fm3d.SingleCameraTriangulator(c)
        sct.set_g12(fp.g12)
        _, (_, mask) = gate_of(fm3d, c, fp.kp1, fp.kp2, 2.0)
        idx, dist = knn_ref(orc, fp.desc1, fp.desc2, typ, mask)
        pipe = fm3d.Pipeline(c)
        pipe.upload(fp.desc1, fp.desc2, fp.kp1, fp.kp2, None, None, binary=binary)
        P, st = pipe.run_dlt()
        m, pts, _ = pipe.dlt_results(st["matches"], P)
        assert len(m) > 100
        assert_nndr(orc, m, idx, dist, c.settings.nndrEpsilon)
        sct.setKeypoints(fp.kp1, fp.kp2, m)
        ref_pts, _ = sct.triangulate()
        assert P == len(ref_pts) > 0 and np.array_equal(pts, ref_pts)
        # the gate changed the matches: the unguided pipeline keeps another list
        return m
    finally:
        c.close()


def test_pipeline_dlt_guided(fm3d, orc, pair):
    m = run_dlt_checked(fm3d, orc, pair, orc.U8, False)
    plain = orc.match_nndr(pair.desc1, pair.desc2, orc.U8, 0.55, 16)
    assert len(m) != len(plain[0]) or not np.array_equal(m["trainIdx"], plain[1])


def test_pipeline_dlt_guided_orb(fm3d, synth, orc):
    run_dlt_checked(fm3d, orc, synth.make_frame_pair(2000, seed=11, desc="orb"), orc.BITS, True)


def full_run(fm3d, fp, px):
    c = fm3d.Context(guided_settings(fm3d, fp.cam, px), device=0)
    try:
        fm3d.SingleCameraTriangulator(c).set_g12(fp.g12)
        pipe = fm3d.Pipeline(c)
        pipe.upload(fp.desc1, fp.desc2, fp.kp1, fp.kp2, fp.img1, fp.img2)
        n, _ = pipe.run()
        return pipe.records(n)
    finally:
        c.close()


def test_pipeline_huge_gate_records(fm3d, pair):
    off, huge = full_run(fm3d, pair, 0.0), full_run(fm3d, pair, 1e9)
    assert len(off) > 100 and off.tobytes() == huge.tobytes()


@pytest.mark.parametrize("block", [None, 256], ids=["block-default", "block-256"])
def test_pipeline_mgpu_guided(fm3d, pair, block):
    """shares of the queries (block 256: all four shares hold some) see their own queries' lines"""
    one = full_run(fm3d, pair, 2.0)
    kw = {} if block is None else {"block": block}
    mg = fm3d.MultiGPU(guided_settings(fm3d, pair.cam, 2.0), devices=(0,), shares=4, **kw)
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
    out = np.zeros((4, 2), dtype=fm3d.DMATCH)
    n = ctypes.c_int(0)
    vp = lambda x: ctypes.c_void_p(x.ctypes.data)
    dbl = ctypes.c_double

    def knn(c, kp1, kp2, px):
        return L.fm3d_knn2_guided(c.handle, vp(a), 4, vp(b), 6, 128, 1, kp1, kp2, dbl(px), vp(out))

    def nndr(c, kp1, kp2, px):
        return L.fm3d_match_nndr_guided(c.handle, vp(a), 4, vp(b), 6, 128, 1, kp1, kp2, dbl(0.6), dbl(px), vp(out),
                                        ctypes.byref(n))

    for f in (knn, nndr):
        assert f(ctx, vp(k1), vp(k2), 2.0) == fm3d.FM3D_OK
        assert f(ctx, None, vp(k2), 2.0) == inv and f(ctx, vp(k1), None, 2.0) == inv
        for bad in (0.0, -1.0, float("nan"), float("inf")):
            assert f(ctx, vp(k1), vp(k2), bad) == inv
    assert L.fm3d_epipolar_lines(ctx.handle, None, 4, vp(out)) == inv
    assert L.fm3d_epipolar_lines(ctx.handle, vp(k1), 4, None) == inv
    fresh = make_ctx(fm3d, synth.Camera.reference(WIDTH))  # g12 not set
    try:
        assert knn(fresh, vp(k1), vp(k2), 2.0) == inv and nndr(fresh, vp(k1), vp(k2), 2.0) == inv
        assert L.fm3d_epipolar_lines(fresh.handle, vp(k1), 4, vp(out)) == inv
    finally:
        fresh.close()
