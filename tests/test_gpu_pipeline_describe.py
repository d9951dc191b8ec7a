"""fm3d_pipeline_describe (csrc/fm3d_tail.cpp): the tail of main.cpp:157-183 in one call on points and
normals that lie on the device, against (a) the chain of one-shot wrappers it replaces --
computeFeaturesFrames, projectReferencePointsToImageWithFrames, extractDescriptorsFromPatches -- and
(b) the oracle's features_frames -> export_patches(DETMATH) -> surf_describe / sift_compute of the
centred keypoint.  Every comparison is of bytes.

The pair is the pipeline-state tests': synth.make_frame_pair(300, width=160, height=120, seed=5),
pixelsRay 8, pyramids 1, nndrEpsilon 0.55, the pose pair.g12, rodriguesIC as tests/patch_cases.py sets
it.  Neighborhoods.epsilon 0.645 at cmPerPixel 1.0 gives 128 x 128 patches 1.29 m wide: about 57 px
of the 160 x 120 image at the points' depths (1.6 .. 2.4 m, fx 89), so the patches are full of image
and some cross its border.  The oracle chain alone must keep >= 7 points of which at least half have
patches more than half non-zero (the synthetic image has no zero pixel): asserted in `world`.
The second size is 22 (epsilon 0.115): 484 bytes per patch, no multiple of 256."""
import ctypes

import numpy as np
import pytest

import patch_cases as pc

pytestmark = pytest.mark.gpu

EPS, CMPP, SIZE = 0.645, 1.0, 128
EPS_SMALL, SIZE_SMALL = 0.115, 22
INV, UNSUPPORTED = -1, -3

KINDS = {
    "surf_upright_128": dict(extractor="SURF", surfExtended=1, surfUpright=1),
    "surf_upright_64": dict(extractor="SURF", surfExtended=0, surfUpright=1),
    "surf_oriented": dict(extractor="SURF", surfExtended=1, surfUpright=0),
    "sift": dict(extractor="SIFT"),
}


def settings(fm3d, pair, kind="surf_upright_128", eps=EPS, **kw):
    s = fm3d.Settings.default()
    s.set_camera(pair.cam)
    s.pixelsRay, s.pyramids, s.nndrEpsilon = 8, 1, 0.55
    s.rodriguesIC = pc.RODRIGUES_IC
    s.neighEpsilon, s.cmPerPixel = eps, CMPP
    k = dict(KINDS[kind])
    s.extractorType = getattr(fm3d, "FEAT_" + k.pop("extractor"))
    for name, v in {**k, **kw}.items():
        setattr(s, name, v)
    return s


def make_pipe(fm3d, pair, kind="surf_upright_128", eps=EPS, **kw):
    c = fm3d.Context(settings(fm3d, pair, kind, eps, **kw), device=0)
    fm3d.SingleCameraTriangulator(c).set_g12(pair.g12)
    p = fm3d.Pipeline(c)
    p.upload(pair.desc1, pair.desc2, pair.kp1, pair.kp2, pair.img1, pair.img2)
    return p


class Oracle:
    """the oracle chain of one pair, computed once and never changed: the kept points and normals of the
    hot path, their frames, and per (patch size, kind) the patches and descriptor rows"""

    def __init__(self, fm3d, orc, pair):
        self.fm3d, self.orc, self.pair = fm3d, orc, pair
        s = settings(fm3d, pair)
        q, t, _ = orc.match_nndr(pair.desc1, pair.desc2, orc.U8, s.nndrEpsilon)
        pts, mask = orc.triangulate(pair.cam, pair.g12, s.zThresholdMin, s.zThresholdMax, pair.kp1, pair.kp2, q, t)
        self.R2, self.t2 = fm3d.camera2_from_g12(pair.g12)
        ref = orc.optimize_normals(pair.cam, self.R2, self.t2, pair.img1, pair.img2, s.pyramids, pts, s.pixelsRay,
                                   mode=orc.DETMATH)
        ok = ref["status"] == 0
        self.inliers = pts
        self.points, self.normals = pts[ok], ref["normals"][ok]
        self.g = orc.gravity(list(pc.RODRIGUES_IC))
        self.frames = self.frames_of(self.points, self.normals)
        self._patches, self._desc = {}, {}

    def frames_of(self, points, normals):
        return self.orc.features_frames(points, normals, self.g)

    def patches_of(self, frames, eps=EPS):
        return self.orc.export_patches(self.pair.cam, self.pair.img1, frames, eps, CMPP, mode=self.orc.DETMATH)

    def patches(self, eps=EPS):
        if eps not in self._patches:
            self._patches[eps] = self.patches_of(self.frames, eps)
            self._patches[eps].setflags(write=False)
        return self._patches[eps]

    def describe(self, patches, kind):
        size = patches.shape[1]
        kp = np.zeros(1, dtype=self.fm3d.KEYPOINT)
        kp["x"] = kp["y"] = size // 2
        kp["size"], kp["angle"], kp["response"] = size, -1, 1
        k = KINDS[kind]
        rows = []
        for p in patches:
            if k["extractor"] == "SIFT":
                d = self.orc.sift_compute(p, kp)[2]
            else:
                d = self.orc.surf_describe(p, kp, extended=bool(k["surfExtended"]), upright=bool(k["surfUpright"]))[2]
            assert len(d) == 1, "the oracle drops the centred keypoint"
            rows.append(d[0])
        return np.stack(rows) if rows else np.zeros((0, 128), dtype=np.float32)

    def desc(self, kind, eps=EPS):
        if (kind, eps) not in self._desc:
            self._desc[kind, eps] = self.describe(self.patches(eps), kind)
            self._desc[kind, eps].setflags(write=False)
        return self._desc[kind, eps]


@pytest.fixture(scope="module")
def world(fm3d, orc, synth):
    w = Oracle(fm3d, orc, synth.make_frame_pair(300, width=160, height=120, seed=5))
    pa = w.patches()
    assert pa.shape[1:] == (SIZE, SIZE) and w.patches(EPS_SMALL).shape[1:] == (SIZE_SMALL, SIZE_SMALL)
    filled = (pa != 0).reshape(len(pa), -1).mean(axis=1)
    assert len(pa) >= 7 and 2 * int((filled > 0.5).sum()) >= len(pa), (len(pa), filled)
    return w


def chain(fm3d, ctx, points, normals):
    """what the call replaces, through the existing wrappers: (descriptor rows, frames, patches)"""
    frames = fm3d.NormalOptimizer(ctx).computeFeaturesFrames(points, normals)
    patches = fm3d.SingleCameraTriangulator(ctx).projectReferencePointsToImageWithFrames(None, frames)
    return fm3d.Features(ctx).extractDescriptorsFromPatches(patches), frames, patches


def same(got, ref):
    """byte equality of (desc, frames, patches) triples, NaN frames included"""
    for g, r, name in zip(got, ref, ("desc", "frames", "patches")):
        assert g.dtype == r.dtype and g.shape == r.shape, (name, g.dtype, g.shape, r.dtype, r.shape)
        assert g.tobytes() == r.tobytes(), name


class Hip:
    """Device memory of the caller's own, and the device-wide free memory, from the HIP runtime the
    library itself is linked to (the copy already mapped into the process).  Not torch: torch brings its
    own HIP runtime, which finds no GPU in a process where libfm3d initialised its runtime first, as
    every earlier test of a suite run has (tests/buffer_ownership_probe.py).  mem_free() is
    hipMemGetInfo's figure, the one torch.cuda.mem_get_info reports."""
    H2D = 1

    def __init__(self, fm3d):
        fm3d.lib()
        with open("/proc/self/maps") as f:
            path = next(line.split()[-1] for line in f if "libamdhip64" in line)
        self.rt = ctypes.CDLL(path)
        self.owned = []

    def check(self, rc):
        assert rc == 0, f"HIP error {rc}"

    def alloc(self, nbytes):
        p = ctypes.c_void_p()
        self.check(self.rt.hipMalloc(ctypes.byref(p), ctypes.c_size_t(max(nbytes, 64))))
        self.owned.append(p.value)
        return p.value

    def upload(self, arr):
        """a host array in device memory of its own: the device pointer"""
        b = np.ascontiguousarray(arr).tobytes()
        p = self.alloc(len(b))
        if b:
            self.check(self.rt.hipMemcpy(ctypes.c_void_p(p), b, ctypes.c_size_t(len(b)), self.H2D))
        return p

    def mem_free(self):
        free, total = ctypes.c_size_t(), ctypes.c_size_t()
        self.check(self.rt.hipDeviceSynchronize())
        self.check(self.rt.hipMemGetInfo(ctypes.byref(free), ctypes.byref(total)))
        return free.value

    def release(self):
        for p in self.owned:
            self.rt.hipFree(ctypes.c_void_p(p))
        self.owned = []


@pytest.fixture
def hip(fm3d):
    h = Hip(fm3d)
    yield h
    h.release()


@pytest.mark.parametrize("kind", list(KINDS))
def test_equals_the_chain_and_the_oracle(fm3d, world, kind):
    p = make_pipe(fm3d, world.pair, kind)
    try:
        n, _ = p.run()
        rec = p.records(n)
        assert n == len(world.points)
        assert np.array_equal(rec["point"], world.points) and np.array_equal(rec["normal"], world.normals)
        desc, frames, patches, st = p.describe(n, frames=True, patches=True)
        same((desc, frames, patches), chain(fm3d, p.ctx, rec["point"], rec["normal"]))
        same((desc, frames, patches), (world.desc(kind), world.frames, world.patches()))
        assert (st["points"], st["patchSize"], st["cols"], st["type"]) == (n, SIZE, desc.shape[1], fm3d.DESC_F32)
        assert st["chunks"] == 1 and st["total_ms"] > 0
        # without frames / patches nothing else is returned, and the rows are the same
        d2, f2, p2, _ = p.describe(n)
        assert f2 is None and p2 is None and d2.tobytes() == desc.tobytes()
    finally:
        p.ctx.close()


@pytest.mark.parametrize("chunk", [1, 3, None])
def test_chunk_borders(fm3d, world, monkeypatch, chunk):
    """prefixes of the records across chunk borders: the same bytes whatever the chunk, Upright 0 so that
    the kept sum runs over several chunks"""
    kind = "surf_oriented"
    if chunk is None:
        monkeypatch.delenv("FM3D_DESCRIBE_CHUNK", raising=False)
    else:
        monkeypatch.setenv("FM3D_DESCRIBE_CHUNK", str(chunk))
    p = make_pipe(fm3d, world.pair, kind)
    try:
        assert p.run()[0] >= 7
        for n in (7, 0, 1, 2, 3, 4):
            desc, frames, patches, st = p.describe(n, frames=True, patches=True)
            same((desc, frames, patches), (world.desc(kind)[:n], world.frames[:n], world.patches()[:n]))
            assert st["chunks"] == (-(-n // chunk) if chunk else min(n, 1)), (n, st)
            assert st["points"] == n
    finally:
        p.ctx.close()


@pytest.mark.parametrize("kind", ["surf_upright_128", "sift"])
def test_small_patches_across_chunks(fm3d, world, monkeypatch, kind):
    """22 x 22 patches (484 bytes, the last block of each patch half empty), 3 per chunk"""
    monkeypatch.setenv("FM3D_DESCRIBE_CHUNK", "3")
    p = make_pipe(fm3d, world.pair, kind, eps=EPS_SMALL)
    try:
        n = p.run()[0]
        rec = p.records(n)
        got = p.describe(7, frames=True, patches=True)
        assert got[3]["chunks"] == 3 and got[3]["patchSize"] == SIZE_SMALL
        same(got[:3], chain(fm3d, p.ctx, rec["point"][:7], rec["normal"][:7]))
        same(got[:3], (world.desc(kind, EPS_SMALL)[:7], world.frames[:7], world.patches(EPS_SMALL)[:7]))
    finally:
        p.ctx.close()


def test_callers_record_buffer(fm3d, world, hip):
    """records written by run(records_dev_ptr=...) into the caller's device buffer and passed back"""
    p = make_pipe(fm3d, world.pair)
    try:
        buf = hip.upload(np.zeros(p.n_queries, dtype=fm3d.RECORD))
        n, _ = p.run(records_dev_ptr=buf)
        assert n == len(world.points)
        mine = p.describe(n, records_dev_ptr=buf, frames=True, patches=True)
        same(mine[:3], (world.desc("surf_upright_128"), world.frames, world.patches()))
        n2, _ = p.run()  # the internal buffer
        same(p.describe(n2, frames=True, patches=True)[:3], mine[:3])
    finally:
        p.ctx.close()


@pytest.mark.parametrize("kind", ["surf_upright_128", "surf_oriented"])
def test_rare_branches_of_the_frame_arithmetic(fm3d, world, hip, kind):
    """patch_cases' (point, normal) cases -- NaN / inf normals, the normal along and against gravity, both
    sides of normalize3's DBL_EPSILON -- as records on the device: the shared __device__ bodies give the
    one-shot kernels' frames, R, t (through the patches) and rows"""
    cases = pc.frame_cases()
    g = tuple(world.g)
    assert g[0] == 0.0 and g[1] == -1.0  # patch_cases.RODRIGUES_IC: the cross products cancel exactly
    pts, nrm = pc.case_normals(cases, g)
    assert np.isnan(nrm).any() and np.isinf(nrm).any()
    rec = np.zeros(len(pts), dtype=fm3d.RECORD)
    rec["point"], rec["normal"] = pts, nrm
    ctx = fm3d.Context(settings(fm3d, world.pair, kind), device=0)
    try:
        fm3d.NormalOptimizer(ctx).setImages(world.pair.img1, world.pair.img2)
        got = fm3d.Pipeline(ctx).describe(len(rec), records_dev_ptr=hip.upload(rec), frames=True, patches=True)
        ref = chain(fm3d, ctx, pts, nrm)
        assert np.isnan(ref[1]).any()
        assert np.array_equal(got[1], ref[1], equal_nan=True)
        same(got[:3], ref)
        # and the oracle's frames and patches (DETMATH), the rank-deficient and non-finite cases included
        of = world.frames_of(pts, nrm)
        assert np.array_equal(got[1], of, equal_nan=True)
        assert np.array_equal(got[2], world.patches_of(of))
    finally:
        ctx.close()


def test_ncc_source(fm3d, orc, world):
    """the points of dlt_download and the best normals of ncc_download, read where they lie.  This pair
    has points whose best is -1 at 4 x 4 hypotheses (48 of its 208 inliers by the oracle; asserted): no
    hypothesis scores, their normal is the initial guess, and they are described like the others."""
    p = make_pipe(fm3d, world.pair, "surf_oriented")
    try:
        with pytest.raises(fm3d.Fm3dError) as e:
            p.describe(3, source="ncc")  # no NCC run yet
        assert e.value.code == INV
        n, st = p.run_ncc(4, 4)
        assert n == len(world.inliers) > 7
        _, pts, _ = p.dlt_results(st["matches"], n)
        _, nrm, best = p.ncc_results(n, 16)
        assert np.array_equal(pts, world.inliers)
        assert 0 < int((best < 0).sum()) < n
        got = p.describe(n, source="ncc", frames=True, patches=True)
        same(got[:3], chain(fm3d, p.ctx, pts, nrm))
        of = world.frames_of(pts, nrm)
        same(got[1:3], (of, world.patches_of(of)))
        assert got[0].tobytes() == world.describe(got[2], "surf_oriented").tobytes()
        for bad in (n - 1, n + 1):
            with pytest.raises(fm3d.Fm3dError):
                p.describe(bad, source="ncc")
        # a later full run leaves the NCC rows where they are; the records source reads the records
        k, _ = p.run()
        same(p.describe(k, frames=True, patches=True)[:3],
             (world.desc("surf_oriented"), world.frames, world.patches()))
    finally:
        p.ctx.close()


def code_of(fm3d, fn):
    with pytest.raises(fm3d.Fm3dError) as e:
        fn()
    return e.value.code


def test_refusals(fm3d, world, hip):
    L = fm3d.lib()
    pair = world.pair
    full = (pair.desc1, pair.desc2, pair.kp1, pair.kp2, pair.img1, pair.img2)
    ref = (world.desc("surf_upright_128")[:5], world.frames[:5], world.patches()[:5])
    p = make_pipe(fm3d, pair)
    try:
        n = p.run()[0]
        h = p.ctx.handle
        out = np.zeros((n, 128), dtype=np.float32)
        vp = lambda a: ctypes.c_void_p(a.ctypes.data)
        raw = lambda ctx, src, rec, m, d: L.fm3d_pipeline_describe(ctx, src, ctypes.c_void_p(rec), m, d, None, None, None)
        good = lambda: same(p.describe(5, frames=True, patches=True)[:3], ref)
        assert raw(None, 0, 0, n, vp(out)) == INV                 # a null context
        assert raw(h, 0, 0, -1, vp(out)) == INV                   # n < 0
        assert raw(h, 2, 0, n, vp(out)) == INV                    # a source outside {0, 1}
        assert raw(h, -1, 0, n, vp(out)) == INV
        assert raw(h, 0, 0, n, None) == INV                       # a null desc with n > 0
        assert raw(h, 1, 0, n, vp(out)) == INV                    # NCC before any NCC run
        good()
        k = p.run_ncc(4, 4)[0]
        dummy = hip.upload(np.zeros(k, dtype=fm3d.RECORD))
        assert raw(h, 1, dummy, k, vp(out)) == INV                # NCC with a record buffer
        assert raw(h, 1, 0, k - 1, vp(out)) == INV                # NCC with another count
        assert p.run()[0] == n
        good()
        # a pending submit of every kind; its own wait then gives what it would have given
        p.submit(*full)
        assert code_of(fm3d, lambda: p.describe(5)) == INV
        rec, _ = p.wait()
        assert np.array_equal(rec["point"], world.points)
        good()
        p.submit_dlt()
        assert code_of(fm3d, lambda: p.describe(5)) == INV
        assert p.wait_dlt()[0] == len(world.inliers)
        p.submit_verified(*full, max_px=2.0, hypotheses=64)
        assert code_of(fm3d, lambda: p.describe(5)) == INV
        p.wait_verified()
        assert p.run()[0] == n
        good()
        # n == 0: nothing done, stats zeroed
        d0, _, _, st0 = p.describe(0)
        assert d0.shape[0] == 0 and not any(st0.values())
    finally:
        p.ctx.close()
    # no image 1 on the context (records in a caller's buffer, so that only the image is missing)
    c = fm3d.Context(settings(fm3d, pair), device=0)
    try:
        dev = hip.upload(np.zeros(4, dtype=fm3d.RECORD))
        assert code_of(fm3d, lambda: fm3d.Pipeline(c).describe(4, records_dev_ptr=dev)) == INV
        assert code_of(fm3d, lambda: fm3d.Pipeline(c).describe(4)) == INV  # nor any record
    finally:
        c.close()
    # a patch size <= 0
    q = make_pipe(fm3d, pair, eps=0.001)  # 2 * floor(0.1) = 0
    try:
        k = q.run()[0]
        assert k > 0 and code_of(fm3d, lambda: q.describe(k)) == INV
    finally:
        q.ctx.close()
    # the binary extractors: later work, their one-shot path stays
    for ex in ("FEAT_ORB", "FEAT_BRISK", "FEAT_FREAK"):
        q = make_pipe(fm3d, pair, extractorType=getattr(fm3d, ex))
        try:
            k = q.run()[0]
            assert code_of(fm3d, lambda: q.describe(k)) == UNSUPPORTED, ex
        finally:
            q.ctx.close()


def test_reuse(fm3d, orc, synth, world, hip):
    """a repeated call allocates nothing; the one-shot SURF calls that share the sf* buffers still give
    the oracle's rows afterwards; a second, different pair on the same context is right"""
    kind = "surf_oriented"
    p = make_pipe(fm3d, world.pair, kind)
    try:
        n = p.run()[0]
        ref = (world.desc(kind), world.frames, world.patches())
        same(p.describe(n, frames=True, patches=True)[:3], ref)
        same(p.describe(n, frames=True, patches=True)[:3], ref)
        free2 = hip.mem_free()
        same(p.describe(n, frames=True, patches=True)[:3], ref)
        free3 = hip.mem_free()
        same(p.describe(n - 3, frames=True, patches=True)[:3], tuple(r[:n - 3] for r in ref))
        assert free2 == free3 == hip.mem_free()
        # the one-shot calls on the same context
        kin = np.zeros(20, dtype=fm3d.KEYPOINT)
        kin["x"], kin["y"] = world.pair.kp1[:20, 0], world.pair.kp1[:20, 1]
        kin["size"], kin["angle"], kin["response"] = 14, -1, 1
        k, kept, d = fm3d.SURF(p.ctx).compute(world.pair.img1, kin)
        ko, kepto, do = orc.surf_describe(world.pair.img1, kin, extended=True, upright=False)
        assert len(ko) > 0 and np.array_equal(kept, kepto) and np.array_equal(d, do)
        one = fm3d.SURF(p.ctx).extractDescriptorsFromPatches(world.patches()[:9])
        assert one.tobytes() == world.desc(kind)[:9].tobytes()
        same(p.describe(n, frames=True, patches=True)[:3], ref)
        # another pair, same context
        other = Oracle(fm3d, orc, synth.make_frame_pair(300, width=160, height=120, seed=6))
        assert len(other.points) >= 7 and len(other.points) != n
        fm3d.SingleCameraTriangulator(p.ctx).set_g12(other.pair.g12)
        o = other.pair
        p.upload(o.desc1, o.desc2, o.kp1, o.kp2, o.img1, o.img2)
        m = p.run()[0]
        assert m == len(other.points)
        same(p.describe(m, frames=True, patches=True)[:3], (other.desc(kind), other.frames, other.patches()))
    finally:
        p.ctx.close()
