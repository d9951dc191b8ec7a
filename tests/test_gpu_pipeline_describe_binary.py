"""fm3d_pipeline_describe_any (csrc/fm3d_tail.cpp) with the binary extractors, and the batched ORB behind
fm3d_extract_descriptors_from_patches_any: against the oracle's orb_compute on each oracle patch with its
centred keypoint (centre, size, angle -1, response 1), and against a loop of the single-image
fm3d.ORB(ctx).compute over the same patches.  Every comparison is of bytes.

The pair and the settings are tests/test_gpu_pipeline_describe.py's.  Patch edges by Neighborhoods.epsilon
at cmPerPixel 1.0: 0.645 -> 128, 0.325 -> 64 (the smallest ORB keeps at edgeThreshold 31), 0.315 -> 62
(dropped), 0.275 -> 54 (the smallest at edgeThreshold 26), 0.265 -> 52 (dropped), 3.175 -> 634 (BRISK's
first kept edge; FREAK's is 680).  The module fixture asserts from the oracle alone that the ORB rows
at 128 are many, pairwise distinct and about half ones, so that constant rows cannot pass."""
import ctypes

import numpy as np
import pytest

import patch_cases as pc
from test_gpu_pipeline_describe import EPS, Hip, Oracle, chain, code_of, make_pipe, same, settings

pytestmark = pytest.mark.gpu

INV, UNSUPPORTED = -1, -3
SIZES = {0.645: (128, 31), 0.325: (64, 31), 0.275: (54, 26)}   # epsilon: (edge, orbEdgeThreshold), kept
DROPS = {0.315: (62, 31), 0.265: (52, 26)}
EPS_634 = 3.175


def centred(fm3d, size):
    kp = np.zeros(1, dtype=fm3d.KEYPOINT)
    kp["x"] = kp["y"] = size // 2
    kp["size"], kp["angle"], kp["response"] = size, -1, 1
    return kp


def orb_rows(w, patches, edge=31, patch_size=31, pattern=None):
    """the oracle's ORB row of each patch"""
    kp = centred(w.fm3d, patches.shape[1])
    rows = []
    for p in patches:
        d = w.orc.orb_compute(p, kp, edgeThreshold=edge, patchSize=patch_size, pattern=pattern)[2]
        assert len(d) == 1, "the oracle drops the centred keypoint"
        rows.append(d[0])
    return np.stack(rows) if rows else np.zeros((0, 32), dtype=np.uint8)


def orb_loop(fm3d, ctx, patches):
    """the unchanged single-image call, patch by patch"""
    kp = centred(fm3d, patches.shape[1])
    rows = []
    for p in patches:
        d = fm3d.ORB(ctx).compute(p, kp)[2]
        assert len(d) == 1
        rows.append(d[0])
    return np.stack(rows) if rows else np.zeros((0, 32), dtype=np.uint8)


def orb_pipe(fm3d, pair, eps=EPS, edge=31, **kw):
    return make_pipe(fm3d, pair, eps=eps, extractorType=fm3d.FEAT_ORB, orbEdgeThreshold=edge, **kw)


@pytest.fixture(scope="module")
def world(fm3d, orc, synth):
    w = Oracle(fm3d, orc, synth.make_frame_pair(300, width=160, height=120, seed=5))
    w.orb = {eps: orb_rows(w, w.patches(eps), edge) for eps, (_, edge) in SIZES.items()}
    for eps, (size, _) in {**SIZES, **DROPS}.items():
        assert w.patches(eps).shape[1:] == (size, size)
    rows = w.orb[EPS]
    assert len(rows) >= 100
    assert len({r.tobytes() for r in rows}) == len(rows), "two patches with the same ORB row"
    density = np.unpackbits(rows).mean()
    assert 0.4 <= density <= 0.6, density
    for r in w.orb.values():
        r.setflags(write=False)
    return w


@pytest.fixture
def hip(fm3d):
    h = Hip(fm3d)
    yield h
    h.release()


@pytest.mark.parametrize("eps", list(SIZES))
def test_sizes(fm3d, world, eps):
    size, edge = SIZES[eps]
    p = orb_pipe(fm3d, world.pair, eps, edge)
    try:
        n = p.run()[0]
        assert n == len(world.points)
        assert fm3d.Features(p.ctx).patch_keypoint_kept(size)
        desc, frames, patches, st = p.describe_any(n, frames=True, patches=True)
        same((desc, frames, patches), (world.orb[eps], world.frames, world.patches(eps)))
        assert desc.tobytes() == orb_loop(fm3d, p.ctx, patches).tobytes()
        assert (st["points"], st["patchSize"], st["cols"], st["type"]) == (n, size, 32, fm3d.DESC_BITS)
        assert st["chunks"] == 1 and st["total_ms"] > 0
        d2, f2, p2, _ = p.describe_any(n)
        assert f2 is None and p2 is None and d2.tobytes() == desc.tobytes()
    finally:
        p.ctx.close()


@pytest.mark.parametrize("eps", list(DROPS))
def test_drops(fm3d, world, eps):
    """an edge at which ORB's border filter drops the centred keypoint; the next call at a kept size, on a
    context of its own settings, is right"""
    size, edge = DROPS[eps]
    keep = {31: 0.325, 26: 0.275}[edge]
    p = orb_pipe(fm3d, world.pair, eps, edge)
    try:
        n = p.run()[0]
        assert not fm3d.Features(p.ctx).patch_keypoint_kept(size)
        with pytest.raises(fm3d.Fm3dError) as e:
            p.describe_any(n, frames=True, patches=True)
        assert e.value.code == INV and "ORB drops the first patch's keypoint" in str(e.value)
        with pytest.raises(fm3d.Fm3dError) as e:
            fm3d.Features(p.ctx).extractDescriptorsFromPatches(world.patches(eps)[:3])
        assert e.value.code == INV and "ORB drops the first patch's keypoint" in str(e.value)
        # the same context, patches of the next edge up
        one = fm3d.Features(p.ctx).extractDescriptorsFromPatches(world.patches(keep)[:5])
        assert one.tobytes() == world.orb[keep][:5].tobytes()
    finally:
        p.ctx.close()
    q = orb_pipe(fm3d, world.pair, keep, edge)
    try:
        n = q.run()[0]
        same(q.describe_any(n, frames=True, patches=True)[:3], (world.orb[keep], world.frames, world.patches(keep)))
    finally:
        q.ctx.close()


def test_patterns(fm3d, world):
    """orbPatchSize 15 and a user pattern set and cleared between calls on one context: a stale offset
    table would give another pattern's rows"""
    n = 8
    pa = world.patches()[:n]
    user = np.random.default_rng(3).integers(-15, 16, 1024).astype(np.int32)
    ref31, ref15, refu = world.orb[EPS][:n], orb_rows(world, pa, patch_size=15), orb_rows(world, pa, pattern=user)
    for a, b in ((ref31, ref15), (ref31, refu), (ref15, refu)):
        assert all(x.tobytes() != y.tobytes() for x, y in zip(a, b))
    p = orb_pipe(fm3d, world.pair)
    try:
        assert p.run()[0] >= n
        assert p.describe_any(n)[0].tobytes() == ref31.tobytes()
        fm3d.ORB(p.ctx).set_pattern(user)
        assert p.describe_any(n)[0].tobytes() == refu.tobytes()
        assert fm3d.Features(p.ctx).extractDescriptorsFromPatches(pa).tobytes() == refu.tobytes()
        fm3d.ORB(p.ctx).set_pattern(None)
        assert p.describe_any(n)[0].tobytes() == ref31.tobytes()
    finally:
        p.ctx.close()
    q = orb_pipe(fm3d, world.pair, orbPatchSize=15)
    try:
        assert q.run()[0] >= n
        got = q.describe_any(n, patches=True)
        assert got[2].tobytes() == pa.tobytes() and got[0].tobytes() == ref15.tobytes()
    finally:
        q.ctx.close()


@pytest.mark.parametrize("chunk", [1, 3, None])
def test_chunk_borders(fm3d, world, monkeypatch, chunk):
    if chunk is None:
        monkeypatch.delenv("FM3D_DESCRIBE_CHUNK", raising=False)
    else:
        monkeypatch.setenv("FM3D_DESCRIBE_CHUNK", str(chunk))
    p = orb_pipe(fm3d, world.pair)
    try:
        assert p.run()[0] >= 7
        for n in (7, 0, 1, 2, 3, 4):
            desc, frames, patches, st = p.describe_any(n, frames=True, patches=True)
            same((desc, frames, patches), (world.orb[EPS][:n], world.frames[:n], world.patches()[:n]))
            assert st["chunks"] == (-(-n // chunk) if chunk else min(n, 1)), (n, st)
            if n:
                assert (st["points"], st["patchSize"], st["cols"], st["type"]) == (n, 128, 32, fm3d.DESC_BITS)
            else:
                assert not any(st.values())
    finally:
        p.ctx.close()


def test_callers_record_buffer(fm3d, world, hip):
    p = orb_pipe(fm3d, world.pair)
    try:
        buf = hip.upload(np.zeros(p.n_queries, dtype=fm3d.RECORD))
        n, _ = p.run(records_dev_ptr=buf)
        assert n == len(world.points)
        mine = p.describe_any(n, records_dev_ptr=buf, frames=True, patches=True)
        same(mine[:3], (world.orb[EPS], world.frames, world.patches()))
    finally:
        p.ctx.close()


def test_ncc_source(fm3d, world):
    p = orb_pipe(fm3d, world.pair)
    try:
        n, st = p.run_ncc(4, 4)
        assert n == len(world.inliers) > 7
        _, pts, _ = p.dlt_results(st["matches"], n)
        _, nrm, _ = p.ncc_results(n, 16)
        got = p.describe_any(n, source="ncc", frames=True, patches=True)
        of = world.frames_of(pts, nrm)
        op = world.patches_of(of)
        same(got[:3], (orb_rows(world, op), of, op))
    finally:
        p.ctx.close()


def test_nan_and_inf_normals(fm3d, world, hip):
    """patch_cases' frame cases as records: whatever patch a NaN or inf frame gives, its row is the
    single-image call's on that patch"""
    pts, nrm = pc.case_normals(pc.frame_cases(), tuple(world.g))
    assert np.isnan(nrm).any() and np.isinf(nrm).any()
    rec = np.zeros(len(pts), dtype=fm3d.RECORD)
    rec["point"], rec["normal"] = pts, nrm
    s = settings(fm3d, world.pair, extractorType=fm3d.FEAT_ORB)
    ctx = fm3d.Context(s, device=0)
    try:
        fm3d.NormalOptimizer(ctx).setImages(world.pair.img1, world.pair.img2)
        got = fm3d.Pipeline(ctx).describe_any(len(rec), records_dev_ptr=hip.upload(rec), frames=True, patches=True)
        of = world.frames_of(pts, nrm)
        assert np.array_equal(got[1], of, equal_nan=True)
        assert np.array_equal(got[2], world.patches_of(of))
        assert got[0].tobytes() == orb_loop(fm3d, ctx, got[2]).tobytes()
    finally:
        ctx.close()


def test_one_shot(fm3d, world, hip, monkeypatch):
    """extractDescriptorsFromPatches with ORB: one launch per chunk instead of a compute per patch"""
    monkeypatch.delenv("FM3D_DESCRIBE_CHUNK", raising=False)
    for eps in (0.645, 0.275):
        size, edge = SIZES[eps]
        ctx = fm3d.Context(settings(fm3d, world.pair, eps=eps, extractorType=fm3d.FEAT_ORB, orbEdgeThreshold=edge),
                           device=0)
        try:
            f = fm3d.Features(ctx)
            assert f.extractDescriptorsFromPatches(world.patches(eps)[:9]).tobytes() == world.orb[eps][:9].tobytes()
            none = f.extractDescriptorsFromPatches(np.zeros((0, size, size), dtype=np.uint8))
            assert none.shape == (0, 32) and none.dtype == np.uint8
            monkeypatch.setenv("FM3D_DESCRIBE_CHUNK", "4")  # 4 + 4 + 1
            assert f.extractDescriptorsFromPatches(world.patches(eps)[:9]).tobytes() == world.orb[eps][:9].tobytes()
            monkeypatch.delenv("FM3D_DESCRIBE_CHUNK")
        finally:
            ctx.close()
    # a repeated describe_any allocates nothing, nor does the one-shot call on fewer patches in between
    p = orb_pipe(fm3d, world.pair)
    try:
        n = p.run()[0]
        ref = (world.orb[EPS], world.frames, world.patches())
        same(p.describe_any(n, frames=True, patches=True)[:3], ref)
        free1 = hip.mem_free()
        same(p.describe_any(n, frames=True, patches=True)[:3], ref)
        free2 = hip.mem_free()
        one = fm3d.Features(p.ctx).extractDescriptorsFromPatches(world.patches()[:9])
        assert one.tobytes() == world.orb[EPS][:9].tobytes()
        same(p.describe_any(n, frames=True, patches=True)[:3], ref)
        assert free1 == free2 == hip.mem_free()
    finally:
        p.ctx.close()


@pytest.mark.parametrize("ex", ["FEAT_BRISK", "FEAT_FREAK"])
def test_brisk_and_freak(fm3d, world, ex):
    """below 634 / 680 px both drop the centred keypoint: the reference's Mat::zeros rows"""
    p = make_pipe(fm3d, world.pair, extractorType=getattr(fm3d, ex))
    try:
        n = p.run()[0]
        assert n == len(world.points)
        assert not fm3d.Features(p.ctx).patch_keypoint_kept(128)
        desc, frames, patches, st = p.describe_any(n, frames=True, patches=True)
        zeros = np.zeros((n, 64), dtype=np.uint8)
        same((desc, frames, patches), (zeros, world.frames, world.patches()))
        assert (st["points"], st["patchSize"], st["cols"], st["type"]) == (n, 128, 64, fm3d.DESC_BITS)
        d2, f2, p2, st2 = p.describe_any(n)
        assert f2 is None and p2 is None and d2.dtype == np.uint8 and d2.tobytes() == zeros.tobytes()
        assert st2["chunks"] == 0
        one = fm3d.Features(p.ctx).extractDescriptorsFromPatches(patches[:5])
        assert one.dtype == np.uint8 and one.tobytes() == zeros[:5].tobytes()
    finally:
        p.ctx.close()
    q = make_pipe(fm3d, world.pair, eps=EPS_634, extractorType=getattr(fm3d, ex))
    try:
        k = q.run()[0]
        assert k >= 3
        assert fm3d.lib().fm3d_patch_size(ctypes.byref(q.ctx.settings)) == 634
        if ex == "FEAT_BRISK":  # kept from 634: no batched form
            assert fm3d.Features(q.ctx).patch_keypoint_kept(634)
            with pytest.raises(fm3d.Fm3dError) as e:
                q.describe_any(3)
            assert e.value.code == UNSUPPORTED and "634" in str(e.value)
        else:                   # FREAK's pattern still reaches past a 634 px patch
            d, _, _, st = q.describe_any(3)
            assert d.tobytes() == bytes(3 * 64) and (st["cols"], st["type"]) == (64, fm3d.DESC_BITS)
    finally:
        q.ctx.close()


@pytest.mark.parametrize("kind", ["surf_oriented", "sift"])
def test_surf_and_sift_through_the_new_call(fm3d, world, kind):
    p = make_pipe(fm3d, world.pair, kind)
    try:
        assert p.run()[0] >= 7
        a, b = p.describe_any(7, frames=True, patches=True), p.describe(7, frames=True, patches=True)
        same(a[:3], b[:3])
        assert a[0].dtype == np.float32 and a[0].any()
        assert {k: v for k, v in a[3].items() if k != "total_ms"} == {k: v for k, v in b[3].items() if k != "total_ms"}
    finally:
        p.ctx.close()


def test_refusals(fm3d, world, hip):
    L = fm3d.lib()
    pair = world.pair
    full = (pair.desc1, pair.desc2, pair.kp1, pair.kp2, pair.img1, pair.img2)
    ref = (world.orb[EPS][:5], world.frames[:5], world.patches()[:5])
    p = orb_pipe(fm3d, pair)
    try:
        n = p.run()[0]
        h = p.ctx.handle
        out = np.zeros((n, 32), dtype=np.uint8)
        vp = lambda a: ctypes.c_void_p(a.ctypes.data)
        raw = lambda ctx, src, rec, m, d: L.fm3d_pipeline_describe_any(ctx, src, ctypes.c_void_p(rec), m, d, None, None,
                                                                       None)
        good = lambda: same(p.describe_any(5, frames=True, patches=True)[:3], ref)
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
        p.submit(*full)                                           # a pending submit
        assert code_of(fm3d, lambda: p.describe_any(5)) == INV
        p.wait()
        good()
        # the older call keeps its refusal of the binary extractors
        assert code_of(fm3d, lambda: p.describe(5)) == UNSUPPORTED
        good()
    finally:
        p.ctx.close()
    c = fm3d.Context(settings(fm3d, pair, extractorType=fm3d.FEAT_ORB), device=0)  # no image 1
    try:
        dev = hip.upload(np.zeros(4, dtype=fm3d.RECORD))
        assert code_of(fm3d, lambda: fm3d.Pipeline(c).describe_any(4, records_dev_ptr=dev)) == INV
    finally:
        c.close()
    # settings that fm3d_orb_compute refuses are refused with its code
    q = orb_pipe(fm3d, pair, edge=20)  # < ceil(15 * 1.4143) + 4
    try:
        k = q.run()[0]
        assert k > 0
        with pytest.raises(fm3d.Fm3dError) as e:
            q.describe_any(k)
        assert e.value.code == INV and "edgeThreshold too small" in str(e.value)
    finally:
        q.ctx.close()
