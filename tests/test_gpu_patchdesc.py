"""The patch describer (csrc/fm3d_patchdesc.cpp) behind both fm3d_extract_descriptors_from_patches(_any)
and fm3d_pipeline_describe(_any): the cached per-patch tables that the two share on one context, with
the one-shot calls repeated and the two taking turns.  Every comparison is of bytes, against the oracle's rows
of the oracle's own patches (tests/test_gpu_pipeline_describe.py's chain: features_frames ->
export_patches(DETMATH) -> surf_describe / sift_compute / orb_compute of the centred keypoint), never
against the other entry point.

The pair and the settings are tests/test_gpu_pipeline_describe.py's.  Patch edges by
Neighborhoods.epsilon at cmPerPixel 1.0: 0.645 -> 128 (the tail's here), 0.115 -> 22 and 0.135 -> 26 for
SURF and SIFT, 0.275 -> 54 and 0.325 -> 64 for ORB at edgeThreshold 26 (54 is the smallest edge it keeps).
The oracle describes the first 7 points only."""
import numpy as np
import pytest

from test_gpu_pipeline_describe import EPS, EPS_SMALL, SIZE, SIZE_SMALL, Oracle, make_pipe, settings
from test_gpu_pipeline_describe_binary import orb_rows

pytestmark = pytest.mark.gpu

N = 7
EPS_26, EPS_54, EPS_64, ORB_EDGE = 0.135, 0.275, 0.325, 26
FLOAT_KINDS = ["surf_upright_128", "surf_oriented", "sift"]


@pytest.fixture(scope="module")
def world(fm3d, orc, synth):
    """the oracle's first N patches per edge and their rows per kind, computed once and read-only"""
    w = Oracle(fm3d, orc, synth.make_frame_pair(300, width=160, height=120, seed=5))
    assert len(w.points) >= N
    w.pa = {eps: w.patches_of(w.frames[:N], eps) for eps in (EPS, EPS_SMALL, EPS_26, EPS_54, EPS_64)}
    for eps, size in ((EPS, SIZE), (EPS_SMALL, SIZE_SMALL), (EPS_26, 26), (EPS_54, 54), (EPS_64, 64)):
        assert w.pa[eps].shape == (N, size, size)
    w.rows = {(k, eps): w.describe(w.pa[eps], k) for k in FLOAT_KINDS for eps in (EPS, EPS_SMALL, EPS_26)}
    w.user = np.random.default_rng(3).integers(-15, 16, 1024).astype(np.int32)
    for eps in (EPS, EPS_54, EPS_64):
        w.rows["orb", eps] = orb_rows(w, w.pa[eps], edge=ORB_EDGE)
    w.rows["orb_user", EPS_54] = orb_rows(w, w.pa[EPS_54], edge=ORB_EDGE, pattern=w.user)
    for a in list(w.pa.values()) + list(w.rows.values()):
        a.setflags(write=False)
    # rows that tell the kinds, the edges and the patterns apart, so that a stale table cannot pass
    for eps in (EPS, EPS_SMALL, EPS_26):
        assert w.rows["surf_upright_128", eps].tobytes() != w.rows["surf_oriented", eps].tobytes()
    assert w.rows["orb", EPS_54].tobytes() != w.rows["orb_user", EPS_54].tobytes()
    for r in w.rows.values():
        assert len({x.tobytes() for x in r}) == N and r.any()
    return w


def set_chunk(monkeypatch, chunk):
    if chunk is None:
        monkeypatch.delenv("FM3D_DESCRIBE_CHUNK", raising=False)
    else:
        monkeypatch.setenv("FM3D_DESCRIBE_CHUNK", str(chunk))


@pytest.mark.parametrize("kind", FLOAT_KINDS)
def test_one_shot_repeated(fm3d, world, monkeypatch, kind):
    """7 patches of 22 x 22 through the one-shot call, which takes SURF and SIFT patches all at once
    whatever FM3D_DESCRIBE_CHUNK says: the second call finds every table cached, the third reads a
    prefix of them"""
    set_chunk(monkeypatch, 3)
    ctx = fm3d.Context(settings(fm3d, world.pair, kind, eps=EPS_SMALL), device=0)
    try:
        f = fm3d.Features(ctx)
        for n in (N, N, 3):
            got = f.extractDescriptorsFromPatches(world.pa[EPS_SMALL][:n])
            assert got.dtype == np.float32 and got.tobytes() == world.rows[kind, EPS_SMALL][:n].tobytes()
    finally:
        ctx.close()


def one_shot(fm3d, p, world, key, eps, n):
    got = fm3d.Features(p.ctx).extractDescriptorsFromPatches(world.pa[eps][:n])
    assert got.tobytes() == world.rows[key, eps][:n].tobytes(), (key, eps, n)


def tail(p, world, key, any_form=False):
    """the tail at the pipeline's 128 px edge, 7 points in chunks of 3"""
    desc, _, patches, st = (p.describe_any if any_form else p.describe)(N, patches=True)
    assert st["chunks"] == 3 and st["patchSize"] == SIZE
    assert patches.tobytes() == world.pa[EPS].tobytes()
    assert desc.tobytes() == world.rows[key, EPS].tobytes(), key


def test_shared_tables_sift(fm3d, world, monkeypatch):
    """the tables are keyed by (capacity, edge, angle) and by sigma: the one-shot call and the tail
    take turns on one context, at three edges and falling capacities"""
    set_chunk(monkeypatch, 3)
    p = make_pipe(fm3d, world.pair, "sift")
    try:
        assert p.run()[0] >= N
        one_shot(fm3d, p, world, "sift", EPS_SMALL, 5)
        tail(p, world, "sift")
        one_shot(fm3d, p, world, "sift", EPS_SMALL, 2)  # a smaller capacity reads a prefix
        one_shot(fm3d, p, world, "sift", EPS_26, N)
    finally:
        p.ctx.close()


def set_upright(fm3d, ctx, upright):
    """No call of the ABI changes a context's settings.  The context keeps its copy as its first member
    (csrc/fm3d_ctx.h), so the test writes the one field there -- after checking that this is the copy."""
    live = fm3d.Settings.from_address(ctx.handle.value)
    assert bytes(live) == bytes(ctx.settings)
    live.surfUpright = ctx.settings.surfUpright = upright


def test_shared_tables_surf(fm3d, world, monkeypatch):
    """as for SIFT on a context of its own, and Upright 1 -> 0 between the steps: the keypoint table's
    angle key goes from 270 to -1 at an unchanged capacity and edge"""
    set_chunk(monkeypatch, 3)
    up, ori = "surf_upright_128", "surf_oriented"
    p = make_pipe(fm3d, world.pair, up)
    try:
        assert p.run()[0] >= N
        one_shot(fm3d, p, world, up, EPS_SMALL, 5)
        tail(p, world, up)
        set_upright(fm3d, p.ctx, 0)
        tail(p, world, ori)  # capacity 3, edge 128 as the call before: only the angle differs
        one_shot(fm3d, p, world, ori, EPS_SMALL, 2)
        one_shot(fm3d, p, world, ori, EPS_26, N)
        set_upright(fm3d, p.ctx, 1)
        one_shot(fm3d, p, world, up, EPS_26, N)
    finally:
        p.ctx.close()


def test_shared_tables_orb(fm3d, world, monkeypatch):
    """ORB's table is the rotated pattern's offsets; fm3d_orb_set_pattern still invalidates it for both
    callers"""
    set_chunk(monkeypatch, 3)
    p = make_pipe(fm3d, world.pair, extractorType=fm3d.FEAT_ORB, orbEdgeThreshold=ORB_EDGE)
    try:
        assert p.run()[0] >= N
        one_shot(fm3d, p, world, "orb", EPS_54, 5)
        tail(p, world, "orb", any_form=True)
        one_shot(fm3d, p, world, "orb", EPS_54, 2)
        one_shot(fm3d, p, world, "orb", EPS_64, N)
        fm3d.ORB(p.ctx).set_pattern(world.user)
        one_shot(fm3d, p, world, "orb_user", EPS_54, N)
        fm3d.ORB(p.ctx).set_pattern(None)
        tail(p, world, "orb", any_form=True)
    finally:
        p.ctx.close()
