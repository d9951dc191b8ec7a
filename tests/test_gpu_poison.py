"""FM3D_DEBUG_POISON (csrc/fm3d_ctx.h): every block Buf::ensure newly allocates is filled with the
variable's 32-bit word, so a kernel that reads memory nothing wrote gives another result -- the same
one every run -- instead of passing on a fresh hipMalloc block that happened to be zero.

The hook itself first (fm3d_internal_alloc_probe); then every public entry point of reuse_cases.py's
table at its small shape on a fresh context under each of two words: byte-equal to the same call
on an unpoisoned fresh context, and equal to the oracle or restatement where the entry point's own
test compares with one.  Under 1 stale flags read as set, counts as 1, indices stay valid and floats
are denormals; under 0xffffffff ints read as -1 and floats and doubles as NaN."""
import ctypes

import numpy as np
import pytest

import reuse_cases as rc

pytestmark = pytest.mark.gpu

WORDS = ["1", "0xffffffff"]


def _probe(fm3d, nbytes):
    L = fm3d.lib()
    L.fm3d_internal_alloc_probe.argtypes = [ctypes.c_void_p, ctypes.c_size_t, ctypes.c_void_p]
    L.fm3d_internal_alloc_probe.restype = ctypes.c_int
    ctx = fm3d.Context(fm3d.Settings.default())
    try:
        out = np.full(nbytes, 0x5a, dtype=np.uint8)
        ctx.check(L.fm3d_internal_alloc_probe(ctx.handle, nbytes, out.ctypes.data))
    finally:
        ctx.close()
    return out


@pytest.mark.parametrize("word", WORDS)
@pytest.mark.parametrize("nbytes", [256, 4096, 4099])
def test_fresh_blocks_hold_the_poison_word(fm3d, monkeypatch, nbytes, word):
    """every whole word and every tail byte of a fresh device block is the poison; unset, the block
    is whatever hipMalloc gave (nothing asserted about it, only that the call works)"""
    monkeypatch.setenv("FM3D_DEBUG_POISON", word)
    got = _probe(fm3d, nbytes)
    w = np.uint32(int(word, 0))
    assert np.array_equal(got[:nbytes // 4 * 4].view(np.uint32), np.full(nbytes // 4, w, dtype=np.uint32))
    tail = np.frombuffer(w.tobytes(), dtype=np.uint8)[:nbytes % 4]
    assert np.array_equal(got[nbytes // 4 * 4:], tail)
    monkeypatch.delenv("FM3D_DEBUG_POISON")
    assert _probe(fm3d, nbytes).shape == (nbytes,)


def test_probe_refuses_undefined_inputs(fm3d):
    L = fm3d.lib()
    L.fm3d_internal_alloc_probe.argtypes = [ctypes.c_void_p, ctypes.c_size_t, ctypes.c_void_p]
    L.fm3d_internal_alloc_probe.restype = ctypes.c_int
    ctx = fm3d.Context(fm3d.Settings.default())
    try:
        out = np.zeros(16, dtype=np.uint8)
        assert L.fm3d_internal_alloc_probe(ctx.handle, 0, out.ctypes.data) == fm3d.ERR_INVALID
        assert L.fm3d_internal_alloc_probe(ctx.handle, 16, None) == fm3d.ERR_INVALID
    finally:
        ctx.close()


@pytest.mark.parametrize("word", WORDS)
@pytest.mark.parametrize("case", rc.CASES, ids=[c.name for c in rc.CASES])
def test_entry_point_ignores_what_fresh_blocks_hold(fm3d, orc, synth, monkeypatch, case, word):
    """the entry point at its small shape on a poisoned fresh context: byte-equal to an unpoisoned
    fresh context's result and equal to the oracle"""
    world = rc.world(fm3d, orc, synth)
    for x in case.small_keys:
        clean = world.once(("unpoisoned", case.name, x), lambda: rc.run_fresh(fm3d, case, world, x))  # shared by the words
        monkeypatch.setenv("FM3D_DEBUG_POISON", word)
        dirty = rc.run_fresh(fm3d, case, world, x)
        monkeypatch.delenv("FM3D_DEBUG_POISON")
        rc.assert_same(dirty, clean, f"{case.name} at {x} under {word} vs unpoisoned")
        rc.check_reference(case, world, x, clean)
        rc.check_reference(case, world, x, dirty)
