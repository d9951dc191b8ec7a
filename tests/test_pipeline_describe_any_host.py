"""fm3d_pipeline_describe_any's host side, no GPU: the header declares the call and the keep rule, the
library exports them, and the keep rule -- fm3d_patch_keypoint_kept, here through its settings-only form
since a context needs a device -- gives the oracle's answer: whether orb_compute / brisk_compute /
freak_compute / surf_describe keep the centred keypoint of a random size x size image, at the edges on
both sides of every threshold."""
import ctypes
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

EDGES = (52, 54, 62, 64, 128, 632, 634, 678, 680)
KEPT = {  # the oracle's answers, written down: the smallest kept edge per extractor
    ("ORB", 31): 64,
    ("ORB", 26): 54,
    ("BRISK", None): 634,
    ("FREAK", None): 680,
}


def header():
    with open(os.path.join(ROOT, "include", "fm3d.h")) as f:
        return f.read()


def args_of(name):
    decl = re.search(r"int %s\(([^;]*)\);" % name, header())
    assert decl, name + " is not declared"
    return " ".join(decl.group(1).split())


def test_header_declares_the_calls():
    assert args_of("fm3d_pipeline_describe_any") == (
        "fm3d_ctx *ctx, int source, const fm3d_record *recordsDev, int n, void *desc, double *frames, "
        "uint8_t *patches, fm3d_describe_stats *stats")
    assert args_of("fm3d_patch_keypoint_kept") == "const fm3d_ctx *ctx, int size, int *kept"
    assert args_of("fm3d_patch_keypoint_kept_for") == "const fm3d_settings *s, int size, int *kept"


def test_library_exports_the_symbols(fm3d):
    for name in ("fm3d_pipeline_describe_any", "fm3d_patch_keypoint_kept", "fm3d_patch_keypoint_kept_for"):
        assert name in fm3d.EXPORTS
        assert hasattr(fm3d.lib(), name)
    assert hasattr(fm3d.Pipeline, "describe_any")
    assert hasattr(fm3d.Features, "patch_keypoint_kept")


def kept(fm3d, s, size):
    k = ctypes.c_int(-1)
    assert fm3d.lib().fm3d_patch_keypoint_kept_for(ctypes.byref(s), size, ctypes.byref(k)) == fm3d.FM3D_OK
    assert k.value in (0, 1)
    return bool(k.value)


def centred(fm3d, size):
    kp = np.zeros(1, dtype=fm3d.KEYPOINT)
    kp["x"] = kp["y"] = size // 2
    kp["size"], kp["angle"], kp["response"] = size, -1, 1
    return kp


@pytest.fixture(scope="module")
def images():
    rng = np.random.default_rng(11)
    return {e: rng.integers(0, 256, (e, e), dtype=np.uint8) for e in EDGES + (22,)}


@pytest.mark.parametrize("extractor,edge_threshold", list(KEPT))
def test_keep_rule_equals_the_oracle(fm3d, orc, images, extractor, edge_threshold):
    s = fm3d.Settings.default()
    s.extractorType = getattr(fm3d, "FEAT_" + extractor)
    if edge_threshold is not None:
        s.orbEdgeThreshold = edge_threshold
    for e in EDGES:
        kp = centred(fm3d, e)
        if extractor == "ORB":
            ref = orc.orb_compute(images[e], kp, edgeThreshold=edge_threshold)[0]
        elif extractor == "BRISK":
            ref = orc.brisk_compute(images[e], kp)[0]
        else:
            ref = orc.freak_compute(images[e], kp)[0]
        assert len(ref) in (0, 1)
        assert (len(ref) == 1) == (e >= KEPT[extractor, edge_threshold]), (extractor, e, "the oracle's table moved")
        assert kept(fm3d, s, e) == (len(ref) == 1), (extractor, edge_threshold, e)


def test_surf_and_sift(fm3d, orc, images):
    s = fm3d.Settings.default()
    s.extractorType = fm3d.FEAT_SURF
    for e in (22, 128):
        ref = orc.surf_describe(images[e], centred(fm3d, e))[0]
        assert kept(fm3d, s, e) == (len(ref) == 1), e
        assert len(ref) == 1  # the wavelet, 2 * round(2 * 1.2 e / 9), is about half the edge
    s.extractorType = fm3d.FEAT_SIFT
    assert all(kept(fm3d, s, e) for e in (2, 22, 128, 680))


def test_refusals(fm3d):
    L = fm3d.lib()
    s = fm3d.Settings.default()
    k = ctypes.c_int(0)
    assert L.fm3d_patch_keypoint_kept_for(None, 128, ctypes.byref(k)) == fm3d.ERR_INVALID
    assert L.fm3d_patch_keypoint_kept_for(ctypes.byref(s), 128, None) == fm3d.ERR_INVALID
    assert L.fm3d_patch_keypoint_kept_for(ctypes.byref(s), 0, ctypes.byref(k)) == fm3d.ERR_INVALID
    assert L.fm3d_patch_keypoint_kept(None, 128, ctypes.byref(k)) == fm3d.ERR_INVALID
    s.extractorType = fm3d.FEAT_OTHER
    assert L.fm3d_patch_keypoint_kept_for(ctypes.byref(s), 128, ctypes.byref(k)) == fm3d.ERR_UNSUPPORTED
