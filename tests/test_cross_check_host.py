"""Cross-check matching, the host side: the settings field and its key, the
argument rules that hold before any device is looked for, the C++ shim -- no GPU compute here."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

from conftest import ROOT


def test_settings_default_and_key(fm3d, tmp_path):
    assert fm3d.Settings.default().crossCheck == 0
    p = tmp_path / "s.yml"
    p.write_text("%YAML:1.0\nNNDR:\n   epsilon: 0.6\nFm3d:\n   guidedMatchPx: 2.5\n   crossCheck: 2\n")
    s = fm3d.Settings.load(str(p))
    assert s.crossCheck == 2 and s.guidedMatchPx == 2.5 and s.nndrEpsilon == 0.6
    p.write_text("%YAML:1.0\nNNDR:\n   epsilon: 0.6\nFm3d:\n   guidedMatchPx: 2.5\n")
    s = fm3d.Settings.load(str(p))
    assert s.crossCheck == 0 and s.guidedMatchPx == 2.5


def test_settings_field_is_last(fm3d):
    """an int appended after guidedMatchPx: the layout before it is unchanged"""
    names = [f[0] for f in fm3d.Settings._fields_]
    assert names[-2:] == ["guidedMatchPx", "crossCheck"]
    assert fm3d.Settings.crossCheck.offset == fm3d.Settings.guidedMatchPx.offset + 8


@pytest.mark.parametrize("bad", [-1, 3, 7])
def test_ctx_create_rejects_bad_setting(fm3d, bad):
    """a crossCheck outside {0, 1, 2}: FM3D_ERR_INVALID before any device is looked for"""
    s = fm3d.Settings.default()
    s.crossCheck = bad
    h = ctypes.c_void_p()
    assert fm3d.lib().fm3d_ctx_create(ctypes.byref(s), 0, ctypes.byref(h)) == fm3d.ERR_INVALID
    assert not h


def test_ctx_create_accepts_good_setting(fm3d):
    for good in (0, 1, 2):
        s = fm3d.Settings.default()
        s.crossCheck = good
        h = ctypes.c_void_p()
        rc = fm3d.lib().fm3d_ctx_create(ctypes.byref(s), 0, ctypes.byref(h))
        assert rc in (fm3d.FM3D_OK, fm3d.ERR_HIP)
        if rc == fm3d.FM3D_OK:
            fm3d.lib().fm3d_ctx_destroy(h)


def test_entry_points_null_context(fm3d):
    L = fm3d.lib()
    n = ctypes.c_int(0)
    dbl = ctypes.c_double
    for mode in (1, 2, 0):
        assert L.fm3d_match_mutual(None, None, 0, None, 0, 128, 1, dbl(0.6), mode, None,
                                   ctypes.byref(n)) == fm3d.ERR_INVALID
        assert L.fm3d_match_mutual_guided(None, None, 0, None, 0, 128, 1, None, None, dbl(0.6), dbl(1.0), mode, None,
                                          ctypes.byref(n)) == fm3d.ERR_INVALID


@pytest.mark.parametrize("bad", [0, 3, -1])
def test_python_mirror_rejects_bad_mode(fm3d, bad):
    """the Python mirror applies the C rule before any device work"""
    m = fm3d.DescriptorsMatcher(ctx=None)
    a = np.zeros((2, 128), dtype=np.uint8)
    k = np.zeros((2, 2), dtype=np.float32)
    with pytest.raises(fm3d.Fm3dError) as e:
        m.compareWithNNDRMutual(0.6, a, a, mode=bad)
    assert e.value.code == fm3d.ERR_INVALID
    with pytest.raises(fm3d.Fm3dError) as e:
        m.compareWithNNDRMutualGuided(0.6, a, a, k, k, 2.0, mode=bad)
    assert e.value.code == fm3d.ERR_INVALID
    with pytest.raises(fm3d.Fm3dError) as e:
        m.compareWithNNDRMutualGuided(0.6, a, a, k, k, 0.0, mode=1)
    assert e.value.code == fm3d.ERR_INVALID


def test_exports_listed(fm3d):
    assert "fm3d_match_mutual" in fm3d.EXPORTS and "fm3d_match_mutual_guided" in fm3d.EXPORTS
    assert hasattr(fm3d.lib(), "fm3d_match_mutual") and hasattr(fm3d.lib(), "fm3d_match_mutual_guided")


@pytest.mark.parametrize("mode", [1, 2])
def test_mgpu_two_devices_unsupported(fm3d, mode):
    """a device's context holds only its own queries, so the reverse search needs ndev == 1: refused
    without touching a device (the answer is the same with no GPU, one GPU or eight), aliased or not"""
    L = fm3d.lib()
    s = fm3d.Settings.default()
    s.crossCheck = mode
    for devs in ((0, 1), (0, 0)):
        d = np.array(devs, dtype=np.int32)
        h = ctypes.c_void_p()
        rc = L.fm3d_mgpu_create(ctypes.byref(s), 2, d.ctypes.data_as(ctypes.POINTER(ctypes.c_int32)), 2, 0,
                                ctypes.byref(h))
        assert rc == fm3d.ERR_UNSUPPORTED and not h
        why = (L.fm3d_mgpu_last_error(None) or b"").decode()
        assert "crossCheck" in why and "ndev" in why
    s.crossCheck = 5  # a bad value is invalid, not unsupported
    h = ctypes.c_void_p()
    d = np.array((0,), dtype=np.int32)
    assert L.fm3d_mgpu_create(ctypes.byref(s), 1, d.ctypes.data_as(ctypes.POINTER(ctypes.c_int32)), 1, 0,
                              ctypes.byref(h)) == fm3d.ERR_INVALID


CONSUMER = r"""
#include "fm3d_compat.hpp"
#include <vector>
using namespace fm3d::compat;
void use(Device& dev, SingleCameraTriangulator& sct, const DescMat& A, const DescMat& B,
         const std::vector<KeyPoint>& ka, const std::vector<KeyPoint>& kb) {
    DescriptorsMatcher dm(dev);
    std::vector<DMatch> m;
    dm.compareWithNNDRMutual(0.6, m, A, B);
    dm.compareWithNNDRMutual(0.6, m, A, B, 2);
    dm.compareWithNNDRMutualGuided(0.6, 2.0, sct, m, ka, kb, A, B);
    dm.compareWithNNDRMutualGuided(0.6, 2.0, sct, m, ka, kb, A, B, 2);
}
int main() { return 0; }
"""


def test_shim_methods_compile(tmp_path):
    p = tmp_path / "consumer.cpp"
    p.write_text(CONSUMER)
    r = subprocess.run(["g++", "-std=c++17", "-fsyntax-only", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"),
                        str(p)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
