"""Epipolar-guided matching, the host side: the essential matrix, the settings field and its key,
the argument rules -- no GPU compute here."""
import ctypes
import math

import numpy as np
import pytest


def essential_np(R2, t2):
    """E[r][c] = (T[r][0] R2[0][c] + T[r][1] R2[1][c]) + T[r][2] R2[2][c], T = [t2]x"""
    tx, ty, tz = (float(v) for v in t2)
    T = [[0.0, -tz, ty], [tz, 0.0, -tx], [-ty, tx, 0.0]]
    E = np.zeros((3, 3))
    for r in range(3):
        for c in range(3):
            E[r, c] = (T[r][0] * float(R2[0, c]) + T[r][1] * float(R2[1, c])) + T[r][2] * float(R2[2, c])
    return E


def test_epipolar_matrix_bitwise(fm3d, synth):
    g12 = synth.reference_g12()
    R2, t2 = fm3d.camera2_from_g12(g12)
    E = fm3d.epipolar_matrix(g12)
    assert E.shape == (3, 3) and np.isfinite(E).all() and np.abs(E).max() > 0.1
    assert np.array_equal(E, essential_np(R2, t2))
    # a point of the scene satisfies x2^T E x1 = 0 (normalised coordinates, no distortion involved)
    X = np.array([0.3, -0.2, 2.0])
    X2 = R2 @ X + t2
    assert abs((X2 / X2[2]) @ E @ (X / X[2])) < 1e-12
    # null arguments
    L = fm3d.lib()
    out = np.zeros(9)
    assert L.fm3d_epipolar_matrix(None, out.ctypes.data_as(ctypes.POINTER(ctypes.c_double))) == fm3d.ERR_INVALID
    assert L.fm3d_epipolar_matrix(np.ascontiguousarray(g12).ctypes.data_as(ctypes.POINTER(ctypes.c_double)),
                                  None) == fm3d.ERR_INVALID


def test_identity_pose_has_no_lines(fm3d):
    assert np.array_equal(fm3d.epipolar_matrix(np.eye(4)), np.zeros((3, 3)))


def test_settings_default_and_key(fm3d, tmp_path):
    assert fm3d.Settings.default().guidedMatchPx == 0
    p = tmp_path / "s.yml"
    p.write_text("%YAML:1.0\nNNDR:\n   epsilon: 0.6\nFm3d:\n   guidedMatchPx: 2.5\n")
    s = fm3d.Settings.load(str(p))
    assert s.guidedMatchPx == 2.5 and s.nndrEpsilon == 0.6
    p.write_text("%YAML:1.0\nNNDR:\n   epsilon: 0.6\n")
    assert fm3d.Settings.load(str(p)).guidedMatchPx == 0


@pytest.mark.parametrize("bad", [-1.0, -0.0 - 1e-300, math.nan, math.inf, -math.inf])
def test_ctx_create_rejects_bad_setting(fm3d, bad):
    """negative or non-finite guidedMatchPx: FM3D_ERR_INVALID before any device is looked for"""
    s = fm3d.Settings.default()
    s.guidedMatchPx = bad
    h = ctypes.c_void_p()
    assert fm3d.lib().fm3d_ctx_create(ctypes.byref(s), 0, ctypes.byref(h)) == fm3d.ERR_INVALID
    assert not h


def test_ctx_create_accepts_good_setting(fm3d):
    """0 (off) and a positive value pass the settings check: what remains is the device's answer"""
    for good in (0.0, 2.0):
        s = fm3d.Settings.default()
        s.guidedMatchPx = good
        h = ctypes.c_void_p()
        rc = fm3d.lib().fm3d_ctx_create(ctypes.byref(s), 0, ctypes.byref(h))
        assert rc in (fm3d.FM3D_OK, fm3d.ERR_HIP)
        if rc == fm3d.FM3D_OK:
            fm3d.lib().fm3d_ctx_destroy(h)


@pytest.mark.parametrize("bad", [0.0, -2.0, math.nan, math.inf])
def test_max_px_rejected(fm3d, bad):
    """a maxPx of 0, negative or not finite is FM3D_ERR_INVALID (the Python mirror applies the C rule
    before any device work; the C entry points are checked on the GPU, tests/test_guided_match.py)"""
    m = fm3d.DescriptorsMatcher(ctx=None)
    a = np.zeros((2, 128), dtype=np.uint8)
    k = np.zeros((2, 2), dtype=np.float32)
    with pytest.raises(fm3d.Fm3dError) as e:
        m.knn_match_guided(a, a, k, k, bad)
    assert e.value.code == fm3d.ERR_INVALID
    with pytest.raises(fm3d.Fm3dError) as e:
        m.compareWithNNDRGuided(0.6, a, a, k, k, bad)
    assert e.value.code == fm3d.ERR_INVALID


def test_guided_entry_points_null_context(fm3d):
    L = fm3d.lib()
    n = ctypes.c_int(0)
    assert L.fm3d_epipolar_lines(None, None, 0, None) == fm3d.ERR_INVALID
    assert L.fm3d_knn2_guided(None, None, 0, None, 0, 128, 1, None, None, ctypes.c_double(1.0), None) == fm3d.ERR_INVALID
    assert L.fm3d_match_nndr_guided(None, None, 0, None, 0, 128, 1, None, None, ctypes.c_double(0.6),
                                    ctypes.c_double(1.0), None, ctypes.byref(n)) == fm3d.ERR_INVALID
