"""The LM kernel's two layouts of image 2 ("Gather geometry"): the row-major pyramid
levels, and their column-major copies, in which the 64 lanes of a chunk -- 64 consecutive rows of one
image-1 column -- gather from 1-3 cache lines.  FM3D_LM_IMG2 = rows | cols forces one, auto (the
default) chooses per launch from the camera-2 pose.  The layout changes no result: the column copy is
pinned byte for byte against the row-major levels, and the LM's statuses, lmdif info, evaluation counts
and normals bit for bit between the layouts and against the oracle, on neighbourhoods that reach image
2's last columns and rows and the guards past them."""
import ctypes

import numpy as np
import pytest

from conftest import oracle_threads

pytestmark = pytest.mark.gpu

W, H, RAY = 96, 80, 8


def _lib(fm3d):
    L = fm3d.lib()
    L.fm3d_internal_level_cols.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p] + [ctypes.c_void_p] * 4
    L.fm3d_internal_level_cols.restype = ctypes.c_int
    L.fm3d_internal_lm_img2_cols.argtypes = [ctypes.c_void_p]
    L.fm3d_internal_lm_img2_cols.restype = ctypes.c_int
    return L


def _settings(fm3d, cam, **kw):
    s = fm3d.Settings.default()
    s.set_camera(cam)
    for k, v in kw.items():
        setattr(s, k, v)
    return s


# ---------------------------------------------------------------- the column copy
def _level_cols(fm3d, ctx, level):
    L = _lib(fm3d)
    w, h, hs = ctypes.c_int(0), ctypes.c_int(0), ctypes.c_int(0)
    n = ctypes.c_size_t(0)
    ctx.check(L.fm3d_internal_level_cols(ctx.handle, level, None, ctypes.byref(w), ctypes.byref(h), ctypes.byref(hs),
                                         ctypes.byref(n)))
    out = np.full(n.value, 0xA5, dtype=np.uint8)
    ctx.check(L.fm3d_internal_level_cols(ctx.handle, level, out.ctypes.data, None, None, None, None))
    return out, w.value, h.value, hs.value


def _check_copies(fm3d, ctx, no, levels):
    for L in range(levels + 1):
        row = no.pyramid(2, L)
        T, w, h, hs = _level_cols(fm3d, ctx, L)
        assert row.shape == (h, w) and hs >= h + 2 and T.size >= (w + 2) * hs
        # flat: the row-major level with its zero guard; T(x, y) = flat[y w + x] over (w + 2) x (h + 2)
        flat = np.zeros((h + 2) * w + w + 2, dtype=np.uint8)
        flat[:h * w] = row.ravel()
        x, y = np.meshgrid(np.arange(w + 2), np.arange(h + 2), indexing="ij")
        want = np.zeros_like(T)
        want[(x * hs + y).ravel()] = flat[(y * w + x).ravel()]  # everything else is guard: zero
        assert np.array_equal(T, want), f"level {L} ({w} x {h}, stride {hs})"
        assert not T[(w + 2) * hs:].any() and not T.reshape(-1)[:(w + 2) * hs].reshape(w + 2, hs)[:, h + 2:].any()


@pytest.mark.parametrize("sizes", [[(64, 48)], [(75, 59)], [(75, 59), (64, 48), (64, 48), (75, 59)]])
def test_column_copy_equals_row_major_levels(fm3d, synth, sizes):
    """every level's column-major copy against flat[y w + x] of the level the API returns, guards
    included; the longer sequence reuses one context's buffers across sizes and frame pairs"""
    rng = np.random.default_rng(5)
    ctx = fm3d.Context(_settings(fm3d, synth.Camera.reference(64), pyramids=3))
    try:
        no = fm3d.NormalOptimizer(ctx)
        for w, h in sizes:
            a, b = (rng.integers(1, 256, (h, w), dtype=np.uint8) for _ in range(2))  # no zero pixel: guards differ
            no.setImages(a, b)
            assert np.array_equal(no.pyramid(2, 0), b)
            _check_copies(fm3d, ctx, no, 3)
    finally:
        ctx.close()


# ---------------------------------------------------------------- LM on the two layouts
def _roll90(g12):
    """the same pair with camera 2 rolled 90 degrees about its optical axis"""
    Rz = np.eye(4)
    Rz[:2, :2] = [[0., -1.], [1., 0.]]
    return Rz @ g12


@pytest.fixture(scope="module")
def upright(synth):
    return synth.make_frame_pair(3000, W, H, seed=21)


@pytest.fixture(scope="module")
def rolled(synth, upright):
    return synth.make_frame_pair(3000, W, H, seed=21, g12=_roll90(upright.g12), cam=upright.cam)


def _border_points(synth, fm3d, pair):
    """ground-truth points whose ray-8 neighbourhoods project onto image 2's last columns or rows"""
    R2, t2 = fm3d.camera2_from_g12(pair.g12)
    uv = synth.project(pair.cam, pair.points, R2, t2)
    near = ((uv[:, 0] > W - RAY - 5) & (uv[:, 0] < W - RAY + 1)) | ((uv[:, 1] > H - RAY - 5) & (uv[:, 1] < H - RAY + 1))
    return pair.points[near][:160]


@pytest.fixture(scope="module")
def border(synth, fm3d, orc, upright):
    """the border points and the oracle's results on them, per pyramid count (computed once)"""
    P = _border_points(synth, fm3d, upright)
    R2, t2 = fm3d.camera2_from_g12(upright.g12)
    ref = {lv: orc.optimize_normals(upright.cam, R2, t2, upright.img1, upright.img2, lv, P, RAY, W, H,
                                    mode=orc.DETMATH, nthreads=oracle_threads()) for lv in (0, 3)}
    return P, ref


def _lm(fm3d, pair, P, layout, monkeypatch, levels=3, ray=RAY, **kw):
    """computeOptimizedNormals under FM3D_LM_IMG2 = layout: (status, info, nfev, kept, normals, cols)"""
    monkeypatch.setenv("FM3D_LM_IMG2", layout)
    monkeypatch.setenv("FM3D_LM_MAX_SECONDS", "20")
    ctx = fm3d.Context(_settings(fm3d, pair.cam, pixelsRay=ray, pyramids=levels, boundWidth=W, boundHeight=H, **kw))
    try:
        sct = fm3d.SingleCameraTriangulator(ctx)
        sct.set_g12(pair.g12)
        no = fm3d.NormalOptimizer(ctx, sct)
        no.setImages(pair.img1, pair.img2)
        assert _lib(fm3d).fm3d_internal_lm_img2_cols(ctx.handle) == -1
        kept, normals = no.computeOptimizedNormals(P)
        return (no.last_status, no.last_info, no.last_nfev, kept, normals,
                _lib(fm3d).fm3d_internal_lm_img2_cols(ctx.handle))
    finally:
        ctx.close()


def _same(a, b):
    for u, v in zip(a[:5], b[:5]):
        assert u.tobytes() == v.tobytes()


def _vs_oracle(run, ref, P, levels):
    st, info, nfev, kept, normals, _ = run
    L = levels + 1
    ok = ref["status"] == 0
    assert np.array_equal(st, ref["status"])
    assert np.array_equal(info[:, :L], ref["info"][:, :L]) and np.array_equal(nfev[:, :L], ref["nfev"][:, :L])
    assert kept.tobytes() == P[ok].tobytes() and normals.tobytes() == ref["normals"][ok].tobytes()


def test_border_points_reach_the_last_columns_and_rows(fm3d, orc, upright, border):
    """(CPU, oracle) the chosen points include kept points, and kept neighbourhoods whose level-0
    gather starts in the last column or row (floor(fx) >= w - 1 or floor(fy) >= h - 1): their
    windows read column w / row h, the guard of either layout"""
    P, ref = border
    R2, t2 = fm3d.camera2_from_g12(upright.g12)
    for lv in (0, 3):
        ok = np.nonzero(ref[lv]["status"] == 0)[0]
        assert len(ok) >= 5, len(ok)
        reach_x = reach_y = 0
        for i in ok:
            pix = orc.neighborhood(upright.cam, P[i], RAY, W, H)
            uv, st = orc.plane_to_image2(upright.cam, R2, t2, P[i], ref[lv]["normals"][i], pix, 2.4, size=(W, H))
            assert (st == 0).all()
            f = np.floor(uv.astype(np.float32))
            reach_x += f[:, 0].max() >= W - 1
            reach_y += f[:, 1].max() >= H - 1
        print(f"pyramids {lv}: {len(ok)} kept of {len(P)}, reach last column {reach_x}, last row {reach_y}")
        assert reach_x >= 1 or reach_y >= 1


@pytest.mark.parametrize("levels", [0, 3])
@pytest.mark.parametrize("safe", [0, 1])
def test_border_and_guard_reads_rows_equal_cols_equal_oracle(fm3d, upright, border, safe, levels, monkeypatch):
    monkeypatch.setenv("FM3D_LM_SAFE", str(safe))
    P, ref = border
    rows = _lm(fm3d, upright, P, "rows", monkeypatch, levels)
    cols = _lm(fm3d, upright, P, "cols", monkeypatch, levels)
    assert (rows[5], cols[5]) == (0, 1)
    _same(rows, cols)
    _vs_oracle(rows, ref[levels], P, levels)
    _vs_oracle(cols, ref[levels], P, levels)


def test_layout_choice_follows_the_pose(fm3d, upright, rolled, border, monkeypatch):
    """auto: the upright pair reads columns, the same pair rolled 90 degrees about the optical axis
    reads rows; each run equals its forced opposite bit for bit"""
    for pair, P, want, opposite in ((upright, border[0][:60], 1, "rows"), (rolled, rolled.points[:60], 0, "cols")):
        auto = _lm(fm3d, pair, P, "auto", monkeypatch)
        forced = _lm(fm3d, pair, P, opposite, monkeypatch)
        assert auto[5] == want and forced[5] == 1 - want
        _same(auto, forced)
        assert (auto[0] == 0).sum() >= 3
    with pytest.raises(fm3d.Fm3dError):
        _lm(fm3d, upright, border[0][:4], "diagonal", monkeypatch)


def test_linked_pairs_upright_and_rolled(fm3d, upright, rolled, monkeypatch):
    """one LM launch over an upright and a rolled pair reads rows (columns only if every pair chooses
    them); each pair's records equal its own unlinked run's"""
    monkeypatch.delenv("FM3D_LM_IMG2", raising=False)
    L = _lib(fm3d)
    s = _settings(fm3d, upright.cam, pixelsRay=RAY, pyramids=2, boundWidth=W, boundHeight=H)

    def mk(fp):
        c = fm3d.Context(s)
        fm3d.SingleCameraTriangulator(c).set_g12(fp.g12)
        return c, fm3d.Pipeline(c)

    ref, lay = [], []
    for fp in (upright, rolled):
        c, p = mk(fp)
        try:
            p.upload(fp.desc1, fp.desc2, fp.kp1, fp.kp2, fp.img1, fp.img2)
            k, _ = p.run()
            ref.append(p.records(k))
            lay.append(L.fm3d_internal_lm_img2_cols(c.handle))
        finally:
            c.close()
    assert lay == [1, 0] and all(len(r) > 50 for r in ref)
    (cm, m), (cl, l) = mk(upright), mk(rolled)
    try:
        m.link(l)
        m.submit(upright.desc1, upright.desc2, upright.kp1, upright.kp2, upright.img1, upright.img2)
        l.submit(rolled.desc1, rolled.desc2, rolled.kp1, rolled.kp2, rolled.img1, rolled.img2)
        assert m.wait()[0].tobytes() == ref[0].tobytes()
        assert l.wait()[0].tobytes() == ref[1].tobytes()
        assert L.fm3d_internal_lm_img2_cols(cl.handle) == 0 and L.fm3d_internal_lm_img2_cols(cm.handle) == 0
    finally:
        cm.close()
        cl.close()


def test_tree_mode_rows_equal_cols(fm3d, orc, upright, border, monkeypatch):
    P = border[0][:60]
    rows = _lm(fm3d, upright, P, "rows", monkeypatch, lmReduction=1)
    cols = _lm(fm3d, upright, P, "cols", monkeypatch, lmReduction=1)
    assert (rows[5], cols[5]) == (0, 1)
    _same(rows, cols)
    R2, t2 = fm3d.camera2_from_g12(upright.g12)
    ref = orc.optimize_normals(upright.cam, R2, t2, upright.img1, upright.img2, 3, P, RAY, W, H,
                               mode=orc.DETMATH | orc.TREE | orc.GRAM, nthreads=oracle_threads())
    _vs_oracle(cols, ref, P, 3)
    assert (ref["status"] == 0).sum() >= 3
