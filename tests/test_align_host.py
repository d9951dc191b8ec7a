"""3D-3D alignment, the host side: the sampler, the three-point model, the count and
the refit against the plain-Python restatement (tests/align_pyref.py), bit for bit; the restatement's
RANSAC end to end on the quality case; the argument rules and the C++ shim -- no GPU compute here."""
import ctypes
import math
import os
import subprocess

import numpy as np
import pytest

import align_pyref as ref
from conftest import ROOT

SEEDS = (0, 3, 7)
MAX_DIST = 0.005


# ---------------------------------------------------------------- sampler
@pytest.mark.parametrize("M", [3, 4, 5, 1000, 2 ** 31 - 1])
@pytest.mark.parametrize("h", [0, 1, 4095])
def test_sampler_equals_restatement(fm3d, M, h):
    for seed in (0, 1, 0xDEADBEEFCAFEF00D, 2 ** 64 - 1):
        idx, ok = fm3d.ransac_sample3(seed, h, M)
        want = ref.sample3(seed, h, M)
        assert ok == (want is not None)
        if ok:
            assert list(idx) == want and len(set(idx.tolist())) == 3 and 0 <= idx.min() and idx.max() < M


def test_sampler_is_a_prefix_of_the_eight_point_draws(fm3d):
    """the same draws as fm3d_ransac_sample, the first three distinct ones"""
    for h in range(50):
        i3, ok3 = fm3d.ransac_sample3(5, h, 40)
        i8, ok8 = fm3d.ransac_sample(5, h, 40)
        assert ok3 and ok8 and list(i3) == list(i8[:3])


def test_sampler_few_matches(fm3d):
    for M in (0, 1, 2):
        idx, ok = fm3d.ransac_sample3(3, 0, M)
        assert not ok and list(idx) == [-1, -1, -1] and ref.sample3(3, 0, M) is None
    for M in (3, 4):  # enough matches: valid whenever the restatement's 64 draws hold three values
        got = [fm3d.ransac_sample3(9, h, M) for h in range(64)]
        assert all(ok == (ref.sample3(9, h, M) is not None) for h, (_, ok) in enumerate(got))
        assert sum(ok for _, ok in got) >= 60
    L = fm3d.lib()
    out = (ctypes.c_int32 * 3)()
    assert L.fm3d_ransac_sample3(ctypes.c_uint64(0), 0, 100, None) == fm3d.ERR_INVALID
    assert L.fm3d_ransac_sample3(ctypes.c_uint64(0), -1, 100, out) == fm3d.ERR_INVALID
    assert L.fm3d_ransac_sample3(ctypes.c_uint64(0), 0, -1, out) == fm3d.ERR_INVALID


# ---------------------------------------------------------------- three-point model
def random_triples(n, seed=17):
    rng = np.random.default_rng(seed)
    return rng.uniform(-2.0, 2.0, (n, 3, 3)), rng.uniform(-2.0, 2.0, (n, 3, 3))


def det3(m):
    return float(np.linalg.det(np.asarray(m[:9]).reshape(3, 3)))


def test_from3_bitwise_random(fm3d, orc):
    """unrelated triples (a general cross matrix) and rigidly related ones (what a good sample is)"""
    a, b = random_triples(150)
    R = ref.rodrigues([0.3, -0.5, 0.8], 0.7)
    pairs = list(zip(a, b)) + [(p, p @ R.T + [0.1, -0.2, 0.3]) for p in a[:100]]
    nvalid = 0
    for p, q in pairs:
        m, ok = fm3d.rigid_from3(p, q)
        mr, okr = ref.from3(orc, p, q)
        assert ok == okr and np.array_equal(m, mr)
        if ok:
            assert abs(det3(m) - 1) < 1e-12
        nvalid += ok
    assert nvalid >= 245
    for p in a[:100]:  # a rigid triple comes back to within rounding
        m, ok = fm3d.rigid_from3(p, p @ R.T + [0.1, -0.2, 0.3])
        assert ok and np.abs(m[:9].reshape(3, 3) - R).max() < 1e-9 and np.abs(m[9:] - [0.1, -0.2, 0.3]).max() < 1e-9


def test_from3_collinear_is_invalid(fm3d, orc):
    """three points on a line: the centred cross matrix has rank 1.  An exactly representable line gives
    a second singular value of exactly zero"""
    a = np.array([[0.0, 0.0, 1.0], [1.0, 2.0, 3.0], [2.0, 4.0, 5.0]])
    m, ok = fm3d.rigid_from3(a, a + 1.0)
    mr, okr = ref.from3(orc, a, a + 1.0)
    assert not ok and not okr and not m.any() and np.array_equal(m, mr)
    # a general line: whatever the restatement says, bit for bit
    rng = np.random.default_rng(4)
    for _ in range(20):
        p, d = rng.uniform(-1, 1, 3), rng.uniform(-1, 1, 3)
        a = np.stack([p, p + 0.37 * d, p - 1.21 * d])
        m, ok = fm3d.rigid_from3(a, a)
        mr, okr = ref.from3(orc, a, a)
        assert ok == okr and np.array_equal(m, mr) and (ok or not m.any())


def test_from3_two_equal_points(fm3d, orc):
    """duplicate matches can put one pair twice into a sample: rank <= 1"""
    a, b = random_triples(20, seed=5)
    for p, q in zip(a, b):
        p[2], q[2] = p[0], q[0]
        m, ok = fm3d.rigid_from3(p, q)
        mr, okr = ref.from3(orc, p, q)
        assert ok == okr and np.array_equal(m, mr) and (ok or not m.any())
    p = np.array([[1.0, 2.0, 3.0], [1.0, 2.0, 3.0], [1.0, 2.0, 3.0]])
    assert not fm3d.rigid_from3(p, p)[1]


def test_from3_nan_and_inf(fm3d, orc):
    a, b = random_triples(1, seed=2)
    for bad in (math.nan, math.inf, -math.inf):
        for which in (0, 1):
            p, q = a[0].copy(), b[0].copy()
            (p if which == 0 else q)[1, 2] = bad
            m, ok = fm3d.rigid_from3(p, q)
            assert not ok and not m.any() and not ref.from3(orc, p, q)[1]
    L = fm3d.lib()
    buf, out = (ctypes.c_double * 9)(), (ctypes.c_double * 12)()
    assert L.fm3d_rigid_from3(None, buf, out) == fm3d.ERR_INVALID
    assert L.fm3d_rigid_from3(buf, None, out) == fm3d.ERR_INVALID
    assert L.fm3d_rigid_from3(buf, buf, None) == fm3d.ERR_INVALID


def test_from3_mirrored_triangle_stays_a_rotation(fm3d, orc):
    """b is a's mirror image.  The orthogonal matrices that map the centred a onto the centred b with
    zero residual include the reflection itself -- V U^T with a third singular pair of the SVD's own
    choosing can be it -- and one rotation (the triangle turned over); the cross-product completion
    gives the rotation, without a determinant test."""
    rng = np.random.default_rng(8)
    S = np.diag([-1.0, 1.0, 1.0])
    for _ in range(20):
        a = rng.uniform(-1, 1, (3, 3))
        b = a @ S.T + [0.5, 0.0, -0.25]
        ac, bc = a - a.mean(0), b - b.mean(0)
        assert np.abs(ac @ S.T - bc).max() < 1e-15  # the reflection is a zero-residual optimum
        m, ok = fm3d.rigid_from3(a, b)
        mr, okr = ref.from3(orc, a, b)
        assert ok and okr and np.array_equal(m, mr)
        R = m[:9].reshape(3, 3)
        assert abs(np.linalg.det(R) - 1) < 1e-12 and np.abs(R @ R.T - np.eye(3)).max() < 1e-12
        assert np.abs(a @ R.T + m[9:] - b).max() < 1e-12


# ---------------------------------------------------------------- count
def test_count_equals_restatement(fm3d, orc):
    p, r = ref.quality_case(orc, 0)
    a, b = r["a"], r["b"]
    q = np.asarray(p["matches"]["queryIdx"])
    t = np.asarray(p["matches"]["trainIdx"])
    na, nb = p["nA"][q], p["nB"][t]
    for h in (0, 1, r["best"]):
        m = r["models"][h]
        n, mask = fm3d.rigid_count(m, a, b, MAX_DIST)
        want = ref.inliers(m, a, b, MAX_DIST)
        assert n == int(want.sum()) == r["counts"][h] and np.array_equal(mask, want)
        for mc in (-1.0, 0.0, 0.9, 1.0):
            n, mask = fm3d.rigid_count(m, a, b, MAX_DIST, na, nb, mc)
            want = ref.inliers(m, a, b, MAX_DIST, na, nb, mc)
            assert n == int(want.sum()) and np.array_equal(mask, want)
    # the normals are a second test: with the best model a wrong pair that lies close fails it, a true one passes
    n0, m0 = fm3d.rigid_count(r["model"], a, b, 1.0)
    n1, m1 = fm3d.rigid_count(r["model"], a, b, 1.0, na, nb, 0.99)
    assert n0 > n1 >= int(p["true"].sum()) and m1[p["true"]].all()
    # a NaN coordinate or normal fails
    y = a.copy()
    y[0, 0] = math.nan
    assert m0[0] and not fm3d.rigid_count(r["model"], y, b, 1.0)[1][0]
    z = nb.copy()
    z[0, 1] = math.nan
    assert not fm3d.rigid_count(r["model"], a, b, 1.0, na, z, -1.0)[1][0]
    L = fm3d.lib()
    one = ctypes.c_double(1.0)
    buf = (ctypes.c_double * 12)()
    assert L.fm3d_rigid_count(None, None, None, None, None, 0, one, one, None) == fm3d.ERR_INVALID
    assert L.fm3d_rigid_count(buf, buf, buf, buf, None, 1, one, one, None) == fm3d.ERR_INVALID
    assert L.fm3d_rigid_count(buf, None, buf, None, None, 1, one, one, None) == fm3d.ERR_INVALID
    assert L.fm3d_rigid_count(buf, buf, buf, None, None, -1, one, one, None) == fm3d.ERR_INVALID


# ---------------------------------------------------------------- refit
def refit_inputs(n, seed=31):
    """n pairs around a known motion, a third of them far off (so the predicate matters)"""
    rng = np.random.default_rng(seed)
    a = rng.uniform(-1, 1, (n, 3)) + [0, 0, 2.0]
    R = ref.rodrigues([0.2, 0.9, -0.4], 0.3)
    t = np.array([0.05, -0.1, 0.2])
    b = a @ R.T + t + rng.normal(0, 0.001, (n, 3))
    off = rng.random(n) < 0.33
    b[off] += rng.uniform(0.05, 0.5, (int(off.sum()), 3))
    m0 = np.concatenate([R.ravel(), t + 0.002])  # a model slightly off
    return a, b, m0


@pytest.mark.parametrize("n", [1023, 1024, 1025, 2049])
def test_refit_sums_pin_the_tile_order(fm3d, orc, n):
    a, b, m0 = refit_inputs(n)
    m, ok, S = fm3d.rigid_refit(m0, a, b, MAX_DIST, sums=True)
    mr, okr, Sr = ref.refit(orc, m0, a, b, MAX_DIST)
    assert ok and okr and np.array_equal(S, Sr) and np.array_equal(m, mr)
    inl = ref.inliers(m0, a, b, MAX_DIST)
    assert S[6] == int(inl.sum()) and 0.4 * n < S[6] < 0.8 * n
    # the order is part of the contract: adding the same terms one after the other gives other bits
    plain = [0.0] * 3
    for row in a[inl].tolist():
        for k in range(3):
            plain[k] = plain[k] + row[k]
    assert not np.array_equal(np.array(plain), S[:3]) and np.allclose(plain, S[:3], rtol=1e-12)
    # and the refit moves the model towards the motion that made the data
    assert abs(det3(m) - 1) < 1e-12
    assert np.abs(m[9:] - [0.05, -0.1, 0.2]).max() < np.abs(m0[9:] - [0.05, -0.1, 0.2]).max()


def test_refit_with_normals_and_invalid(fm3d, orc):
    a, b, m0 = refit_inputs(1500)
    rng = np.random.default_rng(3)
    na = rng.normal(size=a.shape)
    na /= np.linalg.norm(na, axis=1)[:, None]
    nb = na @ m0[:9].reshape(3, 3).T
    nb[::5] = -nb[::5]  # every fifth pair faces the other way
    m, ok, S = fm3d.rigid_refit(m0, a, b, MAX_DIST, na, nb, 0.5, sums=True)
    mr, okr, Sr = ref.refit(orc, m0, a, b, MAX_DIST, na, nb, 0.5)
    assert ok and okr and np.array_equal(S, Sr) and np.array_equal(m, mr)
    assert S[6] < fm3d.rigid_refit(m0, a, b, MAX_DIST, sums=True)[2][6]
    # fewer than three pairs in: invalid, a zero model
    for keep in (0, 2):
        far = b + 10.0
        far[:keep] = b[:keep]
        m, ok, S = fm3d.rigid_refit(m0, a, far, MAX_DIST, sums=True)
        mr, okr, Sr = ref.refit(orc, m0, a, far, MAX_DIST)
        assert not ok and not okr and not m.any() and S[6] <= keep
        assert np.array_equal(S, Sr, equal_nan=True)
    # a NaN pair is out of every sum
    y = a.copy()
    y[7] = math.nan
    m, ok, S = fm3d.rigid_refit(m0, y, b, MAX_DIST, sums=True)
    mr, okr, Sr = ref.refit(orc, m0, y, b, MAX_DIST)
    assert ok and np.isfinite(S).all() and np.array_equal(S, Sr) and np.array_equal(m, mr)
    L = fm3d.lib()
    one = ctypes.c_double(1.0)
    buf = (ctypes.c_double * 12)()
    assert L.fm3d_rigid_refit(None, buf, buf, None, None, 1, one, one, buf, None) == fm3d.ERR_INVALID
    assert L.fm3d_rigid_refit(buf, buf, buf, None, None, 1, one, one, None, None) == fm3d.ERR_INVALID
    assert L.fm3d_rigid_refit(buf, buf, buf, None, buf, 1, one, one, buf, None) == fm3d.ERR_INVALID


# ---------------------------------------------------------------- RANSAC end to end (restatement)
# What the restatement alone is off on the quality case, computed on the CPU by tests/align_pyref.py
# (DESIGN.md §3.1e): the best three-point model per seed, and the model after four rounds of the refit
# (the same for the three seeds: they end on the same 424 pairs).  The library is held to twice these.
ROT_ERR_DEG = {0: 0.1105, 3: 0.1741, 7: 0.1078}
ROT_ERR_REFINED_DEG = 0.0057


@pytest.mark.parametrize("seed", SEEDS)
def test_restatement_meets_the_caps(orc, seed):
    """600 pairs, 30 % of them wrong, 1 mm noise, maxDist 5 mm, 256 hypotheses: >= 99 % of the true pairs
    kept, <= 1 % of the wrong ones, and four rounds of the refit do not raise the rotation error"""
    p, r = ref.quality_case(orc, seed)
    _, r4 = ref.quality_case(orc, seed, refine=4)
    true = p["true"]
    assert len(true) == 600 and 150 <= int((~true).sum()) <= 210
    for name, run in (("unrefined", r), ("refine=4", r4)):
        kt, kw = int((run["mask"] & true).sum()), int((run["mask"] & ~true).sum())
        print(name, "seed", seed, ": kept", kt, "of", int(true.sum()), "true pairs and", kw, "of", int((~true).sum()),
              "wrong")
        assert kt >= 0.99 * true.sum() and kw <= 0.01 * (~true).sum()
    e0, e4 = ref.rot_err_deg(r["g"][:3, :3], p["R"]), ref.rot_err_deg(r4["g"][:3, :3], p["R"])
    print("rotation error %.4f deg, refined %.4f deg; t error %.2e m, refined %.2e m; rounds %s" %
          (e0, e4, np.linalg.norm(r["g"][:3, 3] - p["t"]), np.linalg.norm(r4["g"][:3, 3] - p["t"]), r4["roundCounts"]))
    assert e4 <= e0
    assert abs(e0 - ROT_ERR_DEG[seed]) < 1e-4 and abs(e4 - ROT_ERR_REFINED_DEG) < 1e-4
    assert r["best"] >= 0 and r["counts"][r["best"]] == r["counts"].max() == int(r["mask"].sum())
    assert r["best"] == int(np.nonzero(r["counts"] == r["counts"].max())[0][0])
    assert r4["adopted"] >= 1 and (np.diff(r4["roundCounts"][:1 + r4["adopted"]]) >= 0).all()


@pytest.mark.parametrize("seed", SEEDS)
def test_host_chain_equals_restatement_and_meets_the_bounds(fm3d, orc, seed):
    """the same RANSAC and rounds driven through the four host functions: every hypothesis's sample,
    model and count, the best model and each round, bit for bit; the pose within twice the
    restatement's error"""
    p, r = ref.quality_case(orc, seed)
    _, r4 = ref.quality_case(orc, seed, refine=4)
    a, b = r["a"], r["b"]
    H = len(r["counts"])
    counts = np.full(H, -1, dtype=np.int32)
    models = np.zeros((H, 12))
    for h in range(H):
        idx, ok = fm3d.ransac_sample3(seed, h, len(a))
        if ok:
            models[h], ok = fm3d.rigid_from3(a[idx], b[idx])
        if ok:
            counts[h] = fm3d.rigid_count(models[h], a, b, MAX_DIST)[0]
    assert np.array_equal(counts, r["counts"]) and np.array_equal(models, r["models"])
    m, cur = models[r["best"]].copy(), int(counts[r["best"]])
    assert ref.rot_err_deg(m[:9].reshape(3, 3), p["R"]) <= 2 * ROT_ERR_DEG[seed]
    for k in range(4):
        mc, ok = fm3d.rigid_refit(m, a, b, MAX_DIST)
        cc = fm3d.rigid_count(mc, a, b, MAX_DIST)[0] if ok else -1
        assert np.array_equal(mc, r4["roundModels"][k]) and cc == r4["roundCounts"][1 + k]
        if not (ok and cc >= cur):
            break
        m, cur = mc, cc
    assert np.array_equal(m, r4["model"])
    assert ref.rot_err_deg(m[:9].reshape(3, 3), p["R"]) <= 2 * ROT_ERR_REFINED_DEG


def test_restatement_other_sizes(orc):
    """the recipe at N = 64 / H = 64: the same picture"""
    p = ref.model_pair(N=64)
    r = ref.align(orc, p["A"], p["B"], p["matches"], MAX_DIST, 64, 0)
    true = p["true"]
    assert int((r["mask"] & true).sum()) >= 0.99 * true.sum() and int((r["mask"] & ~true).sum()) == 0


# ---------------------------------------------------------------- interface
def test_exports_listed(fm3d):
    names = ("fm3d_align_points", "fm3d_match_models", "fm3d_ransac_sample3", "fm3d_rigid_from3", "fm3d_rigid_count",
             "fm3d_rigid_refit")
    for n in names:
        assert n in fm3d.EXPORTS and hasattr(fm3d.lib(), n)
    assert ctypes.sizeof(fm3d.AlignOpts) == 32
    assert [fm3d.AlignOpts.hypotheses.offset, fm3d.AlignOpts.refineIters.offset, fm3d.AlignOpts.maxDist.offset,
            fm3d.AlignOpts.minNormalCos.offset, fm3d.AlignOpts.seed.offset] == [0, 4, 8, 16, 24]


def test_opts_layout_matches_the_header(tmp_path):
    src = ('#include <stdio.h>\n#include <stddef.h>\n#include "fm3d.h"\nint main(void){printf("%zu %zu %zu %zu %zu %zu\\n",'
           "sizeof(fm3d_align_opts), offsetof(fm3d_align_opts, hypotheses), offsetof(fm3d_align_opts, refineIters),"
           "offsetof(fm3d_align_opts, maxDist), offsetof(fm3d_align_opts, minNormalCos), offsetof(fm3d_align_opts, seed));"
           "return 0;}")
    c, exe = tmp_path / "o.c", tmp_path / "o"
    c.write_text(src)
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), str(c), "-o", str(exe)], check=True)
    out = subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()
    assert [int(v) for v in out] == [32, 0, 4, 8, 16, 24]


def test_align_null_context(fm3d):
    L = fm3d.lib()
    n, best = ctypes.c_int(0), ctypes.c_int(0)
    g = (ctypes.c_double * 16)()
    o = fm3d.AlignOpts(16, 0, 1.0, 0.0, 0)
    assert L.fm3d_align_points(None, None, None, 0, None, None, 0, None, 0, ctypes.byref(o), g, None, None,
                               ctypes.byref(n), ctypes.byref(best), None, None, None, None, None) == fm3d.ERR_INVALID
    assert L.fm3d_match_models(None, None, None, None, 0, None, None, None, 0, 128, 1, ctypes.c_double(0.8),
                               ctypes.byref(o), None, ctypes.byref(n), g, None, None, ctypes.byref(n), ctypes.byref(best),
                               None, None, None, None, None) == fm3d.ERR_INVALID


@pytest.mark.parametrize("kw", [dict(max_dist=0.0), dict(max_dist=-1.0), dict(max_dist=math.nan), dict(max_dist=math.inf),
                                dict(hypotheses=0), dict(hypotheses=-3), dict(refine=-1), dict(refine=17),
                                dict(min_normal_cos=1.5), dict(min_normal_cos=-1.01), dict(min_normal_cos=math.nan)])
def test_python_mirror_rejects_bad_options(fm3d, kw):
    """the Python mirror applies the C rules before any device work (the C entry point itself is
    checked on the GPU, tests/test_gpu_align.py)"""
    al = fm3d.ModelAligner(ctx=None)
    pts = np.zeros((4, 3))
    m = np.zeros(3, dtype=fm3d.DMATCH)
    args = dict(max_dist=0.01)
    args.update(kw)
    with pytest.raises(fm3d.Fm3dError) as e:
        al.align(pts, pts, m, **args)
    assert e.value.code == fm3d.ERR_INVALID
    with pytest.raises(fm3d.Fm3dError) as e:
        al.match_and_align(np.zeros((4, 128), dtype=np.uint8), np.zeros((4, 128), dtype=np.uint8), pts, pts, 0.8, **args)
    assert e.value.code == fm3d.ERR_INVALID


def test_python_mirror_rejects_one_normal_array(fm3d):
    al = fm3d.ModelAligner(ctx=None)
    pts = np.zeros((4, 3))
    with pytest.raises(fm3d.Fm3dError) as e:
        al.align(pts, pts, np.zeros(3, dtype=fm3d.DMATCH), 0.01, normals_a=pts)
    assert e.value.code == fm3d.ERR_INVALID
    with pytest.raises(fm3d.Fm3dError):
        fm3d.rigid_count(np.zeros(12), pts, pts, 0.01, normals_b=pts)


CONSUMER = r"""
#include "fm3d_compat.hpp"
#include <vector>
using namespace fm3d::compat;
Matx44d use(Device& d, const std::vector<Vec3d>& a, const std::vector<Vec3d>& b, const std::vector<DMatch>& m) {
    std::vector<DMatch> in;
    Matx44d g = alignModels(d, a, b, m, 0.005);
    g = alignModels(d, a, b, m, 0.005, &in, 4096, 7u, 4, &a, &b, 0.9);
    double pa[9] = {0}, pb[9] = {0}, model[12], sums[16];
    int32_t idx[3];
    fm3d_ransac_sample3(7u, 0, (int)m.size(), idx);
    fm3d_rigid_from3(pa, pb, model);
    fm3d_rigid_count(model, pa, pb, nullptr, nullptr, 3, 1e-3, 0.0, nullptr);
    fm3d_rigid_refit(model, pa, pb, nullptr, nullptr, 3, 1e-3, 0.0, model, sums);
    return g;
}
int main() { return 0; }
"""


def test_shim_function_compiles(tmp_path):
    p = tmp_path / "consumer.cpp"
    p.write_text(CONSUMER)
    r = subprocess.run(["g++", "-std=c++17", "-fsyntax-only", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"),
                        str(p)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
