"""The refit on the inliers ("Refinement"), the host side: fm3d_epipolar_normal45 and
fm3d_epipolar_refit against the plain-Python restatement (tests/verify_refit_pyref.py), bit for bit; the
summation order pinned; the eigenvector against numpy.linalg.eigh; the invalid cases, the argument rules,
the restatement's quality on noisy keypoints and the C++ shim -- no GPU compute here."""
import ctypes
import math
import os
import subprocess

import numpy as np
import pytest

import verify_pyref as ref
import verify_refit_pyref as rr
from conftest import ROOT

SIZES = [8, 9, 257, 1024, 1025, 2049]


@pytest.fixture(scope="module")
def case(synth, orc):
    return ref.reference_case(synth, orc)


def fixture(case, M):
    """the reference case's first M coordinate pairs (cyclically above its 1,800) and its best model"""
    idx = np.arange(M) % len(case["x1"])
    return case["ref"]["E"], case["x1"][idx], case["x2"][idx], case["tau"]


@pytest.fixture(scope="module")
def restated(orc, case):
    """per M: the restatement's normal matrix (tree and index order), count, and refit -- computed once"""
    out = {}
    for M in SIZES:
        E, x1, x2, tau = fixture(case, M)
        N, cnt = rr.normal45(E, x1, x2, tau)
        Ni, _ = rr.normal45(E, x1, x2, tau, order="index")
        out[M] = dict(N=N, Ni=Ni, cnt=cnt, refit=rr.refit_from_normal(orc, N))
    return out


# ---------------------------------------------------------------- bit for bit
@pytest.mark.parametrize("M", SIZES)
def test_normal45_and_refit_equal_restatement(fm3d, case, restated, M):
    E, x1, x2, tau = fixture(case, M)
    want = restated[M]
    N, cnt = fm3d.epipolar_normal45(E, x1, x2, tau)
    assert cnt == want["cnt"] == fm3d.epipolar_count(E, x1, x2, tau)[0]
    assert N.tobytes() == np.array(want["N"]).tobytes()
    assert N[44] == cnt  # a[8] = 1: the last entry counts the pairs in
    Eo, ok = fm3d.epipolar_refit(E, x1, x2, tau)
    Er, okr = want["refit"]
    assert ok == okr == (cnt >= 8) and Eo.tobytes() == np.ascontiguousarray(Er).tobytes()
    assert ok or not Eo.any()


def test_summation_order_is_pinned(restated):
    """the tree's sum differs from the index-order sum in some bit, at every size above one leaf's
    worth: a library that added in another order would not pass the test above"""
    differ = {M: sum(a != b for a, b in zip(r["N"], r["Ni"])) for M, r in restated.items()}
    print("entries of 45 whose tree sum differs from the index-order sum:", differ)
    assert all(differ[M] > 0 for M in (257, 1024, 1025, 2049))


def test_valid_at_the_minimum(fm3d, orc, case):
    """eight and nine pairs that the model accepts: a valid refit, the restatement's bits"""
    E, tau = case["ref"]["E"], case["tau"]
    inl = np.nonzero(case["ref"]["mask"])[0]
    for M in (8, 9):
        x1, x2 = case["x1"][inl[:M]], case["x2"][inl[:M]]
        Eo, ok = fm3d.epipolar_refit(E, x1, x2, tau)
        Er, okr = rr.refit(orc, E, x1, x2, tau)
        assert ok and okr and np.array_equal(Eo, Er)


# ---------------------------------------------------------------- against numpy
# the largest entry-wise difference, up to sign, between E' and project(numpy.linalg.eigh's eigenvector of
# the smallest eigenvalue) over the fixtures with a valid refit, measured on the CPU: 1.34e-13 (M = 257);
# ten times that, for other BLAS builds
EIGH_BOUND = 10 * 1.34e-13


def test_refit_against_numpy_eigh(fm3d, orc, case, restated):
    worst = 0.0
    for M in SIZES:
        E, x1, x2, tau = fixture(case, M)
        Eo, ok = fm3d.epipolar_refit(E, x1, x2, tau)
        if not ok:
            continue
        S = np.zeros((9, 9))
        for (r, c), v in zip(rr.PAIRS, restated[M]["N"]):
            S[r, c] = S[c, r] = v
        w, v = np.linalg.eigh(S)
        En = ref.project(orc, v[:, 0])
        d = min(np.abs(En - Eo).max(), np.abs(En + Eo).max())
        print("M", M, "against numpy.linalg.eigh:", d)
        worst = max(worst, d)
    assert 0.0 < worst < EIGH_BOUND
    # the result is an essential matrix: singular values (1, 1, 0)
    assert np.abs(np.linalg.svd(Eo)[1] - [1, 1, 0]).max() < 1e-12


# ---------------------------------------------------------------- invalid
def test_invalid_refits(fm3d, orc, case):
    E, x1, x2, tau = fixture(case, 257)
    inl = np.nonzero(ref.inliers(E, x1, x2, tau))[0]
    # fewer than 8 pairs in
    for k in (0, 1, 7):
        Eo, ok = fm3d.epipolar_refit(E, x1[inl[:k]], x2[inl[:k]], tau)
        assert not ok and not Eo.any() and not rr.refit(orc, E, x1[inl[:k]], x2[inl[:k]], tau)[1]
    # the zero model accepts nothing
    Eo, ok = fm3d.epipolar_refit(np.zeros((3, 3)), x1, x2, tau)
    assert not ok and not Eo.any()
    N, cnt = fm3d.epipolar_normal45(np.zeros((3, 3)), x1, x2, tau)
    assert cnt == 0 and not N.any() and not np.signbit(N).any()
    # a NaN coordinate is out and adds nothing: the sums are those with any other pair that is out
    y1 = x1.copy()
    y1[inl[3], 1] = math.nan
    z1, z2 = x1.copy(), x2.copy()
    z1[inl[3]], z2[inl[3]] = (0.9, -0.9), (-0.9, 0.9)
    assert not ref.inliers(E, z1, z2, tau)[inl[3]]
    Ny, cy = fm3d.epipolar_normal45(E, y1, x2, tau)
    Nz, cz = fm3d.epipolar_normal45(E, z1, z2, tau)
    assert cy == cz == len(inl) - 1 and np.isfinite(Ny).all() and Ny.tobytes() == Nz.tobytes()
    assert Ny.tobytes() == np.array(rr.normal45(E, y1, x2, tau)[0]).tobytes()
    # only NaN pairs left in: nothing is in
    assert not fm3d.epipolar_refit(E, np.full((16, 2), math.nan), x2[:16], tau)[1]
    # a model with a NaN entry accepts nothing
    En = np.array(E)
    En[1, 1] = math.nan
    assert not fm3d.epipolar_refit(En, x1, x2, tau)[1]


def test_non_finite_normal_matrix_is_invalid(fm3d, orc):
    """pairs so far out that their products overflow, under a model that accepts them: N is not finite"""
    E = np.array([[0.0, 0.0, 0.0], [0.0, 0.0, -1.0], [0.0, 1.0, 0.0]])  # y2 = y1
    x1 = np.array([[1e160 * (k + 1), 0.5] for k in range(9)])
    x2 = np.array([[-1e160 * (k + 2), 0.5] for k in range(9)])
    assert fm3d.epipolar_count(E, x1, x2, 1e-3)[0] == 9
    N, cnt = fm3d.epipolar_normal45(E, x1, x2, 1e-3)
    assert cnt == 9 and not np.isfinite(N).all()
    Eo, ok = fm3d.epipolar_refit(E, x1, x2, 1e-3)
    assert not ok and not Eo.any() and not rr.refit(orc, E, x1, x2, 1e-3)[1]


# ---------------------------------------------------------------- rounds (restatement)
def test_rounds_restatement_adopts_and_refuses(orc, case):
    """the two seeds tests/test_gpu_verify_refit.py runs on the GPU, 64 hypotheses at 1 px"""
    x1, x2, tau = case["x1"], case["x2"], case["tau"]
    a = rr.refined(orc, ref.ransac(orc, x1, x2, 64, tau, 0), x1, x2, tau, 3)
    assert list(a["roundCounts"]) == [1250, 1250, 1251, 1251] and a["adopted"] == 3
    assert int(a["mask"].sum()) == 1251
    ran = ref.ransac(orc, x1, x2, 64, tau, 1)
    b = rr.refined(orc, ran, x1, x2, tau, 3)
    assert list(b["roundCounts"]) == [1252, 1249, -2, -2] and b["adopted"] == 0
    assert np.array_equal(b["E"], ran["E"]) and b["roundModels"][0].any() and not b["roundModels"][1:].any()
    z = rr.refined(orc, ran, x1, x2, tau, 0)
    assert np.array_equal(z["E"], ran["E"]) and np.array_equal(z["mask"], ran["mask"]) and list(z["roundCounts"]) == [1252]


def test_quality_of_the_restatement(synth, orc):
    """The noisy case at M = 300 (sigma = 0.5 px, default_rng(100), 256 hypotheses, seeds 0..7, 1 and 2 px,
    three rounds): the final count is never below c_0 and the rotation error falls in at least 12 of the
    16 runs.  Measured: 16 of 16 (and 15 of 16 at M = 1800, which the GPU test runs)."""
    pair, kp1, kp2, m = rr.noisy_inputs(synth, 300)
    x1, x2 = ref.coords(orc, pair.cam, kp1, kp2, m)
    better = 0
    for px in (1.0, 2.0):
        tau = ref.tau_of(pair.cam, px)
        for seed in range(8):
            ran = ref.ransac(orc, x1, x2, 256, tau, seed)
            out = rr.refined(orc, ran, x1, x2, tau, 3)
            assert int(out["mask"].sum()) >= out["roundCounts"][0] == ran["counts"][ran["best"]]
            err = []
            for E in (ran["E"], out["E"]):
                mk = ref.inliers(E, x1, x2, tau)
                err.append(rr.rot_err_deg(ref.pose(orc, E, x1[mk], x2[mk])[0][:3, :3], pair.g12[:3, :3]))
            better += err[1] < err[0]
    print("better in", better, "of 16")
    assert better >= 12


# ---------------------------------------------------------------- interface
def test_exports_listed(fm3d):
    for n in ("fm3d_verify_matches_refined", "fm3d_epipolar_normal45", "fm3d_epipolar_refit"):
        assert n in fm3d.EXPORTS and hasattr(fm3d.lib(), n)
    assert callable(fm3d.epipolar_normal45) and callable(fm3d.epipolar_refit)


def test_null_pointers(fm3d):
    L = fm3d.lib()
    E = (ctypes.c_double * 9)()
    x = (ctypes.c_double * 32)()
    N = (ctypes.c_double * 45)()
    tau = ctypes.c_double(1e-3)
    assert L.fm3d_epipolar_normal45(None, x, x, 16, tau, N) == fm3d.ERR_INVALID
    assert L.fm3d_epipolar_normal45(E, None, x, 16, tau, N) == fm3d.ERR_INVALID
    assert L.fm3d_epipolar_normal45(E, x, None, 16, tau, N) == fm3d.ERR_INVALID
    assert L.fm3d_epipolar_normal45(E, x, x, 16, tau, None) == fm3d.ERR_INVALID
    assert L.fm3d_epipolar_normal45(E, x, x, -1, tau, N) == fm3d.ERR_INVALID
    assert L.fm3d_epipolar_normal45(E, None, None, 0, tau, N) == 0
    assert L.fm3d_epipolar_refit(None, x, x, 16, tau, E) == fm3d.ERR_INVALID
    assert L.fm3d_epipolar_refit(E, x, None, 16, tau, E) == fm3d.ERR_INVALID
    assert L.fm3d_epipolar_refit(E, x, x, 16, tau, None) == fm3d.ERR_INVALID
    assert L.fm3d_epipolar_refit(E, x, x, -1, tau, E) == fm3d.ERR_INVALID
    assert L.fm3d_epipolar_refit(E, None, None, 0, tau, E) == 1
    n, best = ctypes.c_int(0), ctypes.c_int(0)
    assert L.fm3d_verify_matches_refined(None, None, 0, None, 0, None, 0, 16, ctypes.c_double(1.0), ctypes.c_uint64(0), 1,
                                         E, None, None, ctypes.byref(n), ctypes.byref(best), None, None, None, None,
                                         None) == fm3d.ERR_INVALID


@pytest.mark.parametrize("bad", [-1, 17])
def test_python_mirror_rejects_bad_refine(fm3d, bad):
    """the Python mirror applies the C rule (refineIters in 0 .. 16) before any device work; the C entry
    point itself is checked on the GPU (tests/test_gpu_verify_refit.py)"""
    sct = fm3d.SingleCameraTriangulator(ctx=None)
    k = np.zeros((2, 2), dtype=np.float32)
    m = np.zeros(1, dtype=fm3d.DMATCH)
    with pytest.raises(fm3d.Fm3dError) as e:
        sct.verifyMatches(k, k, m, 1.0, refine=bad)
    assert e.value.code == fm3d.ERR_INVALID


CONSUMER = r"""
#include "fm3d_compat.hpp"
#include <vector>
using namespace fm3d::compat;
int use(SingleCameraTriangulator& sct, const std::vector<KeyPoint>& ka, const std::vector<KeyPoint>& kb,
        const std::vector<DMatch>& m) {
    std::vector<DMatch> in;
    std::array<double, 9> E;
    std::vector<bool> mask;
    int adopted = 0;
    int best = sct.verifyMatches(ka, kb, m, 1.0, 3, in, E);
    best += sct.verifyMatches(ka, kb, m, 1.0, 3, in, E, 4096, 7u, &mask, &adopted);
    best += sct.verifyMatches(ka, kb, m, 1.0, in, E);  // the unrefined overload still resolves
    double x1[16] = {0}, x2[16] = {0}, N[45], Eo[9];
    fm3d_epipolar_normal45(E.data(), x1, x2, 8, 1e-3, N);
    fm3d_epipolar_refit(E.data(), x1, x2, 8, 1e-3, Eo);
    return best + adopted;
}
int main() { return 0; }
"""


def test_shim_overload_compiles(tmp_path):
    p = tmp_path / "consumer.cpp"
    p.write_text(CONSUMER)
    r = subprocess.run(["g++", "-std=c++17", "-fsyntax-only", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"),
                        str(p)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
