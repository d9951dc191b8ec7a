"""2D-3D localisation, the host side: the quartic, the P3P solve, the count and the
Gauss-Newton step against the plain-Python restatement (tests/pnp_pyref.py), bit for bit; the
restatement's RANSAC end to end on the quality cases; the argument rules, the C++ shim and the
header's arithmetic under the sanitizers -- no GPU compute here."""
import ctypes
import math
import os
import subprocess

import numpy as np
import pytest

import pnp_pyref as ref
from conftest import ROOT

SEEDS = (0, 3, 7)
MAX_PX = 2.0


def same(a, b):
    return np.array_equal(np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64), equal_nan=True)


# ---------------------------------------------------------------- quartic
def check_quartic(fm3d, coef):
    """coef lowest first; -> (roots, n, valid) of the library, equal to the restatement's"""
    roots, n, ok = fm3d.quartic_roots(coef)
    nr, xr = ref.quartic_roots(coef[4], coef[3], coef[2], coef[1], coef[0])
    assert ok == (nr >= 0) and n == max(nr, 0) and same(roots, xr)
    return roots, n, ok


def residual(coef, x):
    return (((coef[4] * x + coef[3]) * x + coef[2]) * x + coef[1]) * x + coef[0]


def test_quartic_four_real_roots(fm3d):
    roots, n, ok = check_quartic(fm3d, [24.0, -50.0, 35.0, -10.0, 1.0])  # (x-1)(x-2)(x-3)(x-4)
    assert ok and n == 4 and np.abs(np.sort(roots) - [1, 2, 3, 4]).max() < 1e-12
    roots, n, ok = check_quartic(fm3d, [0.3 * 24.0, -0.3 * 50.0, 0.3 * 35.0, -3.0, 0.3])  # not monic
    assert ok and n == 4 and np.abs(np.sort(roots) - [1, 2, 3, 4]).max() < 1e-12


def test_quartic_two_real_roots(fm3d):
    roots, n, ok = check_quartic(fm3d, [2.0, -3.0, 3.0, -3.0, 1.0])  # (x^2 + 1)(x - 1)(x - 2)
    assert ok and n == 2 and np.abs(np.sort(roots[~np.isnan(roots)]) - [1, 2]).max() < 1e-12
    # the positions are fixed: the pair of one quadratic stays where it is, the other pair is NaN
    assert np.isnan(roots).sum() == 2 and (np.isnan(roots[:2]).all() or np.isnan(roots[2:]).all())


def test_quartic_no_real_root(fm3d):
    for coef in ([1.0, 0.0, 1.0, 0.0, 1.0], [5.0, 2.0, 4.0, 1.0, 1.0], [2.0, -2.0, 3.0, -2.0, 1.0]):
        roots, n, ok = check_quartic(fm3d, coef)
        assert ok and n == 0 and np.isnan(roots).all()


def test_quartic_biquadratic(fm3d):
    """q == 0 after the shift: z = y^2 by a quadratic, then -+sqrt(z) in positions (0, 1) and (2, 3)"""
    roots, n, ok = check_quartic(fm3d, [4.0, 0.0, -5.0, 0.0, 1.0])
    assert ok and n == 4 and list(roots) == [-1.0, 1.0, -2.0, 2.0]
    roots, n, ok = check_quartic(fm3d, [-4.0, 0.0, 3.0, 0.0, 1.0])  # z = -4, 1
    assert ok and n == 2 and np.isnan(roots[:2]).all() and list(roots[2:]) == [-1.0, 1.0]
    # shifted by one: a3 != 0 but the depressed q is exactly zero
    roots, n, ok = check_quartic(fm3d, [0.0, 6.0, 1.0, -4.0, 1.0])  # (x-1)^4 - 5 (x-1)^2 + 4
    assert ok and n == 4 and list(roots) == [0.0, 2.0, -1.0, 3.0]


def test_quartic_zero_leading_coefficient(fm3d):
    for c4 in (0.0, -0.0, 1e-320, math.nan):
        roots, n, ok = check_quartic(fm3d, [1.0, 2.0, 3.0, 4.0, c4])
        assert not ok and n == 0 and np.isnan(roots).all()
    for bad in (math.inf, math.nan):  # a monic coefficient that is not finite
        assert not check_quartic(fm3d, [1.0, bad, 3.0, 4.0, 1.0])[2]
        assert not check_quartic(fm3d, [1.0, 2.0, 3.0, 1e300, 1e-300])[2]


def test_quartic_double_root(fm3d):
    """(x - 1)^2 (x - 2)^2 and (x - 1)^2 (x^2 + 1): whatever the discriminant's rounding leaves, the same
    bits as the restatement, and every root reported is one"""
    for coef in ([4.0, -12.0, 13.0, -6.0, 1.0], [1.0, -2.0, 2.0, -2.0, 1.0], [0.0, 0.0, 0.0, 0.0, 1.0]):
        roots, n, ok = check_quartic(fm3d, coef)
        assert ok
        for x in roots[~np.isnan(roots)]:
            assert abs(residual(coef, x)) < 1e-9
    roots, n, _ = check_quartic(fm3d, [4.0, -12.0, 13.0, -6.0, 1.0])
    assert n == 4 and np.abs(np.sort(roots) - [1, 1, 2, 2]).max() < 1e-7


def test_quartic_random_bitwise(fm3d):
    rng = np.random.default_rng(5)
    seen = set()
    for _ in range(300):
        coef = rng.normal(size=5)
        roots, n, ok = check_quartic(fm3d, coef)
        seen.add(n)
        assert n == int((np.abs(np.roots(coef[::-1]).imag) < 1e-9).sum())
        for x in roots[~np.isnan(roots)]:  # a polished root: the residual is Horner's own rounding, <= 8 eps sum |c_k x^k|
            scale = sum(abs(coef[k]) * abs(x) ** k for k in range(5))
            assert abs(residual(coef, x)) <= 16 * 2.220446049250313e-16 * scale
    assert seen == {0, 2, 4}
    L = fm3d.lib()
    buf, out = (ctypes.c_double * 5)(), (ctypes.c_double * 4)()
    assert L.fm3d_quartic_roots(None, out, None) == fm3d.ERR_INVALID
    assert L.fm3d_quartic_roots(buf, None, None) == fm3d.ERR_INVALID


# ---------------------------------------------------------------- P3P
def random_pose(rng):
    return ref.rodrigues(rng.normal(size=3), rng.uniform(0.05, 0.6)), rng.uniform(-0.3, 0.3, 3)


def random_sample(rng, planar=False):
    """three points in front of a camera at a random pose -> (X, uv, model)"""
    R, t = random_pose(rng)
    Xc = np.stack([rng.uniform(-0.8, 0.8, 3), rng.uniform(-0.6, 0.6, 3),
                   np.full(3, 2.0) if planar else rng.uniform(1.6, 2.3, 3)], axis=1)
    X = (Xc - t) @ R
    Xc = X @ R.T + t
    return X, Xc[:, :2] / Xc[:, 2:3], np.concatenate([R.ravel(), t])


def check_p3p(fm3d, orc, X, uv):
    m, ok = fm3d.p3p(X, uv)
    mr, okr = ref.p3p(orc, X, uv)
    assert list(ok) == list(okr) and np.array_equal(m, mr)
    for k in range(4):
        assert ok[k] or not m[k].any()
    return m, ok


def conditioning(X, uv, truth):
    """The first-order bound on what rounding does to the pose of a noise-free sample: eps kv ku with
    kv = sum |A_k| v^k / (v |A'(v)|), the condition of the quartic's root v = s2 / s0 (|A_k|: the
    coefficients built from the polynomials' absolute values, what the products' rounding acts on), and
    ku = (|D0| + |D1| v) / |D(v)| + sum |N_k| v^k / |N(v)|, the condition of u = N(v) / D(v).  Two
    solutions close in v (kv large) or D(v) near zero (ku large) are the elimination's weak spots."""
    R, t = truth[:9].reshape(3, 3), truth[9:]
    s = np.linalg.norm(X @ R.T + t, axis=1)
    v = s[2] / s[0]
    j = [ref.bearing(*p) for p in uv.tolist()]
    ca, cb, cg = ref._dot(j[1], j[2]), ref._dot(j[0], j[2]), ref._dot(j[0], j[1])
    a2, b2, c2 = ref._dist2(X[1], X[2]), ref._dist2(X[0], X[2]), ref._dist2(X[0], X[1])
    k, q1 = a2 - c2, -2.0 * cb
    N, D, W = np.array([b2 + k, k * q1, k - b2]), np.array([2.0 * b2 * cg, -(2.0 * b2 * ca)]), np.array([b2 - c2, -(c2 * q1), -c2])
    P = np.polynomial.polynomial
    A = b2 * P.polymul(N, N)
    A[:4] -= D[0] * P.polymul(N, D)
    A += P.polymul(W, P.polymul(D, D))
    Am = b2 * P.polymul(abs(N), abs(N))
    Am[:4] += abs(D[0]) * P.polymul(abs(N), abs(D))
    Am += P.polymul(abs(W), P.polymul(abs(D), abs(D)))
    kv = P.polyval(v, Am) / (v * abs(P.polyval(v, P.polyder(A))))
    ku = (abs(D[0]) + abs(D[1]) * v) / abs(D[0] + D[1] * v) + P.polyval(v, abs(N)) / abs(P.polyval(v, N))
    return 2.220446049250313e-16 * kv * ku


def test_p3p_noise_free_sample(fm3d, orc):
    """a slot holds the pose that made the sample, general triangles and fronto-parallel ones: within
    1e-8 wherever the sample's conditioning (above) allows that, and within the conditioning's bound
    everywhere; every valid slot is a rotation that reprojects the three points"""
    rng = np.random.default_rng(12)
    nslots, tight = [], 0
    for i in range(120):
        X, uv, truth = random_sample(rng, planar=i % 3 == 0)
        m, ok = check_p3p(fm3d, orc, X, uv)
        assert ok.any()
        err, bound = min(np.abs(m[k] - truth).max() for k in range(4) if ok[k]), conditioning(X, uv, truth)
        assert err <= bound
        if bound < 1e-8:
            tight += 1
            assert err < 1e-8
        for k in np.nonzero(ok)[0]:
            R, t = m[k][:9].reshape(3, 3), m[k][9:]
            assert abs(np.linalg.det(R) - 1) < 1e-9
            Xc = X @ R.T + t
            assert (Xc[:, 2] > 0).all() and np.abs(Xc[:, :2] / Xc[:, 2:3] - uv).max() < 1e-3  # (under half a pixel)
        nslots.append(int(ok.sum()))
    assert set(nslots) >= {2, 4} and max(nslots) == 4 and tight >= 40


def test_p3p_slots_do_not_move(fm3d, orc):
    """slot k is root position k: an invalid slot is a zero model where it stands, also in front of a
    valid one, and the valid slots sit where the quartic's roots do"""
    rng = np.random.default_rng(3)
    gaps = 0
    for _ in range(200):
        X, uv, _ = random_sample(rng)
        m, ok = check_p3p(fm3d, orc, X, uv)
        first = int(np.argmax(ok))
        gaps += first > 0 or not ok[first:int(ok.sum()) + first].all()
    assert gaps >= 20


def test_p3p_collinear_and_coincident(fm3d, orc):
    X, uv, _ = random_sample(np.random.default_rng(1))
    line = np.array([[0.0, 0.0, 1.0], [1.0, 2.0, 3.0], [2.0, 4.0, 5.0]])
    m, ok = check_p3p(fm3d, orc, line, uv)
    assert not ok.any() and not m.any()
    rng = np.random.default_rng(4)
    for _ in range(20):  # a general line, with its own (consistent) image points: the restatement's verdict
        R, t = random_pose(rng)
        p, d = rng.uniform(-0.5, 0.5, 3) + [0, 0, 2.0], rng.uniform(-1, 1, 3)
        L3 = np.stack([p, p + 0.37 * d, p - 0.21 * d])
        Xc = L3 @ R.T + t
        check_p3p(fm3d, orc, L3, Xc[:, :2] / Xc[:, 2:3])
    for a, b in ((0, 1), (0, 2), (1, 2)):  # duplicate matches: a zero side
        Y = X.copy()
        Y[b] = Y[a]
        m, ok = check_p3p(fm3d, orc, Y, uv)
        assert not ok.any() and not m.any()
    same3 = np.repeat(X[:1], 3, axis=0)
    assert not check_p3p(fm3d, orc, same3, uv)[1].any()
    # three different points seen in one direction: bearings coincide
    check_p3p(fm3d, orc, X, np.repeat(uv[:1], 3, axis=0))


def test_p3p_nan_and_inf(fm3d, orc):
    X, uv, _ = random_sample(np.random.default_rng(2))
    for bad in (math.nan, math.inf, -math.inf):
        for r in range(3):
            for c in range(5):
                Y, w = X.copy(), uv.copy()
                if c < 3:
                    Y[r, c] = bad
                else:
                    w[r, c - 3] = bad
                m, ok = check_p3p(fm3d, orc, Y, w)
                assert np.isfinite(m).all()
                if c < 3 or bad != bad:
                    assert not ok.any() and not m.any()
    L = fm3d.lib()
    b9, b6, out = (ctypes.c_double * 9)(), (ctypes.c_double * 6)(), (ctypes.c_double * 48)()
    assert L.fm3d_p3p(None, b6, out, None) == fm3d.ERR_INVALID
    assert L.fm3d_p3p(b9, None, out, None) == fm3d.ERR_INVALID
    assert L.fm3d_p3p(b9, b6, None, None) == fm3d.ERR_INVALID
    assert L.fm3d_p3p(b9, b6, out, None) == 0


# ---------------------------------------------------------------- count
IDENTITY = np.array([1.0, 0, 0, 0, 1, 0, 0, 0, 1, 0, 0, 0])


def threshold_matches():
    """under the identity, tau = 2^-8: X = (0.5, 0.25, 2) projects to (0.25, 0.125); u = 0.25 - 2^-8 gives
    x - u z = 2^-7 exactly, so (x - u z)^2 == tau^2 z^2 == 2^-14: at the threshold, and one ulp of u either
    side of it lies inside and outside"""
    tau = 2.0 ** -8
    u = 0.25 - tau
    uv = np.array([[u, 0.125], [np.nextafter(u, 1.0), 0.125], [np.nextafter(u, -1.0), 0.125]])
    return uv, np.repeat([[0.5, 0.25, 2.0]], 3, axis=0), tau


def test_match_exactly_at_the_threshold(fm3d):
    uv, X, tau = threshold_matches()
    assert (0.5 - uv[0, 0] * 2.0) ** 2 == tau * tau * 4.0
    n, mask = fm3d.pnp_count(IDENTITY, uv, X, tau)
    assert n == 2 and list(mask) == [True, True, False] and list(ref.inliers(IDENTITY, uv, X, tau)) == [True, True, False]


def test_behind_the_camera_is_rejected(fm3d):
    uv = np.array([[0.25, 0.125]] * 4)
    X = np.array([[0.5, 0.25, 2.0], [-0.5, -0.25, -2.0], [0.0, 0.0, 0.0], [0.5, 0.25, -2.0]])
    n, mask = fm3d.pnp_count(IDENTITY, uv, X, 10.0)
    assert list(mask) == [True, False, False, False] and n == 1
    assert list(ref.inliers(IDENTITY, uv, X, 10.0)) == [True, False, False, False]
    for k in range(5):  # a NaN anywhere fails
        u2, X2 = uv.copy(), X.copy()
        if k < 2:
            u2[0, k] = math.nan
        else:
            X2[0, k - 2] = math.nan
        assert not fm3d.pnp_count(IDENTITY, u2, X2, 10.0)[1][0]


def test_count_equals_restatement(fm3d, orc):
    p, r = ref.quality_case(orc, 0)
    uv, X, tau = r["uv"], r["X"], r["tau"]
    nrm = p["n"][p["matches"]["trainIdx"]]
    valid = np.nonzero(r["counts"] >= 0)[0]
    for h in (valid[0], valid[1], r["best"]):
        m = r["models"][h]
        n, mask = fm3d.pnp_count(m, uv, X, tau)
        want = ref.inliers(m, uv, X, tau)
        assert n == int(want.sum()) == r["counts"][h] and np.array_equal(mask, want)
        for mc in (0.0, 0.5, 0.97, 1.0):
            n, mask = fm3d.pnp_count(m, uv, X, tau, nrm, mc)
            want = ref.inliers(m, uv, X, tau, nrm, mc)
            assert n == int(want.sum()) and np.array_equal(mask, want)
    # the normals are a second test: the scene's normals lie along the viewing rays (cosine 1), so every
    # match the best model keeps also faces the camera; turned round, none does
    n0, m0 = fm3d.pnp_count(r["model"], uv, X, tau)
    n1, m1 = fm3d.pnp_count(r["model"], uv, X, tau, nrm, 0.99)
    n2, _ = fm3d.pnp_count(r["model"], uv, X, tau, -nrm, 0.0)
    assert n0 == n1 > 400 and np.array_equal(m0, m1) and n2 == 0
    z = nrm.copy()
    z[np.nonzero(m0)[0][0], 1] = math.nan
    assert fm3d.pnp_count(r["model"], uv, X, tau, z, 0.0)[0] == n0 - 1
    L = fm3d.lib()
    one = ctypes.c_double(1.0)
    buf = (ctypes.c_double * 12)()
    assert L.fm3d_pnp_count(None, buf, buf, None, 1, one, one, None) == fm3d.ERR_INVALID
    assert L.fm3d_pnp_count(buf, None, buf, None, 1, one, one, None) == fm3d.ERR_INVALID
    assert L.fm3d_pnp_count(buf, buf, None, None, 1, one, one, None) == fm3d.ERR_INVALID
    assert L.fm3d_pnp_count(buf, buf, buf, None, -1, one, one, None) == fm3d.ERR_INVALID
    assert L.fm3d_pnp_count(buf, None, None, None, 0, one, one, None) == 0


# ---------------------------------------------------------------- step
def step_inputs(n, seed=31):
    """n matches around a known pose with 0.5 px of noise at f = 520, a third of them far off (so the
    predicate matters), and a model slightly off"""
    rng = np.random.default_rng(seed)
    R, t = ref.rodrigues([0.2, 0.9, -0.4], 0.2), np.array([0.05, -0.1, 0.2])
    Xc = np.stack([rng.uniform(-0.8, 0.8, n), rng.uniform(-0.6, 0.6, n), rng.uniform(1.6, 2.3, n)], axis=1)
    X = (Xc - t) @ R
    uv = Xc[:, :2] / Xc[:, 2:3] + rng.normal(0, 0.5 / 520.0, (n, 2))
    off = rng.random(n) < 0.33
    uv[off] += rng.uniform(0.02, 0.2, (int(off.sum()), 2))
    m0 = np.concatenate([(ref.rodrigues([1.0, -1.0, 0.5], 0.002) @ R).ravel(), t + 0.002])
    return uv, X, m0, np.concatenate([R.ravel(), t]), 4.0 / 520.0


@pytest.mark.parametrize("n", [1023, 1024, 1025, 2049])
def test_step_sums_pin_the_tile_order(fm3d, n):
    uv, X, m0, truth, tau = step_inputs(n)
    m, ok, S = fm3d.pnp_step(m0, uv, X, tau, sums=True)
    mr, okr, Sr = ref.step(m0, uv, X, tau)
    assert ok and okr and np.array_equal(S, Sr) and np.array_equal(m, mr)
    inl = ref.inliers(m0, uv, X, tau)
    assert S[27] == int(inl.sum()) and 0.4 * n < S[27] < 0.8 * n
    # the sums are J^T J and J^T r of the restated Jacobian: compared with numpy's own products
    J, r = numeric_jacobian(m0, uv[inl], X[inl])
    JtJ, Jtr = J.T @ J, J.T @ r
    assert np.allclose([JtJ[i, k] for i, k in ref.PAIRS], S[:21], rtol=1e-9)
    assert np.allclose(Jtr, S[21:27], rtol=1e-7, atol=1e-9)
    # the order is part of the contract: adding the same terms one after the other gives other bits
    mm = [float(v) for v in m0]
    plain = 0.0
    for row in X[inl].tolist():  # entry (3, 3) of J^T J: a a + 0 0 with a = 1 / z
        a = 1.0 / (ref._rot_row(mm, 2, row[0], row[1], row[2]) + mm[11])
        plain = plain + (a * a + 0.0 * 0.0)
    assert plain != S[ref.PAIRS.index((3, 3))] and math.isclose(plain, S[ref.PAIRS.index((3, 3))], rel_tol=1e-12)
    # and the step moves the model towards the pose that made the data
    assert abs(np.linalg.det(m[:9].reshape(3, 3)) - 1) < 1e-12
    assert np.abs(m - truth).max() < np.abs(m0 - truth).max()


def numeric_jacobian(m, uv, X, h=1e-6):
    """central differences of the residual over (omega, delta t) at zero, rows (r0, r1) per match"""
    R, t = m[:9].reshape(3, 3), m[9:]

    def res(d):
        P = X @ R.T
        Xc = P + np.cross(d[:3], P) + t + d[3:]
        return (Xc[:, :2] / Xc[:, 2:3] - uv).ravel()

    J = np.stack([(res(h * e) - res(-h * e)) / (2 * h) for e in np.eye(6)], axis=1)
    return J, res(np.zeros(6))


def test_step_with_normals_and_invalid(fm3d):
    uv, X, m0, truth, tau = step_inputs(1500)
    Xc = X @ m0[:9].reshape(3, 3).T + m0[9:]
    nrm = (Xc / np.linalg.norm(Xc, axis=1)[:, None]) @ m0[:9].reshape(3, 3)
    nrm[::5] = -nrm[::5]  # every fifth match faces the other way
    m, ok, S = fm3d.pnp_step(m0, uv, X, tau, nrm, 0.5, sums=True)
    mr, okr, Sr = ref.step(m0, uv, X, tau, nrm, 0.5)
    assert ok and okr and np.array_equal(S, Sr) and np.array_equal(m, mr)
    assert S[27] < fm3d.pnp_step(m0, uv, X, tau, sums=True)[2][27]
    # fewer than three matches in: invalid, a zero model
    for keep in (0, 2):
        far = uv + 10.0
        far[:keep] = uv[:keep]
        m, ok, S = fm3d.pnp_step(m0, far, X, tau, sums=True)
        mr, okr, Sr = ref.step(m0, far, X, tau)
        assert not ok and not okr and not m.any() and S[27] <= keep and np.array_equal(S, Sr, equal_nan=True)
    # three matches: the 6 x 6 system has rank 6 at most by a hair; four on one ray: a pivot that is not > 0
    ray = np.repeat(X[:1], 4, axis=0) * np.array([[1.0], [1.5], [2.0], [2.5]])
    R, t = truth[:9].reshape(3, 3), truth[9:]
    model0 = np.concatenate([R.ravel(), np.zeros(3)])
    Xr = ray @ R.T
    m, ok, S = fm3d.pnp_step(model0, Xr[:, :2] / Xr[:, 2:3], ray, tau, sums=True)
    mr, okr, Sr = ref.step(model0, Xr[:, :2] / Xr[:, 2:3], ray, tau)
    assert S[27] == 4 and ok == okr and np.array_equal(m, mr) and np.array_equal(S, Sr)
    # a NaN match is out of every sum
    y = X.copy()
    y[7] = math.nan
    m, ok, S = fm3d.pnp_step(m0, uv, y, tau, sums=True)
    mr, okr, Sr = ref.step(m0, uv, y, tau)
    assert ok and np.isfinite(S).all() and np.array_equal(S, Sr) and np.array_equal(m, mr)
    # a model of NaN accepts nothing
    m, ok, S = fm3d.pnp_step(np.full(12, math.nan), uv, X, tau, sums=True)
    assert not ok and not m.any() and S[27] == 0
    L = fm3d.lib()
    one = ctypes.c_double(1.0)
    buf = (ctypes.c_double * 12)()
    assert L.fm3d_pnp_step(None, buf, buf, None, 1, one, one, buf, None) == fm3d.ERR_INVALID
    assert L.fm3d_pnp_step(buf, buf, buf, None, 1, one, one, None, None) == fm3d.ERR_INVALID
    assert L.fm3d_pnp_step(buf, None, buf, None, 1, one, one, buf, None) == fm3d.ERR_INVALID
    assert L.fm3d_pnp_step(buf, buf, buf, None, -1, one, one, buf, None) == fm3d.ERR_INVALID


# ---------------------------------------------------------------- RANSAC end to end (restatement)
# What the restatement alone is off on the quality cases, computed on the CPU by tests/pnp_pyref.py
# (DESIGN.md §3.1f), relief and planar: the best P3P model per seed, and the model after four rounds of
# the step (the same for the three seeds: they end on the same 424 matches).  The library is held to
# twice these.
ROT_ERR_DEG = {(True, 0): 0.1894, (True, 3): 0.1058, (True, 7): 0.1209,
               (False, 0): 0.1481, (False, 3): 0.1752, (False, 7): 0.2448}
ROT_ERR_REFINED_DEG = {True: 0.0179, False: 0.0058}


@pytest.mark.parametrize("relief", [True, False])
@pytest.mark.parametrize("seed", SEEDS)
def test_restatement_meets_the_caps(orc, seed, relief):
    """600 matches, 30 % of them wrong, 0.5 px noise, maxPx 2, 256 samples, depth 1.6 - 2.3 m or an exact
    plane: >= 99 % of the true matches kept, <= 1 % of the wrong ones, and four rounds of the step do not
    raise the rotation error"""
    p, r = ref.quality_case(orc, seed, relief)
    _, r4 = ref.quality_case(orc, seed, relief, refine=4)
    true = p["true"]
    assert len(true) == 600 and 150 <= int((~true).sum()) <= 210
    for name, run in (("unrefined", r), ("refine=4", r4)):
        kt, kw = int((run["mask"] & true).sum()), int((run["mask"] & ~true).sum())
        print(name, "relief" if relief else "planar", "seed", seed, ": kept", kt, "of", int(true.sum()), "true matches and",
              kw, "of", int((~true).sum()), "wrong")
        assert kt >= 0.99 * true.sum() and kw <= 0.01 * (~true).sum()
    e0, e4 = ref.rot_err_deg(r["g"][:3, :3], p["R"]), ref.rot_err_deg(r4["g"][:3, :3], p["R"])
    print("rotation error %.4f deg, refined %.4f deg; t error %.2e m, refined %.2e m; rounds %s" %
          (e0, e4, np.linalg.norm(r["g"][:3, 3] - p["t"]), np.linalg.norm(r4["g"][:3, 3] - p["t"]), r4["roundCounts"]))
    assert e4 <= e0
    assert abs(e0 - ROT_ERR_DEG[relief, seed]) < 1e-4 and abs(e4 - ROT_ERR_REFINED_DEG[relief]) < 1e-4
    assert r["best"] >= 0 and r["counts"][r["best"]] == r["counts"].max() == int(r["mask"].sum())
    assert r["best"] == int(np.nonzero(r["counts"] == r["counts"].max())[0][0])
    assert r4["adopted"] >= 1 and (np.diff(r4["roundCounts"][:1 + r4["adopted"]]) >= 0).all()


@pytest.mark.parametrize("relief", [True, False])
@pytest.mark.parametrize("seed", SEEDS)
def test_host_chain_equals_restatement_and_meets_the_bounds(fm3d, orc, seed, relief):
    """the same RANSAC and rounds driven through the host functions: every sample's four models and
    counts, the best model and each round, bit for bit; the pose within twice the restatement's error"""
    p, r = ref.quality_case(orc, seed, relief)
    _, r4 = ref.quality_case(orc, seed, relief, refine=4)
    uv, X, tau = r["uv"], r["X"], r["tau"]
    H = len(r["counts"])
    counts = np.full(H, -1, dtype=np.int32)
    models = np.zeros((H, 12))
    for h in range(H // 4):
        idx, ok = fm3d.ransac_sample3(seed, h, len(X))
        if not ok:
            continue
        ms, oks = fm3d.p3p(X[idx], uv[idx])
        for k in range(4):
            if oks[k]:
                models[4 * h + k] = ms[k]
                counts[4 * h + k] = fm3d.pnp_count(ms[k], uv, X, tau)[0]
    assert np.array_equal(counts, r["counts"]) and np.array_equal(models, r["models"])
    m, cur = models[r["best"]].copy(), int(counts[r["best"]])
    assert ref.rot_err_deg(m[:9].reshape(3, 3), p["R"]) <= 2 * ROT_ERR_DEG[relief, seed]
    for k in range(4):
        mc, ok = fm3d.pnp_step(m, uv, X, tau)
        cc = fm3d.pnp_count(mc, uv, X, tau)[0] if ok else -1
        assert np.array_equal(mc, r4["roundModels"][k]) and cc == r4["roundCounts"][1 + k]
        if not (ok and cc >= cur):
            break
        m, cur = mc, cc
    assert np.array_equal(m, r4["model"])
    assert ref.rot_err_deg(m[:9].reshape(3, 3), p["R"]) <= 2 * ROT_ERR_REFINED_DEG[relief]


def test_restatement_other_sizes(orc):
    """the recipe at N = 64 / 64 samples, and with 1 cm of relief at 2 m: the same picture"""
    p = ref.scene(N=64)
    r = ref.localize(orc, p["cam"], p["X"], p["kpts"], p["matches"], MAX_PX, 64, 0)
    true = p["true"]
    assert int((r["mask"] & true).sum()) >= 0.99 * true.sum() and int((r["mask"] & ~true).sum()) == 0
    p = ref.scene(relief=0.01)  # (where a six-point DLT's best model kept a chance-level 17 matches)
    true = p["true"]
    for seed in SEEDS:
        r = ref.localize(orc, p["cam"], p["X"], p["kpts"], p["matches"], MAX_PX, 256, seed, refine=4)
        assert int((r["mask"] & true).sum()) >= 0.99 * true.sum() and int((r["mask"] & ~true).sum()) == 0
        assert ref.rot_err_deg(r["g"][:3, :3], p["R"]) < 0.05


# ---------------------------------------------------------------- interface
def test_exports_listed(fm3d):
    names = ("fm3d_localize_points", "fm3d_localize_model", "fm3d_quartic_roots", "fm3d_p3p", "fm3d_pnp_count",
             "fm3d_pnp_step")
    for n in names:
        assert n in fm3d.EXPORTS and hasattr(fm3d.lib(), n)
    assert ctypes.sizeof(fm3d.LocalizeOpts) == 32
    assert [fm3d.LocalizeOpts.samples.offset, fm3d.LocalizeOpts.refineIters.offset, fm3d.LocalizeOpts.maxPx.offset,
            fm3d.LocalizeOpts.minFacingCos.offset, fm3d.LocalizeOpts.seed.offset] == [0, 4, 8, 16, 24]


def test_opts_layout_matches_the_header(tmp_path):
    src = ('#include <stdio.h>\n#include <stddef.h>\n#include "fm3d.h"\nint main(void){printf("%zu %zu %zu %zu %zu %zu\\n",'
           "sizeof(fm3d_localize_opts), offsetof(fm3d_localize_opts, samples), offsetof(fm3d_localize_opts, refineIters),"
           "offsetof(fm3d_localize_opts, maxPx), offsetof(fm3d_localize_opts, minFacingCos),"
           "offsetof(fm3d_localize_opts, seed));return 0;}")
    c, exe = tmp_path / "o.c", tmp_path / "o"
    c.write_text(src)
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), str(c), "-o", str(exe)], check=True)
    out = subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()
    assert [int(v) for v in out] == [32, 0, 4, 8, 16, 24]


def test_localize_null_context(fm3d):
    L = fm3d.lib()
    n, best = ctypes.c_int(0), ctypes.c_int(0)
    g = (ctypes.c_double * 16)()
    o = fm3d.LocalizeOpts(16, 0, 1.0, 0.0, 0)
    assert L.fm3d_localize_points(None, None, None, 0, None, 0, None, 0, ctypes.byref(o), g, None, None, ctypes.byref(n),
                                  ctypes.byref(best), None, None, None, None, None) == fm3d.ERR_INVALID
    assert L.fm3d_localize_model(None, None, None, 0, None, None, None, 0, 128, 1, ctypes.c_double(0.8), ctypes.byref(o),
                                 None, ctypes.byref(n), g, None, None, ctypes.byref(n), ctypes.byref(best), None, None,
                                 None, None, None) == fm3d.ERR_INVALID


@pytest.mark.parametrize("kw", [dict(max_px=0.0), dict(max_px=-1.0), dict(max_px=math.nan), dict(max_px=math.inf),
                                dict(samples=0), dict(samples=-3), dict(refine=-1), dict(refine=17),
                                dict(min_facing_cos=1.5), dict(min_facing_cos=-0.01), dict(min_facing_cos=math.nan)])
def test_python_mirror_rejects_bad_options(fm3d, kw):
    """the Python mirror applies the C rules before any device work (the C entry point itself is
    checked on the GPU, tests/test_gpu_pnp.py)"""
    loc = fm3d.ModelLocalizer(ctx=None)
    pts, kp = np.zeros((4, 3)), np.zeros((4, 2), dtype=np.float32)
    m = np.zeros(3, dtype=fm3d.DMATCH)
    args = dict(max_px=1.0)
    args.update(kw)
    with pytest.raises(fm3d.Fm3dError) as e:
        loc.localize(pts, kp, m, **args)
    assert e.value.code == fm3d.ERR_INVALID
    d = np.zeros((4, 128), dtype=np.uint8)
    with pytest.raises(fm3d.Fm3dError) as e:
        loc.match_and_localize(d, kp, d, pts, 0.8, **args)
    assert e.value.code == fm3d.ERR_INVALID


CONSUMER = r"""
#include "fm3d_compat.hpp"
#include <vector>
using namespace fm3d::compat;
Matx44d use(Device& d, const std::vector<Vec3d>& X, const std::vector<KeyPoint>& kp, const std::vector<DMatch>& m) {
    std::vector<DMatch> in;
    Matx44d g = localizeImage(d, X, kp, m, 2.0);
    g = localizeImage(d, X, kp, m, 2.0, &in, 1024, 7u, 4, &X, 0.5);
    double c[5] = {0}, r[4], pX[9] = {0}, uv[6] = {0}, models[48], model[12] = {0}, sums[28];
    int n;
    int32_t ok[4];
    fm3d_quartic_roots(c, r, &n);
    fm3d_p3p(pX, uv, models, ok);
    fm3d_pnp_count(model, uv, pX, nullptr, 3, 1e-3, 0.0, nullptr);
    fm3d_pnp_step(model, uv, pX, nullptr, 3, 1e-3, 0.0, model, sums);
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


def test_header_arithmetic_under_asan_ubsan(tmp_path):
    """tests/native/pnp_main.cpp: include/fm3d_pnp.h over its edge cases as a stand-alone host program
    built with the sanitizers and run directly; any report fails the run"""
    exe = tmp_path / "pnp_main"
    r = subprocess.run(["g++", "-std=c++17", "-ffp-contract=off", "-I", os.path.join(ROOT, "include"),
                        "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer", "-g", "-O1",
                        os.path.join(ROOT, "tests", "native", "pnp_main.cpp"), "-o", str(exe)], capture_output=True,
                       text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    env = dict(os.environ)
    env["UBSAN_OPTIONS"] = "print_stacktrace=1:halt_on_error=1"
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300, env=env)
    assert r.returncode == 0 and "pnp_main: ok" in r.stdout, r.stdout[-2000:] + r.stderr[-4000:]
    assert "ERROR: AddressSanitizer" not in r.stderr and "runtime error" not in r.stderr
