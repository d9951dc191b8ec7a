"""The 2D-3D localisation's contract restated in plain Python and numpy, in the order
include/fm3d_pnp.h writes it: Python floats are IEEE doubles and nothing here contracts a multiply and
an add, so the library (host and device) has to give the same bits.  The sampler, the three-point rigid
solve (with the oracle's restatement of OpenCV 2.4's JacobiSVD) and the tile tree are align_pyref's,
the undistortion the oracle's.  The sums are additions of Python floats or element-by-element
additions of equally long numpy arrays -- never a numpy reduction, whose order is not the contract's.
A division or a square root goes through numpy's scalars, which give IEEE's inf and NaN where Python's
own raise."""
import dataclasses
import math

import numpy as np

import align_pyref as aref

DBL_MIN = 2.2250738585072014e-308
NAN = math.nan
BISECT = 64
DMATCH = aref.DMATCH
sample3 = aref.sample3
rot_err_deg = aref.rot_err_deg
rodrigues = aref.rodrigues
g_of = aref.g_of


def _div(a, b):
    with np.errstate(all="ignore"):
        return float(np.float64(a) / np.float64(b))


def _sqrt(a):
    with np.errstate(all="ignore"):
        return float(np.sqrt(np.float64(a)))


def _finite(v):
    return abs(v) <= 1.7976931348623157e308


# ---------------------------------------------------------------- the quartic
def quadratic(b, c):
    disc = b * b - 4.0 * c
    if disc >= 0.0:
        s = _sqrt(disc)
        return _div(-b - s, 2.0), _div(-b + s, 2.0)
    return NAN, NAN


def newton(x, a3, a2, a1, a0):
    f = (((x + a3) * x + a2) * x + a1) * x + a0
    d = ((4.0 * x + 3.0 * a3) * x + 2.0 * a2) * x + a1
    xn = x - _div(f, d)
    return xn if _finite(xn) else x


def quartic_roots(c4, c3, c2, c1q, c0q):
    """-> (n, [x0, x1, x2, x3]): the real roots in their four positions (NaN where none), n = -1 for an
    invalid polynomial"""
    c4, c3, c2, c1q, c0q = float(c4), float(c3), float(c2), float(c1q), float(c0q)
    x = [NAN] * 4
    if not abs(c4) > DBL_MIN:
        return -1, x
    a3, a2, a1, a0 = _div(c3, c4), _div(c2, c4), _div(c1q, c4), _div(c0q, c4)
    if not (_finite(a3) and _finite(a2) and _finite(a1) and _finite(a0)):
        return -1, x
    e = a3 / 4.0
    e2 = e * e
    p = a2 - 6.0 * e2
    q = (a1 - 2.0 * a2 * e) + 8.0 * (e2 * e)
    r = ((a0 - a1 * e) + a2 * e2) - 3.0 * (e2 * e2)
    y = [NAN] * 4
    if q == 0.0:
        z0, z1 = quadratic(p, r)
        if z0 >= 0.0:
            s = _sqrt(z0)
            y[0], y[1] = -s, s
        if z1 >= 0.0:
            s = _sqrt(z1)
            y[2], y[3] = -s, s
    else:
        c1, c0 = (p * p) / 4.0 - r, (q * q) / 8.0
        big = abs(p)
        big = abs(c1) if abs(c1) > big else big
        big = c0 if c0 > big else big
        lo, hi = 0.0, 1.0 + big
        for _ in range(BISECT):
            mid = (lo + hi) / 2.0
            f = ((mid + p) * mid + c1) * mid - c0
            if f < 0.0:
                lo = mid
            else:
                hi = mid
        m = (lo + hi) / 2.0
        if m > 0.0 and _finite(m):
            s = _sqrt(2.0 * m)
            t = _div(q, 2.0 * s)
            w = p / 2.0 + m
            y[0], y[1] = quadratic(-s, w + t)
            y[2], y[3] = quadratic(s, w - t)
    x = [newton(newton(v - e, a3, a2, a1, a0), a3, a2, a1, a0) for v in y]
    return sum(1 for v in x if v == v), x


# ---------------------------------------------------------------- P3P
def _dot(a, b):
    return (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2]


def _dist2(a, b):
    d0, d1, d2 = a[0] - b[0], a[1] - b[1], a[2] - b[2]
    return (d0 * d0 + d1 * d1) + d2 * d2


def bearing(u, v):
    n = _sqrt((u * u + v * v) + 1.0)
    return [_div(u, n), _div(v, n), _div(1.0, n)]


def _slot(orc, v, X, j, b2, q1, N0, N1, N2, D0, D1):
    ok = v > 0.0
    Dv = D0 + D1 * v
    Nv = (N2 * v + N1) * v + N0
    ok = ok and Dv != 0.0
    u = _div(Nv, Dv)
    ok = ok and u > 0.0
    qv = (v * v + q1 * v) + 1.0
    s0 = _sqrt(_div(b2, qv))
    s1, s2 = u * s0, v * s0
    ok = ok and _finite(s0) and _finite(s1) and _finite(s2)
    if not ok:
        return np.zeros(12), False
    C = [[s * j[i][r] for r in range(3)] for i, s in enumerate((s0, s1, s2))]
    return aref.from3(orc, X, C)


def p3p(orc, X, uv):
    """-> (models (4, 12), ok [4]): slot k belongs to root position k; zero when invalid"""
    X = [[float(v) for v in p] for p in np.asarray(X, dtype=np.float64).reshape(3, 3)]
    uv = [[float(v) for v in p] for p in np.asarray(uv, dtype=np.float64).reshape(3, 2)]
    j = [bearing(p[0], p[1]) for p in uv]
    ca, cb, cg = _dot(j[1], j[2]), _dot(j[0], j[2]), _dot(j[0], j[1])
    a2, b2, c2 = _dist2(X[1], X[2]), _dist2(X[0], X[2]), _dist2(X[0], X[1])
    v = [NAN] * 4
    k, q1 = a2 - c2, -2.0 * cb
    N0, N1, N2 = b2 + k, k * q1, k - b2
    D0, D1 = 2.0 * b2 * cg, -(2.0 * b2 * ca)
    if a2 > 0.0 and b2 > 0.0 and c2 > 0.0:
        W0, W1, W2 = b2 - c2, -(c2 * q1), -c2
        NN = [N0 * N0, 2.0 * (N0 * N1), 2.0 * (N0 * N2) + N1 * N1, 2.0 * (N1 * N2), N2 * N2]
        ND = [N0 * D0, N0 * D1 + N1 * D0, N1 * D1 + N2 * D0, N2 * D1, 0.0]
        DD = [D0 * D0, 2.0 * (D0 * D1), D1 * D1]
        WD = [W0 * DD[0], W0 * DD[1] + W1 * DD[0], (W0 * DD[2] + W1 * DD[1]) + W2 * DD[0], W1 * DD[2] + W2 * DD[1],
              W2 * DD[2]]
        A = [(b2 * NN[i] - D0 * ND[i]) + WD[i] for i in range(5)]
        _, v = quartic_roots(A[4], A[3], A[2], A[1], A[0])
    models, ok = np.zeros((4, 12)), [False] * 4
    for s in range(4):
        models[s], ok[s] = _slot(orc, v[s], X, j, b2, q1, N0, N1, N2, D0, D1)
    return models, ok


# ---------------------------------------------------------------- the predicate
def _rot_row(m, k, x, y, z):
    return (m[3 * k] * x + m[3 * k + 1] * y) + m[3 * k + 2] * z


def inliers(m, uv, X, tau, nrm=None, min_cos=0.0):
    """the predicate of every match, vectorised in the contract's operand order"""
    m = [float(v) for v in np.asarray(m, dtype=np.float64).ravel()]
    uv = np.asarray(uv, dtype=np.float64).reshape(-1, 2)
    X = np.asarray(X, dtype=np.float64).reshape(-1, 3)
    tau2 = float(tau) * float(tau)
    with np.errstate(all="ignore"):
        x, y, z = [_rot_row(m, k, X[:, 0], X[:, 1], X[:, 2]) + m[9 + k] for k in range(3)]
        ex, ey = x - uv[:, 0] * z, y - uv[:, 1] * z
        ok = (z > 0.0) & (ex * ex + ey * ey <= tau2 * (z * z))
        if nrm is not None:
            n = np.asarray(nrm, dtype=np.float64).reshape(-1, 3)
            c2 = float(min_cos) * float(min_cos)
            r = [_rot_row(m, k, n[:, 0], n[:, 1], n[:, 2]) for k in range(3)]
            d = (r[0] * x + r[1] * y) + r[2] * z
            ok = ok & (d >= 0.0) & (d * d >= c2 * ((x * x + y * y) + z * z))
    return ok


# ---------------------------------------------------------------- the refit
PAIRS = [(i, k) for i in range(6) for k in range(i, 6)]


def step_sums(m, uv, X, tau, nrm=None, min_cos=0.0):
    """-> list of 28: the sums over the matches m accepts, in the contract's order"""
    mm = [float(v) for v in np.asarray(m, dtype=np.float64).ravel()]
    uv = np.asarray(uv, dtype=np.float64).reshape(-1, 2)
    X = np.asarray(X, dtype=np.float64).reshape(-1, 3)
    inl = inliers(mm, uv, X, tau, nrm, min_cos)
    with np.errstate(all="ignore"):
        Px, Py, Pz = [_rot_row(mm, k, X[:, 0], X[:, 1], X[:, 2]) for k in range(3)]
        x, y, z = Px + mm[9], Py + mm[10], Pz + mm[11]
        iz = 1.0 / z
        xi, yi = x * iz, y * iz
        a, b, c = iz, -(xi * iz), -(yi * iz)
        zero = np.zeros_like(a)
        J0 = [b * Py, a * Pz - b * Px, -(a * Py), a, zero, b]
        J1 = [c * Py - a * Pz, -(c * Px), a * Px, zero, a, c]
        r0, r1 = xi - uv[:, 0], yi - uv[:, 1]
        S = [aref._tiled(np.where(inl, J0[i] * J0[k] + J1[i] * J1[k], 0.0)) for i, k in PAIRS]
        S += [aref._tiled(np.where(inl, J0[i] * r0 + J1[i] * r1, 0.0)) for i in range(6)]
        S.append(aref._tiled(np.where(inl, 1.0, 0.0)))
    return S


def step_solve(S, m):
    """-> the new model (list of 12) or None"""
    m = [float(v) for v in np.asarray(m, dtype=np.float64).ravel()]
    ok = all(_finite(v) for v in S) and S[27] >= 3.0
    A = [[0.0] * 6 for _ in range(6)]
    for n, (i, k) in enumerate(PAIRS):
        A[i][k] = A[k][i] = S[n]
    g = [-S[21 + i] for i in range(6)]
    L = [[0.0] * 6 for _ in range(6)]
    for j in range(6):
        s = A[j][j]
        for k in range(j):
            s = s - L[j][k] * L[j][k]
        ok = ok and s > 0.0
        piv = _sqrt(s)
        L[j][j] = piv
        for i in range(j + 1, 6):
            e = A[i][j]
            for k in range(j):
                e = e - L[i][k] * L[j][k]
            L[i][j] = _div(e, piv)
    yv, d = [0.0] * 6, [0.0] * 6
    for i in range(6):
        s = g[i]
        for k in range(i):
            s = s - L[i][k] * yv[k]
        yv[i] = _div(s, L[i][i])
    for i in range(5, -1, -1):
        s = yv[i]
        for k in range(i + 1, 6):
            s = s - L[k][i] * d[k]
        d[i] = _div(s, L[i][i])
    a0, a1, a2 = d[0] / 2.0, d[1] / 2.0, d[2] / 2.0
    aa = (a0 * a0 + a1 * a1) + a2 * a2
    den, e = 1.0 + aa, 1.0 - aa
    C = [_div(e + 2.0 * (a0 * a0), den), _div(2.0 * (a0 * a1) - 2.0 * a2, den), _div(2.0 * (a0 * a2) + 2.0 * a1, den),
         _div(2.0 * (a1 * a0) + 2.0 * a2, den), _div(e + 2.0 * (a1 * a1), den), _div(2.0 * (a1 * a2) - 2.0 * a0, den),
         _div(2.0 * (a2 * a0) - 2.0 * a1, den), _div(2.0 * (a2 * a1) + 2.0 * a0, den), _div(e + 2.0 * (a2 * a2), den)]
    out = [0.0] * 12
    for r in range(3):
        for c in range(3):
            out[r * 3 + c] = _rot_row(C, r, m[c], m[3 + c], m[6 + c])
    for r in range(3):
        out[9 + r] = m[9 + r] + d[3 + r]
    ok = ok and all(_finite(v) for v in out)
    return out if ok else None


def step(m, uv, X, tau, nrm=None, min_cos=0.0):
    """-> (model' (12,), valid, sums (28,)): zero when invalid"""
    S = step_sums(m, uv, X, tau, nrm, min_cos)
    out = step_solve(S, m)
    return (np.zeros(12), False, np.array(S)) if out is None else (np.array(out), True, np.array(S))


# ---------------------------------------------------------------- RANSAC and rounds
def ransac(orc, uv, X, samples, tau, seed, nrm=None, min_cos=0.0):
    """on matched values -> dict(best, model, mask, counts, models, samples)"""
    uv = np.asarray(uv, dtype=np.float64).reshape(-1, 2)
    X = np.asarray(X, dtype=np.float64).reshape(-1, 3)
    M = X.shape[0]
    H = 4 * samples
    counts = np.full(H, -1, dtype=np.int32)
    models = np.zeros((H, 12))
    drawn = []
    for h in range(samples):
        idx = sample3(seed, h, M)
        drawn.append(idx)
        if idx is None:
            continue
        ms, ok = p3p(orc, X[idx], uv[idx])
        for k in range(4):
            if ok[k]:
                models[4 * h + k] = ms[k]
                counts[4 * h + k] = int(np.count_nonzero(inliers(ms[k], uv, X, tau, nrm, min_cos)))
    best = -1
    for h in range(H):
        if counts[h] >= 0 and (best < 0 or counts[h] > counts[best]):
            best = h
    model = models[best].copy() if best >= 0 else np.zeros(12)
    mask = inliers(model, uv, X, tau, nrm, min_cos) if best >= 0 else np.zeros(M, dtype=bool)
    return dict(best=best, model=model, mask=mask, counts=counts, models=models, samples=drawn)


def rounds(ran, uv, X, tau, iters, nrm=None, min_cos=0.0):
    """fm3d_localize_points' rounds after ransac() -> dict(model, mask, roundCounts, roundModels, adopted)"""
    best = ran["best"]
    m = ran["model"].copy()
    rc = np.full(iters + 1, -2, dtype=np.int32)
    rm = np.zeros((iters, 12))
    cur = int(ran["counts"][best]) if best >= 0 else -1
    rc[0] = cur
    adopted, done = 0, best < 0
    for r in range(iters):
        if done:
            break
        mc, ok, _ = step(m, uv, X, tau, nrm, min_cos)
        cc = int(np.count_nonzero(inliers(mc, uv, X, tau, nrm, min_cos))) if ok else -1
        rc[1 + r], rm[r] = cc, mc
        if ok and cc >= cur:
            m, cur, adopted = mc, cc, adopted + 1
        else:
            done = True
    mask = inliers(m, uv, X, tau, nrm, min_cos) if best >= 0 else np.zeros(np.asarray(X).reshape(-1, 3).shape[0], dtype=bool)
    return dict(model=m, mask=mask, roundCounts=rc, roundModels=rm, adopted=adopted)


def tau_of(cam, max_px):
    return max_px * 2.0 / (cam.fx + cam.fy)


def gather(orc, cam, pts, kpts, matches, nrm=None):
    """the matched values: the keypoints (float32 pixels) through the oracle's undistortion, the points
    and the normals"""
    q = np.asarray(matches["queryIdx"], dtype=np.int64)
    t = np.asarray(matches["trainIdx"], dtype=np.int64)
    kp = np.asarray(kpts, dtype=np.float32).reshape(-1, 2)
    uv = orc.undistort(cam, kp[q].astype(np.float64)) if q.size else np.zeros((0, 2))
    X = np.asarray(pts, dtype=np.float64).reshape(-1, 3)[t]
    return uv, X, None if nrm is None else np.asarray(nrm, dtype=np.float64).reshape(-1, 3)[t]


def localize(orc, cam, pts, kpts, matches, max_px, samples, seed, refine=0, nrm=None, min_cos=0.0):
    """fm3d_localize_points -> dict(g, mask, inliers, best, counts, models, roundCounts, roundModels, adopted)"""
    uv, X, n = gather(orc, cam, pts, kpts, matches, nrm)
    tau = tau_of(cam, max_px)
    ran = ransac(orc, uv, X, samples, tau, seed, n, min_cos)
    out = dict(best=ran["best"], counts=ran["counts"], models=ran["models"], model=ran["model"], mask=ran["mask"],
               ransac=ran, uv=uv, X=X, n=n, tau=tau)
    if refine:
        out.update(rounds(ran, uv, X, tau, refine, n, min_cos))
    else:
        c0 = int(ran["counts"][ran["best"]]) if ran["best"] >= 0 else -1
        out.update(roundCounts=np.array([c0], dtype=np.int32), roundModels=np.zeros((0, 12)), adopted=0)
    out["g"] = g_of(out["model"], out["best"])
    out["inliers"] = np.asarray(matches)[out["mask"]]
    return out


# ---------------------------------------------------------------- the quality recipe
@dataclasses.dataclass
class Cam:
    fx: float = 520.0
    fy: float = 520.0
    cx: float = 320.0
    cy: float = 240.0
    k: tuple = (0.0, 0.0, 0.0, 0.0, 0.0)


def scene(N=600, rng_seed=11, relief=True, sigma_px=0.5, wrong_frac=0.3, angle_deg=12.0, cam=None):
    """The quality case of §3.1f, drawn with default_rng(rng_seed) in this order: N image points uniform
    over the 640 x 480 frame inset by 20 px; their depths uniform in [1.6, 2.3] m (relief True), all
    1.95 m (False: a plane facing the camera) or squeezed about 1.95 m to a spread of `relief` metres; the
    camera-frame points on those rays; a rotation of angle_deg
    about a random axis and t uniform in +-0.3 per axis: the model X = R^T (Xc - t), its normals
    R^T (Xc / |Xc|); Gaussian pixel noise sigma_px on the keypoints, stored as float32 in a random
    permutation (kpts[perm[i]] belongs to X[i]); wrong_frac of the matches given a uniform random
    keypoint -> dict(cam, X, n, kpts, R, t, matches, true)"""
    cam = cam or Cam()
    rng = np.random.default_rng(rng_seed)
    px = np.stack([rng.uniform(20.0, 620.0, N), rng.uniform(20.0, 460.0, N)], axis=1)
    depth = rng.uniform(1.6, 2.3, N)
    if relief is False:
        depth = np.full(N, 1.95)
    elif relief is not True:
        depth = 1.95 + (depth - 1.95) * (float(relief) / 0.7)
    Xc = np.stack([(px[:, 0] - cam.cx) / cam.fx * depth, (px[:, 1] - cam.cy) / cam.fy * depth, depth], axis=1)
    R = rodrigues(rng.normal(size=3), math.radians(angle_deg))
    t = rng.uniform(-0.3, 0.3, 3)
    X = (Xc - t) @ R
    n = (Xc / np.linalg.norm(Xc, axis=1)[:, None]) @ R
    perm = rng.permutation(N)
    kpts = np.zeros((N, 2), dtype=np.float32)
    kpts[perm] = (px + rng.normal(0.0, sigma_px, (N, 2))).astype(np.float32)
    wrong = rng.random(N) < wrong_frac
    query = perm.copy()
    query[wrong] = rng.integers(0, N, int(wrong.sum()))
    m = np.zeros(N, dtype=DMATCH)
    m["queryIdx"], m["trainIdx"] = query, np.arange(N)
    return dict(cam=cam, X=X, n=n, kpts=kpts, R=R, t=t, matches=m, true=query == perm)


_CASE = {}


def quality_case(orc, seed, relief=True, refine=0, normals=False, samples=256, max_px=2.0):
    """scene() and the restatement's run on it, computed once per process"""
    key = (seed, relief, refine, normals, samples, max_px)
    if key not in _CASE:
        if ("scene", relief) not in _CASE:
            _CASE[("scene", relief)] = scene(relief=relief)
        p = _CASE[("scene", relief)]
        _CASE[key] = localize(orc, p["cam"], p["X"], p["kpts"], p["matches"], max_px, samples, seed, refine,
                              p["n"] if normals else None, 0.5)
    return _CASE[("scene", relief)], _CASE[key]
