"""The 3D-3D alignment's contract restated in plain Python and numpy, in the order
include/fm3d_rigid3.h writes it: Python floats are IEEE doubles and nothing here contracts a multiply
and an add, so the library (host and device) has to give the same bits.  The sampler's draws and the
3 x 3 SVD are verify_pyref's (the oracle's restatement of OpenCV 2.4's JacobiSVD), the tile tree
verify_refit_pyref's.  The sums are additions of Python floats or element-by-element additions of
equally long numpy arrays -- never a numpy reduction, whose order is not the contract's."""
import math

import numpy as np

import verify_pyref as ref
import verify_refit_pyref as rref

TILE = rref.TILE


def sample3(seed, h, M):
    """the first three distinct draws of 64, in their order, or None"""
    if M < 3:
        return None
    idx = []
    for a in range(64):
        v = ref.draw(seed, h, a, M)
        if v not in idx:
            idx.append(v)
            if len(idx) == 3:
                return idx
    return None


def _rot_row(m, k, x, y, z):
    return (m[3 * k] * x + m[3 * k + 1] * y) + m[3 * k + 2] * z


def solve(orc, H, ca, cb):
    """the model (list of 12: R row-major, then t) from the row-major cross matrix H (list of 9) and the
    centroids, or None"""
    if not all(math.isfinite(v) for v in H):
        return None
    s = ref.svd_e(orc, np.array(H, dtype=np.float64).reshape(3, 3))
    if s is None:
        return None
    u0, u1, v0, v1 = s
    u2, v2 = ref._cross(u0, u1), ref._cross(v0, v1)
    m = [0.0] * 12
    for r in range(3):
        for c in range(3):
            m[r * 3 + c] = (v0[r] * u0[c] + v1[r] * u1[c]) + v2[r] * u2[c]
    for r in range(3):
        m[9 + r] = cb[r] - _rot_row(m, r, ca[0], ca[1], ca[2])
    if not all(math.isfinite(v) for v in m):
        return None
    return m


def from3(orc, a, b):
    """-> (model (12,), valid): zero when invalid"""
    a = [[float(v) for v in p] for p in np.asarray(a, dtype=np.float64).reshape(3, 3)]
    b = [[float(v) for v in p] for p in np.asarray(b, dtype=np.float64).reshape(3, 3)]
    with np.errstate(all="ignore"):
        ca = [((a[0][r] + a[1][r]) + a[2][r]) / 3.0 for r in range(3)]
        cb = [((b[0][r] + b[1][r]) + b[2][r]) / 3.0 for r in range(3)]
        H = []
        for r in range(3):
            for c in range(3):
                s = 0.0
                for k in range(3):
                    s = s + (a[k][r] - ca[r]) * (b[k][c] - cb[c])
                H.append(s)
    m = solve(orc, H, ca, cb)
    return (np.zeros(12), False) if m is None else (np.array(m), True)


def inliers(m, a, b, max_dist, na=None, nb=None, min_cos=0.0):
    """the predicate of every pair, vectorised in the contract's operand order"""
    m = [float(v) for v in np.asarray(m, dtype=np.float64).ravel()]
    a = np.asarray(a, dtype=np.float64).reshape(-1, 3)
    b = np.asarray(b, dtype=np.float64).reshape(-1, 3)
    tau2 = float(max_dist) * float(max_dist)
    with np.errstate(all="ignore"):
        d = [(_rot_row(m, k, a[:, 0], a[:, 1], a[:, 2]) + m[9 + k]) - b[:, k] for k in range(3)]
        ok = (d[0] * d[0] + d[1] * d[1]) + d[2] * d[2] <= tau2
        if na is not None:
            na = np.asarray(na, dtype=np.float64).reshape(-1, 3)
            nb = np.asarray(nb, dtype=np.float64).reshape(-1, 3)
            r = [_rot_row(m, k, na[:, 0], na[:, 1], na[:, 2]) for k in range(3)]
            ok = ok & ((r[0] * nb[:, 0] + r[1] * nb[:, 1]) + r[2] * nb[:, 2] >= float(min_cos))
    return ok


def _gather(pts_a, pts_b, matches, na=None, nb=None):
    q = np.asarray(matches["queryIdx"], dtype=np.int64)
    t = np.asarray(matches["trainIdx"], dtype=np.int64)
    a = np.asarray(pts_a, dtype=np.float64).reshape(-1, 3)[q]
    b = np.asarray(pts_b, dtype=np.float64).reshape(-1, 3)[t]
    if na is None:
        return a, b, None, None
    return a, b, np.asarray(na, dtype=np.float64).reshape(-1, 3)[q], np.asarray(nb, dtype=np.float64).reshape(-1, 3)[t]


def ransac(orc, a, b, hypotheses, max_dist, seed, na=None, nb=None, min_cos=0.0):
    """on matched coordinates (M, 3) -> dict(best, model, mask, counts, models, samples)"""
    a = np.asarray(a, dtype=np.float64).reshape(-1, 3)
    b = np.asarray(b, dtype=np.float64).reshape(-1, 3)
    M = a.shape[0]
    counts = np.full(hypotheses, -1, dtype=np.int32)
    models = np.zeros((hypotheses, 12))
    samples = []
    for h in range(hypotheses):
        idx = sample3(seed, h, M)
        samples.append(idx)
        if idx is None:
            continue
        m, ok = from3(orc, a[idx], b[idx])
        if ok:
            models[h] = m
            counts[h] = int(np.count_nonzero(inliers(m, a, b, max_dist, na, nb, min_cos)))
    best = -1
    for h in range(hypotheses):
        if counts[h] >= 0 and (best < 0 or counts[h] > counts[best]):
            best = h
    model = models[best].copy() if best >= 0 else np.zeros(12)
    mask = inliers(model, a, b, max_dist, na, nb, min_cos) if best >= 0 else np.zeros(M, dtype=bool)
    return dict(best=best, model=model, mask=mask, counts=counts, models=models, samples=samples)


def _tiled(v):
    """the sum of the slot values v (n,) in the contract's order: tiles of 1,024 (the pad +0.0), a
    tile's tree, the tiles in order from +0.0"""
    n = v.shape[0]
    tiles = (n + TILE - 1) // TILE
    flat = np.zeros(tiles * TILE)
    flat[:n] = v
    s = 0.0
    for t in range(tiles):
        s = s + rref.tile_tree(flat[t * TILE:(t + 1) * TILE])
    return s


def refit_sums(m, a, b, max_dist, na=None, nb=None, min_cos=0.0):
    """-> (S1 list of 7, S2 list of 9): the two passes' sums over the pairs m accepts"""
    a = np.asarray(a, dtype=np.float64).reshape(-1, 3)
    b = np.asarray(b, dtype=np.float64).reshape(-1, 3)
    inl = inliers(m, a, b, max_dist, na, nb, min_cos)
    with np.errstate(all="ignore"):
        S1 = [_tiled(np.where(inl, a[:, r], 0.0)) for r in range(3)]
        S1 += [_tiled(np.where(inl, b[:, r], 0.0)) for r in range(3)]
        S1.append(_tiled(np.where(inl, 1.0, 0.0)))
        n = np.float64(S1[6])
        ca = [float(np.float64(S1[r]) / n) for r in range(3)]
        cb = [float(np.float64(S1[3 + r]) / n) for r in range(3)]
        S2 = [_tiled(np.where(inl, (a[:, r] - ca[r]) * (b[:, c] - cb[c]), 0.0)) for r in range(3) for c in range(3)]
    return S1, S2, ca, cb


def refit(orc, m, a, b, max_dist, na=None, nb=None, min_cos=0.0):
    """-> (model' (12,), valid, sums (16,)): zero when invalid"""
    S1, S2, ca, cb = refit_sums(m, a, b, max_dist, na, nb, min_cos)
    sums = np.array(S1 + S2)
    out = None
    if all(math.isfinite(v) for v in S1) and S1[6] >= 3.0:
        out = solve(orc, S2, ca, cb)
    return (np.zeros(12), False, sums) if out is None else (np.array(out), True, sums)


def rounds(orc, ran, a, b, max_dist, iters, na=None, nb=None, min_cos=0.0):
    """fm3d_align_points' rounds after ransac() -> dict(model, mask, roundCounts, roundModels, adopted)"""
    a = np.asarray(a, dtype=np.float64).reshape(-1, 3)
    b = np.asarray(b, dtype=np.float64).reshape(-1, 3)
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
        mc, ok, _ = refit(orc, m, a, b, max_dist, na, nb, min_cos)
        cc = int(np.count_nonzero(inliers(mc, a, b, max_dist, na, nb, min_cos))) if ok else -1
        rc[1 + r], rm[r] = cc, mc
        if ok and cc >= cur:
            m, cur, adopted = mc, cc, adopted + 1
        else:
            done = True
    mask = inliers(m, a, b, max_dist, na, nb, min_cos) if best >= 0 else np.zeros(a.shape[0], dtype=bool)
    return dict(model=m, mask=mask, roundCounts=rc, roundModels=rm, adopted=adopted)


def g_of(model, best):
    """the row-major 4 x 4 [R | t; 0 0 0 1], zero without a model"""
    g = np.zeros((4, 4))
    if best >= 0:
        g[:3, :3] = np.asarray(model[:9]).reshape(3, 3)
        g[:3, 3] = model[9:12]
        g[3, 3] = 1.0
    return g


def align(orc, pts_a, pts_b, matches, max_dist, hypotheses, seed, refine=0, na=None, nb=None, min_cos=0.0):
    """fm3d_align_points -> dict(g, mask, inliers, best, counts, models, roundCounts, roundModels, adopted)"""
    a, b, ua, ub = _gather(pts_a, pts_b, matches, na, nb)
    ran = ransac(orc, a, b, hypotheses, max_dist, seed, ua, ub, min_cos)
    out = dict(best=ran["best"], counts=ran["counts"], models=ran["models"], model=ran["model"], mask=ran["mask"],
               ransac=ran, a=a, b=b)
    if refine:
        out.update(rounds(orc, ran, a, b, max_dist, refine, ua, ub, min_cos))
    else:
        c0 = int(ran["counts"][ran["best"]]) if ran["best"] >= 0 else -1
        out.update(roundCounts=np.array([c0], dtype=np.int32), roundModels=np.zeros((0, 12)), adopted=0)
    out["g"] = g_of(out["model"], out["best"])
    out["inliers"] = np.asarray(matches)[out["mask"]]
    return out


def rot_err_deg(Ra, Rb):
    return math.degrees(math.acos(max(-1.0, min(1.0, (np.trace(Ra.T @ Rb) - 1) / 2))))


def rodrigues(axis, angle):
    axis = np.asarray(axis, dtype=np.float64)
    axis = axis / np.linalg.norm(axis)
    K = np.array([[0, -axis[2], axis[1]], [axis[2], 0, -axis[0]], [-axis[1], axis[0], 0]])
    return np.eye(3) + math.sin(angle) * K + (1 - math.cos(angle)) * (K @ K)


DMATCH = np.dtype([("queryIdx", "<i4"), ("trainIdx", "<i4"), ("imgIdx", "<i4"), ("distance", "<f4")])


def model_pair(N=600, rng_seed=11, sigma=0.001, wrong_frac=0.3, angle_deg=20.0):
    """The quality case of §3.1e, drawn with default_rng(rng_seed) in this order: N points A uniform in
    x [-1, 1], y [-0.75, 0.75], z [1.5, 2.4]; unit normals; a rotation of angle_deg about a random axis;
    t uniform in +-0.3 per axis; a permutation; B = R A + t plus Gaussian noise sigma, stored permuted
    (B[perm[i]] belongs to A[i]; its normal is R n_a); wrong_frac of the matches given a uniform random
    train index -> dict(A, nA, B, nB, R, t, matches, true)"""
    rng = np.random.default_rng(rng_seed)
    A = np.stack([rng.uniform(-1.0, 1.0, N), rng.uniform(-0.75, 0.75, N), rng.uniform(1.5, 2.4, N)], axis=1)
    nA = rng.normal(size=(N, 3))
    nA /= np.linalg.norm(nA, axis=1)[:, None]
    R = rodrigues(rng.normal(size=3), math.radians(angle_deg))
    t = rng.uniform(-0.3, 0.3, 3)
    perm = rng.permutation(N)
    noise = rng.normal(0.0, sigma, (N, 3))
    B, nB = np.zeros((N, 3)), np.zeros((N, 3))
    B[perm] = A @ R.T + t + noise
    nB[perm] = nA @ R.T
    wrong = rng.random(N) < wrong_frac
    train = perm.copy()
    train[wrong] = rng.integers(0, N, int(wrong.sum()))
    m = np.zeros(N, dtype=DMATCH)
    m["queryIdx"], m["trainIdx"] = np.arange(N), train
    return dict(A=A, nA=nA, B=B, nB=nB, R=R, t=t, matches=m, true=train == perm)


_CASE = {}


def quality_case(orc, seed, refine=0, normals=False, hypotheses=256, max_dist=0.005):
    """model_pair() and the restatement's run on it, computed once per process"""
    key = (seed, refine, normals, hypotheses, max_dist)
    if key not in _CASE:
        if "pair" not in _CASE:
            _CASE["pair"] = model_pair()
        p = _CASE["pair"]
        na, nb = (p["nA"], p["nB"]) if normals else (None, None)
        _CASE[key] = align(orc, p["A"], p["B"], p["matches"], max_dist, hypotheses, seed, refine, na, nb, 0.9)
    return _CASE["pair"], _CASE[key]
