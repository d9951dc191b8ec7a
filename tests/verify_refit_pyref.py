"""The refit on the inliers ("Refinement") restated in plain Python floats, in the
order the contract writes it: the 45 sums of a a^T over the pairs the model accepts (a tile's leaves, its
balanced tree, the tiles in order), the cyclic Jacobi iteration on the symmetric 9 x 9, the projection
(verify_pyref.project) and the rounds.  The sums are additions of Python floats or element-by-element
additions of equally long numpy arrays -- never a numpy reduction, whose order is not the contract's."""
import math

import numpy as np

import verify_pyref as ref

TILE = 1024
LANES = 256
PAIRS = [(r, c) for r in range(9) for c in range(r, 9)]
TOL = 10.0 * 2.220446049250313e-16  # 10 DBL_EPSILON
SWEEPS = 30


def rows9(x1, x2):
    """(n, 9): set_row's entries of every pair (products of two doubles: element by element)"""
    x1 = np.asarray(x1, dtype=np.float64).reshape(-1, 2)
    x2 = np.asarray(x2, dtype=np.float64).reshape(-1, 2)
    a, b, c, d = x1[:, 0], x1[:, 1], x2[:, 0], x2[:, 1]
    with np.errstate(all="ignore"):
        return np.stack([c * a, c * b, c, d * a, d * b, d, a, b, np.ones_like(a)], axis=1)


def tile_tree(v):
    """the sum of one tile's 1,024 slot values: leaf t = (v[t] + v[256 + t]) + (v[512 + t] + v[768 + t]),
    then s[i] = s[2 i] + s[2 i + 1] level by level"""
    assert v.shape == (TILE,)
    with np.errstate(all="ignore"):
        s = (v[0:LANES] + v[LANES:2 * LANES]) + (v[2 * LANES:3 * LANES] + v[3 * LANES:4 * LANES])
        while s.shape[0] > 1:
            s = s[0::2] + s[1::2]
    return float(s[0])


def slots(E, x1, x2, tau):
    """(tiles, 45, 1024): every slot's value -- a[r] a[c] when the pair is in, +0.0 otherwise and in the pad"""
    inl = ref.inliers(E, x1, x2, tau)
    A = rows9(x1, x2)
    n = A.shape[0]
    tiles = (n + TILE - 1) // TILE
    out = np.zeros((tiles, len(PAIRS), TILE))
    for j, (r, c) in enumerate(PAIRS):
        with np.errstate(all="ignore"):
            v = np.where(inl, A[:, r] * A[:, c], 0.0)  # a select: a NaN product of a pair that is out adds nothing
        flat = np.zeros(tiles * TILE)
        flat[:n] = v
        out[:, j, :] = flat.reshape(tiles, TILE)
    return out, int(np.count_nonzero(inl))


def normal45(E, x1, x2, tau, order="tree"):
    """-> (N45 list of 45 floats, pairs in); order="index" adds the slots one after the other (what the
    contract does NOT do: the tests show that the two differ)"""
    v, cnt = slots(E, x1, x2, tau)
    N = []
    for j in range(len(PAIRS)):
        s = 0.0
        if order == "tree":
            for t in range(v.shape[0]):
                s = s + tile_tree(v[t, j])
        else:
            for x in v[:, j, :].ravel().tolist():
                s = s + x
        N.append(s)
    return N, cnt


def jacobi_null9(N45):
    """the eigenvector (list of 9) under the smallest diagonal entry after the cyclic Jacobi iteration"""
    S = [[0.0] * 9 for _ in range(9)]
    for (r, c), v in zip(PAIRS, N45):
        S[r][c] = S[c][r] = float(v)
    V = [[1.0 if r == c else 0.0 for c in range(9)] for r in range(9)]
    for _ in range(SWEEPS):
        rotated = False
        for p in range(8):
            for q in range(p + 1, 9):
                apq, app, aqq = S[p][q], S[p][p], S[q][q]
                prod = app * aqq
                thr = TOL * (math.sqrt(prod) if prod >= 0.0 else math.nan)
                if not (abs(apq) > thr):
                    continue
                rotated = True
                theta = (aqq - app) / (2.0 * apq)
                sq = theta * theta + 1.0
                t = (-1.0 if theta < 0.0 else 1.0) / (abs(theta) + math.sqrt(sq))
                c = 1.0 / math.sqrt(t * t + 1.0)
                s = t * c
                h = t * apq
                S[p][p] = app - h
                S[q][q] = aqq + h
                S[p][q] = S[q][p] = 0.0
                for k in range(9):
                    if k != p and k != q:
                        akp, akq = S[k][p], S[k][q]
                        S[k][p] = S[p][k] = c * akp - s * akq
                        S[k][q] = S[q][k] = s * akp + c * akq
                    vkp, vkq = V[k][p], V[k][q]
                    V[k][p] = c * vkp - s * vkq
                    V[k][q] = s * vkp + c * vkq
        if not rotated:
            break
    m = 0
    for j in range(1, 9):
        if S[j][j] < S[m][m]:
            m = j
    return [V[k][m] for k in range(9)]


def refit_from_normal(orc, N45):
    """-> (E' (3, 3), valid): zero when invalid"""
    bad = (np.zeros((3, 3)), False)
    if not all(math.isfinite(v) for v in N45) or not (N45[-1] >= 8.0):
        return bad
    e = jacobi_null9(N45)
    if not all(math.isfinite(v) for v in e):
        return bad
    E = ref.project(orc, e)
    return bad if E is None else (E, True)


def refit(orc, E, x1, x2, tau):
    N, _ = normal45(E, x1, x2, tau)
    return refit_from_normal(orc, N)


def rounds(orc, E0, c0, best, x1, x2, tau, iters):
    """fm3d_verify_matches_refined's rounds on the RANSAC's result -> dict(E, mask, roundCounts,
    roundModels, adopted)"""
    x1 = np.asarray(x1, dtype=np.float64).reshape(-1, 2)
    x2 = np.asarray(x2, dtype=np.float64).reshape(-1, 2)
    E = np.array(E0, dtype=np.float64).reshape(3, 3)
    rc = np.full(iters + 1, -2, dtype=np.int32)
    rm = np.zeros((iters, 3, 3))
    rc[0] = c0 if best >= 0 else -1
    adopted, cur, done = 0, c0, best < 0
    for r in range(iters):
        if done:
            break
        Ec, ok = refit(orc, E, x1, x2, tau)
        cc = int(np.count_nonzero(ref.inliers(Ec, x1, x2, tau))) if ok else -1
        rc[1 + r], rm[r] = cc, Ec
        if ok and cc >= cur:
            E, cur, adopted = Ec, cc, adopted + 1
        else:
            done = True
    mask = ref.inliers(E, x1, x2, tau) if best >= 0 else np.zeros(x1.shape[0], dtype=bool)
    return dict(E=E, mask=mask, roundCounts=rc, roundModels=rm, adopted=adopted)


def refined(orc, ran, x1, x2, tau, iters):
    """the rounds after a run of verify_pyref.ransac"""
    best = ran["best"]
    c0 = int(ran["counts"][best]) if best >= 0 else -1
    return rounds(orc, ran["E"], c0, best, x1, x2, tau, iters)


def noisy_inputs(synth, M, sigma=0.5, rng_seed=100):
    """The quality case: verify_pyref.verify_inputs' pair with Gaussian noise of sigma pixels on both
    keypoint sets (default_rng(rng_seed): kp1 first, then kp2), its first M matches
    -> (pair, kp1, kp2, matches)"""
    pair, m, _ = ref.verify_inputs(synth)
    rng = np.random.default_rng(rng_seed)
    kp1 = (pair.kp1 + rng.normal(0.0, sigma, pair.kp1.shape)).astype(np.float32)
    kp2 = (pair.kp2 + rng.normal(0.0, sigma, pair.kp2.shape)).astype(np.float32)
    return pair, kp1, kp2, m[:M]


def rot_err_deg(Ra, Rb):
    return math.degrees(math.acos(max(-1.0, min(1.0, (np.trace(Ra.T @ Rb) - 1) / 2))))
