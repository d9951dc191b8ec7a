"""The geometric verification's contract restated in plain Python and numpy, in the
order the contract writes it: Python floats are IEEE doubles and nothing here contracts a multiply
and an add, so the library (include/fm3d_epi8.h, host and device) has to give the same bits.  The
3 x 3 SVD is the oracle's restatement of OpenCV 2.4's JacobiSVD (oracle.cv_svd), the undistortion the
oracle's (oracle.undistort)."""
import math

import numpy as np

MASK64 = (1 << 64) - 1
DBL_MIN = 2.2250738585072014e-308
DBL_MAX = 1.7976931348623157e308


def draw(seed, h, a, M):
    z = (seed + 0x9E3779B97F4A7C15 * (1 + 64 * h + a)) & MASK64
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & MASK64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & MASK64
    z ^= z >> 31
    return ((z >> 32) * M) >> 32


def sample(seed, h, M):
    """the first eight distinct draws of 64, or None"""
    if M < 8:
        return None
    idx = []
    for a in range(64):
        v = draw(seed, h, a, M)
        if v not in idx:
            idx.append(v)
            if len(idx) == 8:
                return idx
    return None


def rows(x1, x2):
    A = []
    for (a, b), (c, d) in zip(x1, x2):
        a, b, c, d = float(a), float(b), float(c), float(d)
        A.append([c * a, c * b, c, d * a, d * b, d, a, b, 1.0])
    return A


def null8(A):
    """Gauss-Jordan with full pivoting on the 8 x 9 rows -> the unit null vector (list of 9) or None"""
    A = [list(r) for r in A]
    used, col = [False] * 9, []
    for s in range(8):
        best, br, bc = -1.0, -1, -1
        for r in range(s, 8):
            for c in range(9):
                if used[c]:
                    continue
                v = abs(A[r][c])
                if v > best:  # False for a NaN
                    best, br, bc = v, r, c
        if br < 0:
            return None
        p = A[br][bc]
        if p == 0.0 or not (abs(p) <= DBL_MAX):
            return None
        A[s], A[br] = A[br], A[s]
        for r in range(8):
            if r == s:
                continue
            f = A[r][bc] / p
            if f != 0.0:
                for j in range(9):
                    A[r][j] = A[r][j] - f * A[s][j]
        used[bc] = True
        col.append(bc)
    free = used.index(False)
    x = [1.0] * 9
    for s in range(8):
        x[col[s]] = -A[s][free] / A[s][col[s]]
    ss = 0.0
    for c in range(9):
        ss += x[c] * x[c]
    if not (ss <= DBL_MAX):
        return None
    inv = 1.0 / math.sqrt(ss)
    return [v * inv for v in x]


def svd_e(orc, E):
    """(u0, u1, v0, v1) of a 3 x 3 E in JacobiSVD's order, or None when W[1] <= DBL_MIN (or NaN)"""
    E = np.asarray(E, dtype=np.float64).reshape(3, 3)
    if not np.isfinite(E).all():
        return None  # (the product's sweep ends with W[1] NaN, which fails W[1] > DBL_MIN)
    w, u, vt = orc.cv_svd(E)
    if not (w[1] > DBL_MIN):
        return None
    return [[float(u[r, i]) for r in range(3)] for i in range(2)] + [[float(vt[i, c]) for c in range(3)] for i in range(2)]


def project(orc, e):
    s = svd_e(orc, e)
    if s is None:
        return None
    u0, u1, v0, v1 = s
    return np.array([[u0[r] * v0[c] + u1[r] * v1[c] for c in range(3)] for r in range(3)])


def from8(orc, x1, x2):
    """-> (E (3, 3), valid): zero when invalid"""
    e = null8(rows(x1, x2))
    E = project(orc, e) if e is not None else None
    return (np.zeros((3, 3)), False) if E is None else (E, True)


def tau_of(cam, max_px):
    return max_px * 2.0 / (cam.fx + cam.fy)


def inliers(E, x1, x2, tau):
    """the Sampson predicate of every pair, vectorised in the contract's operand order"""
    E = np.asarray(E, dtype=np.float64).reshape(3, 3)
    x1 = np.asarray(x1, dtype=np.float64).reshape(-1, 2)
    x2 = np.asarray(x2, dtype=np.float64).reshape(-1, 2)
    a, b, c, d = x1[:, 0], x1[:, 1], x2[:, 0], x2[:, 1]
    tau2 = tau * tau
    with np.errstate(all="ignore"):
        l0 = (E[0, 0] * a + E[0, 1] * b) + E[0, 2]
        l1 = (E[1, 0] * a + E[1, 1] * b) + E[1, 2]
        l2 = (E[2, 0] * a + E[2, 1] * b) + E[2, 2]
        m0 = (E[0, 0] * c + E[1, 0] * d) + E[2, 0]
        m1 = (E[0, 1] * c + E[1, 1] * d) + E[2, 1]
        r = (c * l0 + d * l1) + l2
        den = ((l0 * l0 + l1 * l1) + m0 * m0) + m1 * m1
        return (den > 0) & (r * r <= tau2 * den)


def coords(orc, cam, kp1, kp2, matches):
    """the undistorted normalised coordinates of every match, doubles"""
    q = np.asarray(matches["queryIdx"], dtype=np.int64)
    t = np.asarray(matches["trainIdx"], dtype=np.int64)
    k1 = np.asarray(kp1, dtype=np.float32).reshape(-1, 2)
    k2 = np.asarray(kp2, dtype=np.float32).reshape(-1, 2)
    return orc.undistort(cam, k1[q].astype(np.float64)), orc.undistort(cam, k2[t].astype(np.float64))


def ransac(orc, x1, x2, hypotheses, tau, seed):
    """-> dict(best, E, mask, counts, models, samples): fm3d_verify_matches on coordinates"""
    x1 = np.asarray(x1, dtype=np.float64).reshape(-1, 2)
    x2 = np.asarray(x2, dtype=np.float64).reshape(-1, 2)
    M = x1.shape[0]
    counts = np.full(hypotheses, -1, dtype=np.int32)
    models = np.zeros((hypotheses, 3, 3))
    samples = []
    for h in range(hypotheses):
        idx = sample(seed, h, M)
        samples.append(idx)
        if idx is None:
            continue
        E, ok = from8(orc, x1[idx], x2[idx])
        if ok:
            models[h] = E
            counts[h] = int(inliers(E, x1, x2, tau).sum())
    best = -1
    for h in range(hypotheses):
        if counts[h] >= 0 and (best < 0 or counts[h] > counts[best]):
            best = h
    E = models[best].copy() if best >= 0 else np.zeros((3, 3))
    mask = inliers(E, x1, x2, tau) if best >= 0 else np.zeros(M, dtype=bool)
    return dict(best=best, E=E, mask=mask, counts=counts, models=models, samples=samples)


def _dot(a, b):
    return (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2]


def _cross(a, b):
    return [a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0]]


def pose(orc, E, x1, x2, baseline=1.0):
    """fm3d_pose_from_epipolar -> (g12 (4, 4), votes (4,)) or None"""
    s = svd_e(orc, E)
    if s is None:
        return None
    u0, u1, v0, v1 = s
    u2, v2 = _cross(u0, u1), _cross(v0, v1)
    Ra = [[(u1[r] * v0[c] + (-u0[r]) * v1[c]) + u2[r] * v2[c] for c in range(3)] for r in range(3)]
    Rb = [[((-u1[r]) * v0[c] + u0[r] * v1[c]) + u2[r] * v2[c] for c in range(3)] for r in range(3)]
    cands = [(Ra, 1.0), (Ra, -1.0), (Rb, 1.0), (Rb, -1.0)]
    votes = [0, 0, 0, 0]
    x1 = np.asarray(x1, dtype=np.float64).reshape(-1, 2)
    x2 = np.asarray(x2, dtype=np.float64).reshape(-1, 2)
    for k, (R, sg) in enumerate(cands):
        t = [sg * u2[0], sg * u2[1], sg * u2[2]]
        for (px, py), (qx, qy) in zip(x1.tolist(), x2.tolist()):
            p, b = [px, py, 1.0], [qx, qy, 1.0]
            a = [_dot(R[0], p), _dot(R[1], p), _dot(R[2], p)]
            aa, ab, bb, at, bt = _dot(a, a), _dot(a, b), _dot(b, b), _dot(a, t), _dot(b, t)
            det = aa * bb - ab * ab
            with np.errstate(all="ignore"):  # IEEE division: a zero det gives inf or NaN, as in C
                z1 = np.float64(ab * bt - bb * at) / np.float64(det)
                z2 = np.float64(aa * bt - ab * at) / np.float64(det)
            votes[k] += 1 if (z1 > 0.0 and z2 > 0.0) else 0
    bk = 0
    for k in range(1, 4):
        if votes[k] > votes[bk]:
            bk = k
    R, sg = cands[bk]
    g = np.eye(4)
    for r in range(3):
        g[r, :3] = R[r]
        g[r, 3] = baseline * (sg * u2[r])
    return g, np.array(votes, dtype=np.int32)


def verify_inputs(synth, n=2000, seed=11, wrong_frac=0.3, wrong_seed=5, distortion=False):
    """The end-to-end case of §3.1d: a synthetic pair under the reference camera (zero distortion
    unless asked), its true pairs as the matches, wrong_frac of them given a random train index
    -> (pair, matches (DMATCH-like structured array), true (bool per match))"""
    cam = synth.Camera.reference(640)
    if not distortion:
        cam = synth.Camera(cam.fx, cam.fy, cam.cx, cam.cy, (0.0, 0.0, 0.0, 0.0, 0.0))
    pair = synth.make_frame_pair(n, seed=seed, cam=cam)
    q = np.nonzero(pair.true_train >= 0)[0]
    t = pair.true_train[q].copy()
    rng = np.random.default_rng(wrong_seed)
    wrong = rng.random(q.size) < wrong_frac
    t[wrong] = rng.integers(0, pair.kp2.shape[0], int(wrong.sum()))
    true = t == pair.true_train[q]
    m = np.zeros(q.size, dtype=[("queryIdx", "<i4"), ("trainIdx", "<i4"), ("imgIdx", "<i4"), ("distance", "<f4")])
    m["queryIdx"], m["trainIdx"] = q, t
    return pair, m, true


_CASE = {}


def reference_case(synth, orc, hypotheses=512, max_px=1.0, seed=0):
    """verify_inputs() with its coordinates and the restatement's run, computed once per process:
    dict(pair, matches, true, x1, x2, tau, ref)"""
    key = (hypotheses, max_px, seed)
    if key not in _CASE:
        pair, m, true = verify_inputs(synth)
        x1, x2 = coords(orc, pair.cam, pair.kp1, pair.kp2, m)
        tau = tau_of(pair.cam, max_px)
        _CASE[key] = dict(pair=pair, matches=m, true=true, x1=x1, x2=x2, tau=tau, hypotheses=hypotheses,
                          max_px=max_px, seed=seed, ref=ransac(orc, x1, x2, hypotheses, tau, seed))
    return _CASE[key]
