"""A numpy statement of the float matcher's bf16 prefilter (csrc/fm3d_match.hip: f32_bf16_rows_kernel,
knn2_bf16_kernel, knn2_bf16_bound_kernel, knn2_bf16_margin_kernel) and the inputs that pin its error
model -- test infrastructure shared by tests/test_f32_prefilter_bound.py (CPU: the model itself) and
the GPU tests (tests/test_gpu_f32_mfma.py, tests/test_cross_check.py: the same inputs through the
library).  numpy only; nothing here calls the library.

The emulation is the prefilter's arithmetic without its fp32 roundings: rows rounded to bf16 (RNE, the
kernel's bit arithmetic), exact products, float64 accumulation.  The margin is the kernel's expression
with the |a| B_max coefficient as a parameter, so a test can ask what a given coefficient keeps."""
import numpy as np

K_T = 128          # train rows per LDS tile (kT)
K_Q = 128          # queries per workgroup (kQ)
K_CAND_MAX = 32    # the two-pass form's list (kCandMax)
K_CAND_MAX2 = 128  # the fused pass's list (kCandMax2)


def bf16_rne(x):
    """float32 -> the bf16 value (as float32): (u + 0x7fff + ((u >> 16) & 1)) >> 16, the kernel's"""
    u = np.ascontiguousarray(x, dtype=np.float32).view(np.uint32).astype(np.uint64)
    r = ((u + 0x7FFF + ((u >> 16) & 1)) & 0xFFFFFFFF) >> 16  # uint32 arithmetic
    return (r << 16).astype(np.uint32).view(np.float32).reshape(np.shape(x))


def norms2_f32(X):
    """|row|^2 as the conversion kernel's fp32 holds it (to within its summation order)"""
    X = np.asarray(X, dtype=np.float32)
    with np.errstate(over="ignore", invalid="ignore"):
        return (X * X).sum(axis=1, dtype=np.float32)


def exact_keys(A, B):
    """s_j = |a - b_j|^2 - |a|^2 = |b_j|^2 - 2 a.b_j in float64"""
    A64, B64 = np.asarray(A, dtype=np.float64), np.asarray(B, dtype=np.float64)
    return (B64 * B64).sum(axis=1)[None, :] - 2.0 * (A64 @ B64.T)


def prefilter_keys(A, B):
    """s'_j = |b_j|^2 - 2 bf16(a).bf16(b_j) in float64"""
    B64 = np.asarray(B, dtype=np.float64)
    with np.errstate(over="ignore", invalid="ignore"):
        return (B64 * B64).sum(axis=1)[None, :] - 2.0 * (bf16_rne(A).astype(np.float64) @ bf16_rne(B).astype(np.float64).T)


def margin(A, B, c):
    """knn2_bf16_margin_kernel: 2 (c |a| Bmax + 1e-5 Bmax^2) + 2 * 2e-5 (|a| + Bmax)^2 + 1e-6 (|a| + Bmax)^2,
    rounded up to fp32; -inf for a query the kernel sends to the exact rescan"""
    nb2 = norms2_f32(B)
    bmax2 = np.float32(np.inf) if not np.all(nb2 <= np.float32(3.4e38)) else nb2.max()  # NaN / inf: +inf
    with np.errstate(over="ignore", invalid="ignore"):
        a = np.sqrt(norms2_f32(A).astype(np.float64))
        bm = np.sqrt(np.float64(bmax2))
        m = 2 * (c * a * bm + 1e-5 * bm * bm) + 2 * 2e-5 * (a + bm) * (a + bm) + 1e-6 * (a + bm) * (a + bm)
        ok = (m == m) & (m < 1e37) & (a < 1e18) & (a + bm > 1e-10)
        m32 = m.astype(np.float32)
        m32 = np.where(m32.astype(np.float64) < m, np.nextafter(m32, np.float32(np.inf)), m32)
    return np.where(ok, m32, -np.inf).astype(np.float64)


def _second_smallest(keys):
    return np.partition(keys, 1, axis=1)[:, 1]


def final_lists(A, B, c):
    """per query the rows with s' <= s'_(2) + margin: what the two-pass form lists and what the fused
    form's recheck keeps.  A query without a margin (rescanned exactly) lists every row."""
    keys = prefilter_keys(A, B)
    m = margin(A, B, c)
    with np.errstate(invalid="ignore"):
        thr = _second_smallest(keys) + m
        inside = keys <= thr[:, None]
    every = np.arange(keys.shape[1])
    return [np.flatnonzero(inside[q]) if np.isfinite(m[q]) else every for q in range(keys.shape[0])]


def knn2_u8_parts(nA, nB, nCU, qPerBlock=0, tileRows=0):
    """csrc/fm3d_match.hip knn2_u8_parts (without its tuning-only environment override)"""
    qb = qPerBlock if qPerBlock > 0 else K_Q
    tr = tileRows if tileRows > 0 else K_T
    nBlk = (nA + qb - 1) // qb
    nTiles = (nB + tr - 1) // tr
    if nBlk <= 0 or nCU <= 0:
        return 1
    if nBlk >= nCU:
        if qPerBlock <= 0:
            return 1
        best, bestCost = 1, 0
        for p in range(1, 17):
            if p > 1 and nTiles // p < 4:
                break
            cost = ((nBlk * p + nCU - 1) // nCU) * ((nTiles + p - 1) // p)
            if p == 1 or cost < bestCost:
                best, bestCost = p, cost
        return best
    p = min(16, (4 * nCU + nBlk - 1) // nBlk)
    while p > 1 and nTiles // p < 4:
        p -= 1
    return p


def part_tiles(nA, nB, nCU=256):
    """(parts, tilesPerPart) of launch_knn2_f32_mfma"""
    parts = knn2_u8_parts(nA, nB, nCU, 0, 0)
    nTiles = (nB + K_T - 1) // K_T
    return parts, ((nTiles + parts - 1) // parts if parts > 1 else max(nTiles, 1))


def row_half(rows):
    """the half-wave (lane >> 5) that ranks a train row: the MFMA's accumulator layout"""
    return ((np.asarray(rows) % 32) // 4) % 2


def row_part(rows, nA, nB, nCU=256):
    return (np.asarray(rows) // K_T) // part_tiles(nA, nB, nCU)[1]


def fused_list_lengths(A, B, c, nCU=256):
    """the fused pass's per-query candidate count (knn2_bf16_kernel MODE 2): a lane holds one half of
    each 32-row block, updates its running two smallest with a row's key v and emits the row when
    v <= p2 + margin; it restarts in every train part.  Rows past nB rank as +inf (and are emitted
    while p2 is still +inf, as in the kernel).  A query without a margin holds kCandMax2 + 1."""
    keys = prefilter_keys(A, B)
    nA, nB = keys.shape
    m = margin(A, B, c)
    _, tilesPerPart = part_tiles(nA, nB, nCU)
    nPad = (nB + K_T - 1) // K_T * K_T
    padded = np.full((nA, nPad), np.inf)
    padded[:, :nB] = keys
    rows = np.arange(nPad)
    part, half = (rows // K_T) // tilesPerPart, row_half(rows)
    count = np.zeros(nA, dtype=np.int64)
    with np.errstate(invalid="ignore"):
        for p in range(part.max() + 1):
            for h in (0, 1):
                p1 = np.full(nA, np.inf)
                p2 = np.full(nA, np.inf)
                for j in np.flatnonzero((part == p) & (half == h)):
                    v = padded[:, j]
                    p2 = np.minimum(np.maximum(p1, v), p2)  # v_med3_f32(p1, p2, v) with p1 <= p2
                    p1 = np.minimum(p1, v)
                    count += v <= p2 + m
    return np.where(np.isfinite(m), count, K_CAND_MAX2 + 1)


# ---------------------------------------------------------------- inputs
def _directions(rng, n, dim, rank=None):
    """unit rows of random direction; with a rank, inside a random subspace of that dimension (keys
    spread more against the margin, as descriptors of real images do)"""
    d = rng.normal(0, 1, (n, dim))
    if rank:
        d = rng.normal(0, 1, (n, rank)) @ np.linalg.qr(rng.normal(0, 1, (dim, rank)))[0].T
    return d / np.linalg.norm(d, axis=1, keepdims=True)


def adversarial_rows(nA, nB, K, nCU=256):
    """where the K triples (b*, decoy, decoy) stand among the train rows: row 0 of tile 0, the last two
    rows of the last (partial) tile, different 32-row blocks of one tile, different train parts, both
    half-waves; the rest spread over the tiles.  Distinct rows, every decoy pair in index order."""
    assert K >= 3 and nB >= 3 * K + 2 * K_T and nB % K_T >= 2
    _, tpp = part_tiles(nA, nB, nCU)
    last = (nB - 1) // K_T * K_T                      # first row of the last tile
    mid = (last // K_T // 2) * K_T                    # a tile in the middle
    out = [(0, nB - 2, nB - 1),                       # row 0 of tile 0; the last two rows
           (mid + 1, mid + 32 + 4, mid + 96 + 31),    # one tile, three 32-row blocks, both halves
           (K_T + 7, tpp * K_T + 64, last - 3)]       # three train parts (when the call has them)
    used = {r for t in out for r in t}
    step = (nB - 64) // (3 * (K - 3)) if K > 3 else 0
    r = 33
    for _ in range(K - 3):
        t = []
        while len(t) < 3:
            if r not in used:
                t.append(r)
                used.add(r)
                r += step
            else:
                r += 1
        out.append(tuple(t))
    rows = np.array(out, dtype=np.int64)
    rows[:, 1:] = np.sort(rows[:, 1:], axis=1)
    assert len(np.unique(rows)) == 3 * K and rows.max() < nB
    return rows


def correlated_rounding_case(dim, nA, nB, K, seed):
    """Ordinary rows plus K triples whose bf16 rounding errors all push the same way.  With h = dim / 2,
    x = 1 + 2^-8 - 2^-12 (rounds down to 1) and y = 1 + 2^-8 + 2^-12 (rounds up to 1 + 2^-7):
        query  a  = (x .. x | y .. y)
        b*        = (x .. x | 0 .. 0)                      the exact nearest row
        2 decoys  = (0 .. 0 | p .. p), p = 1 + k 2^-7 + 2^-8 + 2^-12 (rounds up), k = 5 + (i mod 6)
    each triple under its own +-1 signs and element permutation, so triples do not see each other.
    Filler rows have norms in [0.25, 0.9] sqrt(h): the special rows set B_max.  Returns A, B, the K
    query indices and the (K, 3) rows (b*, lower decoy, upper decoy)."""
    rng = np.random.default_rng(seed)
    h = dim // 2
    n = max(nA, nB)
    fill = _directions(rng, n, dim) * rng.uniform(0.25, 0.9, (n, 1)) * np.sqrt(h)
    B = fill[:nB].astype(np.float32)
    A = (fill[:nA] + rng.normal(0, 0.02, (nA, dim))).astype(np.float32)
    rows = adversarial_rows(nA, nB, K)
    queries = np.sort(rng.choice(nA, K, replace=False))
    queries[0], queries[-1] = 0, nA - 1  # the first query of the first block, the last of the last
    x = np.float32(1 + 2.0 ** -8 - 2.0 ** -12)
    y = np.float32(1 + 2.0 ** -8 + 2.0 ** -12)
    for i in range(K):
        p = np.float32(1 + (5 + i % 6) * 2.0 ** -7 + 2.0 ** -8 + 2.0 ** -12)
        sign = rng.choice(np.array([-1, 1], dtype=np.float32), dim)
        perm = rng.permutation(dim)
        a = np.concatenate([np.full(h, x), np.full(h, y)]).astype(np.float32)
        bs = np.concatenate([np.full(h, x), np.zeros(h)]).astype(np.float32)
        dc = np.concatenate([np.zeros(h), np.full(h, p)]).astype(np.float32)
        A[queries[i]] = (a * sign)[perm]
        B[rows[i, 0]] = (bs * sign)[perm]
        B[rows[i, 1]] = B[rows[i, 2]] = (dc * sign)[perm]
    return A, B, queries, rows


def aligned_case(dim, above, seed):
    """a parallel to b (here a == b), every element a float next to a bf16 tie -- just below it (rounds
    down by almost 2^-8 relative to the bf16 value) or just above it -- under random signs and powers of
    two: the rounding errors of all dim products add up.  One query, one row."""
    rng = np.random.default_rng(seed)
    tie = np.float32(1 + 2.0 ** -8)
    v = np.nextafter(tie, np.float32(2 if above else 0), dtype=np.float32)
    row = v * np.exp2(rng.integers(-6, 7, dim)).astype(np.float32) * rng.choice(np.array([-1, 1], dtype=np.float32), dim)
    return row[None, :].copy(), row[None, :].copy()


def retry_route_case(dim, nA, nB, seed):
    """Train rows of random direction with |b_j|^2 = 1 - j * 1e-4, strictly decreasing by more than the
    margin of a tiny query (6.1e-5 B_max^2); the first nA / 4 queries have norm 1e-6 -- far above the
    1e-10 rescan threshold, which tests |a| + B_max -- so their keys are |b_j|^2 to within 2e-6: every
    row is a running best and the fused lists overflow, while the final lists hold two rows.  The
    other queries are train rows plus noise."""
    rng = np.random.default_rng(seed)
    B = (_directions(rng, nB, dim) * np.sqrt(1.0 - 1e-4 * np.arange(nB))[:, None]).astype(np.float32)
    nTiny = (nA + 3) // 4
    A = np.empty((nA, dim), dtype=np.float32)
    A[:nTiny] = (_directions(rng, nTiny, dim) * 1e-6).astype(np.float32)
    src = rng.integers(0, nB, nA - nTiny)
    A[nTiny:] = (B[src] + rng.normal(0, 0.02, (nA - nTiny, dim))).astype(np.float32)
    return A, B, nTiny


def duplicates_case(dim, nA, nB, share, seed, groups=4, copies=140):
    """nA // share queries stand next to one of `groups` train rows that each occur `copies` times, the
    copies scattered over all tiles and parts: those queries' lists overflow in both forms.  The other
    queries are unduplicated train rows plus noise.  Returns A, B, the overflowing queries, and per
    such query the two lowest copies of its row (the exact top-2: equal distances, lowest index first)."""
    rng = np.random.default_rng(seed)
    B = _directions(rng, nB, dim, rank=16).astype(np.float32)
    spots = rng.permutation(nB)[: groups * copies].reshape(groups, copies)
    spots.sort(axis=1)
    B[spots.ravel()] = np.repeat(_directions(rng, groups, dim), copies, axis=0)  # outside the others' subspace
    plain = np.setdiff1d(np.arange(nB), spots.ravel())
    nDup = nA // share
    A = (B[rng.choice(plain, nA)] + rng.normal(0, 0.02, (nA, dim))).astype(np.float32)
    dupq = np.sort(rng.choice(nA, nDup, replace=False))
    grp = rng.integers(0, groups, nDup)
    A[dupq] = (B[spots[grp, 0]] + rng.normal(0, 0.005, (nDup, dim))).astype(np.float32)
    return A, B, dupq, spots[grp, :2]


def magnitude_cases(dim, nA, nB, seed):
    """{name: (A, B)}: one ordinary problem (unit train rows, queries next to them) at the magnitudes
    where the prefilter's bound stops covering it"""
    rng = np.random.default_rng(seed)
    B = _directions(rng, nB, dim).astype(np.float32)
    A = (B[rng.integers(0, nB, nA)] + rng.normal(0, 0.02, (nA, dim))).astype(np.float32)
    out = {"tiny": (A * np.float32(1e-12), B * np.float32(1e-12)),      # |a| + B_max < 1e-10: every query rescanned
           "large": (A * np.float32(1e15), B * np.float32(1e15))}      # still inside the bound's range
    A2 = A.copy()
    A2[5] = B[9] * np.float32(2e19)    # |a|^2 overflows fp32: no finite distance
    A2[700] = B[11] * np.float32(2e18)  # |a| >= 1e18 with a finite norm: rescanned, finite distances
    out["huge_query"] = (A2, B)
    B2 = B.copy()
    B2[1234] *= np.float32(1e6)        # B_max is an outlier's: the margin swallows every row
    out["outlier_row"] = (A, B2)
    B3 = B.copy()
    B3[77, 3] = np.float32(3.4e38)     # finite in fp32, +inf in bf16 (and |b|^2 overflows)
    out["bf16_inf"] = (A, B3)
    return out
