"""Inputs and plain numpy restatements for the matcher's width tests (test_match_widths_oracle.py on
the CPU, test_gpu_match_widths.py on the GPU).

The restatements are written to be read, not to be fast:
  u8    int64 squared differences, float32(sqrt(float32(d2))), order (d2, index)
  bits  popcount of xor (np.unpackbits), order (distance, index)
  f32   FLANN's L2<float> in float32: per group of four
        result += ((d0*d0 + d1*d1) + d2*d2) + d3*d3, every operation rounded to float32, then the
        tail result += d*d; a strictly smaller key replaces, so equal keys keep the lower index and a
        NaN or +inf key never ranks.

The rows of a case come from a four-value alphabet (test_cross_check.py's descriptors()), so equal
distances are everywhere; on top of them a case plants
  * the extremes: an all-0 and an all-255 (bits: all-0xFF) row at the head of both sides,
  * groups of two identical train rows, each group at one place where the kernels change hands (the
    same 32-row block, the other epilogue chain, the first row of the next tile or part, the last
    row), each with a query that copies them,
  * copies of other train rows on both sides (zero distances, tied seconds)."""
import numpy as np

F32, U8, BITS = 0, 1, 2
INF, NAN = float("inf"), float("nan")
EPS_EDGES = [0.0, 1.0, 1e300, -1.0, INF, NAN]

# kind -> (oracle type, binary, alphabet, the planted groups' first elements start here, has extremes)
FAMILIES = {
    "u8": (U8, False, np.array([100, 101, 102, 103], dtype=np.uint8), 110, True),
    "bits": (BITS, True, np.array([0x00, 0x01, 0x03, 0x07], dtype=np.uint8), 0x10, True),
    "f32": (F32, False, np.array([0.25, 0.5, 0.75, 1.0], dtype=np.float32), 1.25, False),
    "f32int": (F32, False, np.array([0, 1, 254, 255], dtype=np.float32), 100, True),
}
WIDTHS = {
    "u8": [1, 16, 64, 100, 127, 128, 129, 200, 255, 256],
    "bits": [1, 4, 15, 16, 17, 31, 32, 33, 48, 63, 64],
    "f32": [1, 3, 4, 5, 36, 63, 65, 127, 129, 301],
    "f32int": [5, 36, 100, 128, 129, 200, 255, 256],
}

# (source row, its copy): the copy's place is what the group is there for
#   6     the source's 32-row block, the other lane half of the int8 kernel's epilogue
#   36    the next 32-row block: the other epilogue chain
#   128   first row of the second 128-row tile (FM3D_I8_PARTS=3 at 300 rows: of part 1)
#   200   the upper half of a 256-row tile (the eighth row bit)
#   256   first row of the second 256-row tile / third 128-row tile (FM3D_I8_PARTS=3: of a part)
#   512   first row of part 2 at 700 rows in three parts
#   2050  first row of the scans' part 1 at 4099 rows
#   -1    the last row
GROUPS = [(3, 6), (4, 36), (5, 128), (8, 200), (9, 256), (10, 512), (11, 2050), (12, -1)]
HEAD = 13  # rows below it are the extremes and the groups' sources


# ---------------------------------------------------------------- restatements
def keys_np(a, b, typ):
    """(nA, nB) ranking keys: squared L2 as int64 (u8), Hamming as int64 (bits), FLANN's float32 L2"""
    if typ == U8:
        d = a.astype(np.int64)[:, None, :] - b.astype(np.int64)[None, :, :]
        return (d * d).sum(axis=2)
    if typ == BITS:
        x = a[:, None, :] ^ b[None, :, :]
        return np.unpackbits(x, axis=2).sum(axis=2).astype(np.int64)
    assert a.dtype == np.float32 and b.dtype == np.float32
    dim = a.shape[1]
    result = np.zeros((a.shape[0], b.shape[0]), dtype=np.float32)
    sq = lambda i: (a[:, None, i] - b[None, :, i]) * (a[:, None, i] - b[None, :, i])  # float32 throughout
    with np.errstate(all="ignore"):
        i = 0
        while i + 3 < dim:
            result = result + (((sq(i) + sq(i + 1)) + sq(i + 2)) + sq(i + 3))
            i += 4
        while i < dim:
            result = result + sq(i)
            i += 1
    assert result.dtype == np.float32
    return result


def knn2_np(a, b, typ):
    """the two nearest train rows of every query: (idx (nA, 2) int32, -1 where absent; dist (nA, 2)
    float32, +inf where absent)"""
    K = keys_np(a, b, typ)
    nA, nB = K.shape
    idx = np.full((nA, 2), -1, dtype=np.int32)
    key = np.full((nA, 2), np.inf, dtype=np.float32 if typ == F32 else np.float64)
    if typ == F32:  # the scan itself: NaN and +inf never replace
        for j in range(nB):
            k = K[:, j]
            first = k < key[:, 0]
            second = ~first & (k < key[:, 1])
            key[:, 1] = np.where(first, key[:, 0], np.where(second, k, key[:, 1]))
            idx[:, 1] = np.where(first, idx[:, 0], np.where(second, j, idx[:, 1]))
            key[:, 0] = np.where(first, k, key[:, 0])
            idx[:, 0] = np.where(first, j, idx[:, 0])
    else:  # order by (key, index)
        order = np.argsort(K, axis=1, kind="stable")[:, :2]
        n = order.shape[1]
        idx[:, :n] = order
        key[:, :n] = np.take_along_axis(K, order, axis=1)
    with np.errstate(all="ignore"):
        dist = key.astype(np.float32) if typ == BITS else np.sqrt(key.astype(np.float32))
    return idx, dist.astype(np.float32)


def nndr_np(idx, dist, eps):
    """compareWithNNDR's rule: two neighbours and (double)d1 <= eps * (double)d2 -> (q, t, d)"""
    with np.errstate(all="ignore"):
        keep = (idx[:, 0] >= 0) & (idx[:, 1] >= 0) & (dist[:, 0].astype(np.float64) <= eps * dist[:, 1].astype(np.float64))
    q = np.flatnonzero(keep).astype(np.int32)
    return q, idx[q, 0], dist[q, 0]


# ---------------------------------------------------------------- inputs
class Case:
    pass


def make_case(kind, width, nA, nB, seed=1):
    typ, binary, alpha, mark, extremes = FAMILIES[kind]
    rng = np.random.default_rng([seed, width, nA, nB])
    a = alpha[rng.integers(0, 4, (nA, width))]
    b = alpha[rng.integers(0, 4, (nB, width))]
    hi = np.float32(255) if typ == F32 else np.uint8(255)
    c = Case()
    c.kind, c.width, c.typ, c.binary, c.extremes = kind, width, typ, binary, extremes
    c.groups = []  # (query, source row, copy)
    c.copies = np.zeros(0, dtype=np.int64)  # queries that copy a train row
    if nB > HEAD + 1:
        # a quarter of the ordinary train rows copy another ordinary row: a query nearest to one of a
        # pair has two equal neighbours
        used = {s for s, _ in GROUPS} | {d if d >= 0 else nB - 1 for _, d in GROUPS} | {0, 1}
        free = np.array([j for j in range(nB) if j not in used and j >= HEAD])
        tgt = rng.choice(free, len(free) // 4, replace=False)
        src = rng.choice(np.setdiff1d(free, tgt), len(tgt))
        b[tgt] = b[src]
        taken = set()
        for g, (s, d) in enumerate(GROUPS):
            d = nB - 1 if d < 0 else d
            if d >= nB or d in taken or d < HEAD or 2 + g >= nA:
                continue
            taken.add(d)
            b[s, 0] = alpha.dtype.type(mark + (0.25 if kind == "f32" else 1) * g)  # like no other row
            b[d] = b[s]
            a[2 + g] = b[s]
            c.groups.append((2 + g, s, d))
        if nA >= 130:  # 20 queries that copy ordinary train rows: d1 = 0, and d2 = 0 where the row has a copy
            c.copies = np.arange(HEAD, HEAD + 20)
            a[c.copies] = b[np.concatenate([tgt[:10], rng.choice(free, 10, replace=False)])]
    if extremes:
        b[0] = 0
        a[0] = 0
        if nB > 1:
            b[1] = hi
        if nA > 1:
            a[1] = hi
    c.a, c.b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return c


def far_distance(kind, width):
    """the distance of an all-0 row to an all-255 / all-0xFF one, as a DMatch holds it"""
    if kind == "bits":
        return np.float32(8 * width)
    return np.sqrt(np.float32(width * 255 * 255))


def check_case(c, idx, dist, knn2):
    """what a case is there for, read from the reference's output (idx, dist) alone; knn2(a, b) is the
    reference for the one pair that no top-2 shows"""
    nA, nB = len(c.a), len(c.b)
    if nB >= 129:
        assert (dist[:, 0] == dist[:, 1]).sum() * 10 >= nA, "fewer than 10 % of the queries have tied neighbours"
        assert c.groups
    for q, s, d in c.groups:
        assert tuple(idx[q]) == (s, d) and dist[q, 0] == 0 and dist[q, 1] == 0, (q, s, d)
    if len(c.copies):
        assert np.all(dist[c.copies, 0] == 0) and np.any(dist[c.copies, 1] == 0)
    if c.extremes:
        assert idx[0, 0] == 0 and dist[0, 0] == 0
        if nB > 1 and c.width * 255 * 255 < 2 ** 24:  # (wider float rows: the float sum rounds)
            far = knn2(c.a[:1], c.b[1:2])[1][0, 0]
            assert far == far_distance(c.kind, c.width)
            if c.kind != "bits":
                assert abs(float(far) - np.sqrt(c.width) * 255) <= 2.0 ** -24 * float(far)
