"""The matcher's oracle pinned where nothing pinned it: orc.knn2 and orc.nndr against the plain numpy
restatements of tests/match_widths_cases.py, bit for bit, at every row width the GPU tests
(test_gpu_match_widths.py) lean on it for -- float rows whose width is no multiple of four (FLANN's
tail loop), byte rows of 1 .. 256 columns, binary rows of 1 .. 64 bytes -- and NNDR's rule at
epsilon 0, 1, 1e300, -1, +inf and NaN.  No GPU."""
import numpy as np
import pytest

import match_widths_cases as mw

SHAPES = [(1, 2), (7, 1), (33, 129)]
CASES = [(k, w) for k in mw.WIDTHS for w in mw.WIDTHS[k]] + [("f32", 64), ("f32", 128), ("f32int", 257), ("f32int", 300)]


def assert_same(got, ref):
    assert got[0].dtype == ref[0].dtype == np.int32 and got[1].dtype == ref[1].dtype == np.float32
    assert np.array_equal(got[0], ref[0])
    assert np.array_equal(got[1].view(np.uint32), ref[1].view(np.uint32))  # +inf where absent, on both sides


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
@pytest.mark.parametrize("kind,width", CASES, ids=lambda v: str(v))
def test_knn2_and_nndr(orc, kind, width, shape):
    c = mw.make_case(kind, width, *shape)
    idx, dist = orc.knn2(c.a, c.b, c.typ, 1)
    ref = mw.knn2_np(c.a, c.b, c.typ)
    mw.check_case(c, ref[0], ref[1], lambda a, b: mw.knn2_np(a, b, c.typ))
    assert_same((idx, dist), ref)
    for eps in mw.EPS_EDGES:
        q, t, d = orc.nndr(idx, dist, eps)
        rq, rt, rd = mw.nndr_np(idx, dist, eps)
        assert np.array_equal(q, rq) and np.array_equal(t, rt) and np.array_equal(d.view(np.uint32), rd.view(np.uint32)), eps
    if shape[1] >= 129:
        # the edges of the rule do something here: 0 keeps exactly the pairs at distance 0, +inf drops
        # exactly those whose second neighbour is at 0 (inf * 0 is NaN), -1 keeps the pairs whose two
        # neighbours are both at 0 (0 <= -0), NaN keeps nothing
        zero = set(np.flatnonzero(dist[:, 0] == 0).tolist())
        assert set(orc.nndr(idx, dist, 0.0)[0].tolist()) == zero and zero
        assert set(orc.nndr(idx, dist, mw.INF)[0].tolist()) == set(np.flatnonzero(dist[:, 1] > 0).tolist())
        assert len(orc.nndr(idx, dist, 1.0)[0]) == len(idx) == len(orc.nndr(idx, dist, 1e300)[0])
        assert set(orc.nndr(idx, dist, -1.0)[0].tolist()) == set(np.flatnonzero(dist[:, 1] == 0).tolist())
        assert len(orc.nndr(idx, dist, mw.NAN)[0]) == 0


@pytest.mark.parametrize("width", [1, 3, 5, 7, 63, 129])
def test_f32_tail_is_flann_order(orc, width):
    """random float rows, where the order of the additions shows in the last bit: the tail adds one
    square at a time after the groups of four.  Summing all squares left to right, or the tail as a
    group of its own, gives other bits for some pair where the forms differ at all (from the second
    group on; a tail of two or three after a group) -- so this test would see either"""
    rng = np.random.default_rng(width)
    a = rng.normal(0, 1, (40, width)).astype(np.float32)
    b = rng.normal(0, 1, (90, width)).astype(np.float32)
    assert_same(orc.knn2(a, b, orc.F32, 1), mw.knn2_np(a, b, orc.F32))
    keys = mw.keys_np(a, b, orc.F32)
    d = a[:, None, :] - b[None, :, :]
    sq = d * d
    zero = np.zeros(sq.shape[:2], dtype=np.float32)
    seq = zero
    for i in range(width):
        seq = seq + sq[:, :, i]
    assert (seq != keys).any() == (width >= 8)
    full = width - width % 4
    grouped, tail = zero, zero
    for g in range(0, full, 4):
        grouped = grouped + (((sq[:, :, g] + sq[:, :, g + 1]) + sq[:, :, g + 2]) + sq[:, :, g + 3])
    for i in range(full, width):
        tail = tail + sq[:, :, i]
    assert ((grouped + tail) != keys).any() == (width % 4 >= 2 and width >= 6)


SPECIALS = [0.5, 255.5, 256.0, -1.0, mw.NAN, mw.INF, 1e10, -0.0]


@pytest.mark.parametrize("value", SPECIALS, ids=lambda v: repr(v))
@pytest.mark.parametrize("width", [5, 36])
def test_f32_special_elements(orc, width, value):
    """one element of integer-valued float rows replaced: a NaN or +inf key never replaces, so the
    row never ranks (as a query: no neighbour at all)"""
    for side, pos in (("a", (0, 0)), ("a", (-1, -1)), ("b", (0, 0)), ("b", (-1, -1)), ("b", (40, width - 1))):
        c = mw.make_case("f32int", width, 33, 129)
        getattr(c, side)[pos] = value
        got = orc.knn2(c.a, c.b, orc.F32, 1)
        assert_same(got, mw.knn2_np(c.a, c.b, orc.F32))
        if value != value or value == mw.INF:
            if side == "a":
                assert tuple(got[0][pos[0]]) == (-1, -1)
            else:
                assert not (got[0] == pos[0] % 129).any()
