"""The matcher at every row width, tail and key extreme on every route (DESIGN.md §3.1's table):
both neighbours of knn_match and compareWithNNDR against the oracle, bit for bit, for byte rows of
1 .. 256 columns, binary rows of 1 .. 64 bytes, float rows whose width is no multiple of four and
integer-valued float rows that the packer hands to the byte kernel -- on ragged single tiles, a second
query block row, a partial last tile, and a split train set per kernel family; the packer's flag for
one bad element anywhere; NNDR's rule at epsilon 0, 1, 1e300, -1, +inf and NaN.

The oracle is itself pinned at these widths on the CPU (test_match_widths_oracle.py); the inputs and
what each case checks on them before the GPU is compared are tests/match_widths_cases.py's."""
import numpy as np
import pytest

import match_widths_cases as mw
from conftest import oracle_threads
from test_cross_check import assert_matches, mutual_ref, two_way
from test_guided_match import WIDTH, assert_knn, assert_nndr, keypoints, make_ctx

pytestmark = pytest.mark.gpu

BASE = [(1, 2), (2, 1), (33, 129), (130, 257)]
PARTS3 = {"FM3D_I8_PARTS": "3"}  # read on every call: three parts of train tiles on the int8-MFMA kernels
SCAN_SPLIT = (33, 4099)  # knn2_parts: two parts of 2050 rows wherever the device has two CUs


def route_cases():
    """(kind, width, shape, environment)"""
    out = []
    for w in mw.WIDTHS["u8"]:
        out += [("u8", w, s, {}) for s in BASE] + [("u8", w, (33, 700), PARTS3)]
        if w > 128:  # 128-row tiles: every part a single tile, the last one partial
            out.append(("u8", w, (33, 300), PARTS3))
    for w in mw.WIDTHS["bits"]:
        if (w + 3) // 4 == 8:  # padded to 32 bytes: the int8-MFMA kernel, or the popcount scan when switched off
            out += [("bits", w, s, {"FM3D_BITS_MFMA": "1"}) for s in BASE]
            out += [("bits", w, (33, 700), {"FM3D_BITS_MFMA": "1", **PARTS3}),
                    ("bits", w, (33, 300), {"FM3D_BITS_MFMA": "1", **PARTS3})]
            out += [("bits", w, s, {"FM3D_BITS_MFMA": "0"}) for s in BASE + [SCAN_SPLIT]]
        else:
            out += [("bits", w, s, {}) for s in BASE + [SCAN_SPLIT]]
    for w in mw.WIDTHS["f32"]:
        out += [("f32", w, s, {}) for s in BASE]
    out.append(("f32", 5, SCAN_SPLIT, {}))  # the generic scan has no parts: one long scan with a tail
    for w in (64, 128):  # the packed-f32 scalar-operand scan, whole and in two parts
        out += [("f32", w, (33, 129), {}), ("f32", w, SCAN_SPLIT, {})]
    for w in mw.WIDTHS["f32int"]:
        out += [("f32int", w, s, {}) for s in BASE] + [("f32int", w, (33, 700), PARTS3)]
        if w > 128:
            out.append(("f32int", w, (33, 300), PARTS3))
    for w in (257, 300):  # wider than the byte kernel takes: they stay on the float scan
        out += [("f32int", w, (33, 129), {}), ("f32int", w, (130, 257), {})]
    return out


def case_id(v):
    kind, width, shape, env = v
    tag = "".join(f"-{k[5:].lower()}{x}" for k, x in sorted(env.items()))
    return f"{kind}-{width}-{shape[0]}x{shape[1]}{tag}"


@pytest.fixture(scope="module")
def ctx(fm3d, synth):
    c = make_ctx(fm3d, synth.Camera.reference(WIDTH), synth.reference_g12())
    yield c
    c.close()


_REFS = {}


def reference(orc, kind, width, shape):
    """the case, the oracle's lists for it, checked once for what the case is there for, then shared"""
    key = (kind, width, shape)
    if key not in _REFS:
        c = mw.make_case(kind, width, *shape)
        idx, dist = orc.knn2(c.a, c.b, c.typ, oracle_threads())
        mw.check_case(c, idx, dist, lambda a, b: orc.knn2(a, b, c.typ, 1))
        for x in (c.a, c.b, idx, dist):
            x.setflags(write=False)
        _REFS[key] = (c, idx, dist)
    return _REFS[key]


def set_env(monkeypatch, env):
    for k in ("FM3D_I8_PARTS", "FM3D_BITS_MFMA"):
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)


# ---------------------------------------------------------------- 1. widths x routes x shapes
@pytest.mark.parametrize("case", route_cases(), ids=case_id)
def test_widths_routes_shapes(fm3d, orc, ctx, monkeypatch, case):
    kind, width, shape, env = case
    set_env(monkeypatch, env)
    c, idx, dist = reference(orc, kind, width, shape)
    dm = fm3d.DescriptorsMatcher(ctx, binary=c.binary)
    assert_knn(dm.knn_match(c.a, c.b), idx, dist)
    for eps in (1.0, 0.98):
        assert_nndr(orc, dm.compareWithNNDR(eps, c.a, c.b), idx, dist, eps)
    if "FM3D_I8_PARTS" in env:  # the parts' lists merged inside the fused NNDR launch
        fwd, rev = (idx, dist), orc.knn2(c.b, c.a, c.typ, oracle_threads())
        assert_matches(dm.compareWithNNDRMutual(1.0, c.a, c.b, mode=1), mutual_ref(orc, fwd, rev, 1.0, 1))


@pytest.mark.parametrize("kind,width", [(k, w) for k in ("u8", "bits", "f32int") for w in mw.WIDTHS[k]],
                         ids=lambda v: str(v))
def test_extreme_pair_alone(fm3d, orc, ctx, monkeypatch, kind, width):
    """all-0 and all-255 (all-0xFF) rows against each other with nothing else in the way: both ends of
    the packed key's range come out as distances"""
    set_env(monkeypatch, {})
    c = mw.make_case(kind, width, 2, 2)
    idx, dist = orc.knn2(c.a, c.b, c.typ, 1)
    far = mw.far_distance(kind, width)
    assert idx.tolist() == [[0, 1], [1, 0]] and dist.tolist() == [[0.0, far], [0.0, far]]
    assert_knn(fm3d.DescriptorsMatcher(ctx, binary=c.binary).knn_match(c.a, c.b), idx, dist)


# ---------------------------------------------------------------- 2. refusals
def code_of(fm3d, call):
    try:
        call()
    except fm3d.Fm3dError as e:
        return e.code
    return fm3d.FM3D_OK


@pytest.mark.parametrize("kind,width,code", [("u8", 257, "ERR_UNSUPPORTED"), ("bits", 65, "ERR_UNSUPPORTED"),
                                             ("u8", 0, "ERR_INVALID"), ("bits", 0, "ERR_INVALID"),
                                             ("f32", 0, "ERR_INVALID")])
def test_refused_widths(fm3d, orc, ctx, kind, width, code):
    typ, binary, alpha, _, _ = mw.FAMILIES[kind]
    a, b = np.zeros((4, width), dtype=alpha.dtype), np.zeros((6, width), dtype=alpha.dtype)
    k1, k2 = keypoints(4, 6)
    dm = fm3d.DescriptorsMatcher(ctx, binary=binary)
    want = getattr(fm3d, code)
    calls = [lambda: dm.knn_match(a, b), lambda: dm.compareWithNNDR(0.6, a, b),
             lambda: dm.knn_match_guided(a, b, k1, k2, 8.0), lambda: dm.compareWithNNDRGuided(0.6, a, b, k1, k2, 8.0),
             lambda: dm.compareWithNNDRMutual(0.6, a, b, mode=1), lambda: dm.compareWithNNDRMutual(0.6, a, b, mode=2),
             lambda: dm.compareWithNNDRMutualGuided(0.6, a, b, k1, k2, 8.0, mode=1)]
    for i, call in enumerate(calls):
        assert code_of(fm3d, call) == want, i
    c, idx, dist = reference(orc, kind, 5, (33, 129))  # the context still works
    assert_knn(dm.knn_match(c.a, c.b), idx, dist)


# ---------------------------------------------------------------- 3. the packer's flag
BAD_VALUES = [0.5, 255.5, 256.0, -1.0, mw.NAN, mw.INF, 1e10, -0.0]


@pytest.mark.parametrize("value", BAD_VALUES, ids=lambda v: repr(v))
@pytest.mark.parametrize("width", [5, 36, 129, 256])
def test_packer_flag_one_element(fm3d, orc, ctx, monkeypatch, width, value):
    """integer-valued float rows with exactly one element that is no integer in [0, 255]: a missed flag
    packs it as 0 and the distances change, so whatever the route the result is the float oracle's on
    the same rows.  (-0.0 is an integer: either route is legal, the result is the same.)"""
    set_env(monkeypatch, {})
    base, idx0, _ = reference(orc, "f32int", width, (33, 129))
    dm = fm3d.DescriptorsMatcher(ctx)
    places = [("a", 0, 0), ("a", -1, -1), ("b", 0, 0), ("b", -1, -1)]
    if width % 4:  # the last real column of a row whose 4-byte group straddles the width (a row that ranks)
        places += [("a", 17, width - 1), ("b", int(idx0[20, 0]), width - 1)]
    for side, row, col in places:
        a, b = base.a.copy(), base.b.copy()
        (a if side == "a" else b)[row, col] = value
        idx, dist = orc.knn2(a, b, orc.F32, oracle_threads())
        if value != 0 and (row, col) == (0, 0):
            # packed as 0 the element would show in the result: the all-0 rows are each other's nearest
            # at distance 0.  (Elsewhere it need not: half a unit drowns in a float sum of 256 squares.)
            (a if side == "a" else b)[row, col] = 0
            missed = orc.knn2(a, b, orc.F32, oracle_threads())
            assert not (np.array_equal(idx, missed[0]) and np.array_equal(dist, missed[1])), side
            (a if side == "a" else b)[row, col] = value
        assert_knn(dm.knn_match(a, b), idx, dist)
        assert_nndr(orc, dm.compareWithNNDR(0.98, a, b), idx, dist, 0.98)


# ---------------------------------------------------------------- 4. NNDR's rule at its edges
@pytest.mark.parametrize("kind,width", [("u8", 128), ("bits", 32), ("f32", 36)], ids=lambda v: str(v))
def test_nndr_edges(fm3d, orc, ctx, monkeypatch, kind, width):
    set_env(monkeypatch, {})
    c, idx, dist = reference(orc, kind, width, (130, 257))
    # d1 = 0 with d2 = 0 and with d2 > 0 both occur: 0 <= 0, 0 <= eps * d2 and inf * 0 all get decided
    assert (dist[c.copies, 0] == 0).sum() == 20 and (dist[c.copies, 1] == 0).any() and (dist[c.copies, 1] > 0).any()
    dm = fm3d.DescriptorsMatcher(ctx, binary=c.binary)
    counts = {}
    for eps in mw.EPS_EDGES:
        out = dm.compareWithNNDR(eps, c.a, c.b)
        assert_nndr(orc, out, idx, dist, eps)
        counts[repr(eps)] = len(out)
    zeros, both = int((dist[:, 0] == 0).sum()), int((dist[:, 1] == 0).sum())
    assert counts == {"0.0": zeros, "1.0": 130, "1e+300": 130, "-1.0": both, "inf": 130 - both, "nan": 0}
    assert 0 < both < zeros < 130
    k1, k2 = keypoints(130, 257)
    fwd, rev = two_way(orc, c.a, c.b, c.typ)
    for eps in (0.0, 1.0, 1e300):
        for mode in (1, 2):
            assert_matches(dm.compareWithNNDRMutual(eps, c.a, c.b, mode=mode), mutual_ref(orc, fwd, rev, eps, mode))
        assert_nndr(orc, dm.compareWithNNDRGuided(eps, c.a, c.b, k1, k2, 1e9), idx, dist, eps)
