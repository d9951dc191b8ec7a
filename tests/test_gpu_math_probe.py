"""The shared math headers on the device, on inputs of the suite's own choosing (fm3d_math_probe,
csrc/fm3d_probe.hip): include/fm3d_crmath.h, fm3d_detmath.h and fm3d_cvmath.h as hipcc
builds them for gfx950 against the host build the oracle uses (orc_math_eval) and against mpmath,
csrc/fm3d_fastdiv.h against the IEEE quotient (numpy's), and the plain / and sqrt of both widths
against numpy's (they pin -fhip-fp32-correctly-rounded-divide-sqrt and the fp64 expansions).

Every comparison is on the bit patterns (int64 views of the doubles, int32 views of the floats), a
NaN matching any NaN.  The input sets are tests/math_cases.py's, shared with tests/test_crmath.py."""
import numpy as np
import pytest

import math_cases

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def probe(fm3d):
    s = fm3d.Settings.default()
    s.pixelsRay = 8
    ctx = fm3d.Context(s)

    def run(fn, x, y=None):
        return fm3d.math_probe(ctx, fn, x, y)

    run.ctx = ctx
    yield run
    ctx.close()


def _same(a, b):
    return (a.view(np.int64) == b.view(np.int64)) | (np.isnan(a) & np.isnan(b))


def _same32(a, b):
    """doubles holding floats: compared as floats, on the int32 views"""
    a32, b32 = a.astype(np.float32), b.astype(np.float32)
    assert (np.isnan(a) | (a32.astype(np.float64) == a)).all(), "the device returned a double that is no float"
    return (a32.view(np.int32) == b32.view(np.int32)) | (np.isnan(a32) & np.isnan(b32))


def _assert_same(got, ref, *inputs, same=_same):
    bad = np.flatnonzero(~same(got, ref))
    assert bad.size == 0, (bad.size, [tuple(float(v[i]).hex() for v in inputs) + (float(got[i]).hex(), float(ref[i]).hex())
                                      for i in bad[:5]])


def _crmath_sets():
    """per function (probe name, oracle name, x, y): the sets test_crmath.py pins the host build on,
    plus the arguments beyond the double-double ranges and the special values"""
    ang = np.concatenate([math_cases.angles(np.random.default_rng(1), 3000), math_cases.angles_beyond()])
    ay, ax = math_cases.atan2_pairs()
    ey, ex = math_cases.atan2_extremes()
    sy = np.array([np.inf, -np.inf, np.inf, 1.0, -1.0, np.nan, 1.0, 0.0, -0.0, 0.0, -0.0, 5e-324])
    sx = np.array([np.inf, -np.inf, 1.0, np.inf, -np.inf, 1.0, np.nan, -1.0, -1.0, 5e-324, -5e-324, -0.0])
    aty, atx = np.concatenate([ay, ey, sy]), np.concatenate([ax, ex, sx])
    e = np.concatenate([math_cases.exp_args(), math_cases.exp_beyond()])
    hx, hy, _ = math_cases.hypot_pairs()
    qx, qy = math_cases.hypot_specials()
    hx, hy = np.concatenate([hx, qx]), np.concatenate([hy, qy])
    return ang, (aty, atx), e, (hx, hy)


def test_crmath_detmath_device_equals_host(probe, orc):
    """fm3d_crmath.h and fm3d_detmath.h: the device build returns the host build's bits -- signed
    zeros, subnormals (arguments and results: exp's ldexp below 2^-1022), infinities, NaN, the
    arguments at and beyond 2^19 and the atan2 operands at every magnitude included"""
    ang, (aty, atx), e, (hx, hy) = _crmath_sets()
    one = orc.DETMATH | orc.DET_1ULP
    for name, ofn, mode, x, y in (
            ("sin_cr", "sin", orc.DETMATH, ang, None), ("cos_cr", "cos", orc.DETMATH, ang, None),
            ("sincos_sel_cr0", "sincos_sel0", orc.DETMATH, ang, None),
            ("sincos_sel_cr1", "sincos_sel1", orc.DETMATH, ang, None),
            ("atan2_cr", "atan2", orc.DETMATH, aty, atx), ("exp_cr", "exp", orc.DETMATH, e, None),
            ("hypot_cr", "hypot", orc.DETMATH, hx, hy),
            ("sin", "sin", one, ang, None), ("cos", "cos", one, ang, None), ("atan2", "atan2", one, aty, atx),
            ("exp", "exp", one, e, None), ("acos", "acos", orc.DETMATH, math_cases.acos_args(), None)):
        got = probe(name, x, y)
        ref = orc.math_eval(ofn, x, y, mode=mode)
        bad = np.flatnonzero(~_same(got, ref))
        assert bad.size == 0, (name, bad.size, [(float(x[i]).hex(), None if y is None else float(y[i]).hex(),
                                                 float(got[i]).hex(), float(ref[i]).hex()) for i in bad[:5]])


def test_crmath_device_correctly_rounded(probe):
    """fm3d_crmath.h on the device against mpmath, on the inputs test_crmath.py asserts it on for the
    host: every result mpmath's value rounded to nearest (hypot_cr pins the device's double sqrt and
    / on the way)"""
    x = math_cases.angles(np.random.default_rng(1), 3000)
    for name, fn in (("sin_cr", "sin"), ("cos_cr", "cos"), ("sincos_sel_cr0", "sin"), ("sincos_sel_cr1", "cos")):
        got, ref = probe(name, x), math_cases.ref_mpmath(fn, x)
        bad = math_cases.mismatch(got, ref)
        assert bad.size == 0, (name, [(x[i], got[i], ref[i]) for i in bad[:5]])
    x = math_cases.exp_args()
    bad = math_cases.mismatch(probe("exp_cr", x), math_cases.ref_mpmath("exp", x))
    assert bad.size == 0, [x[i] for i in bad[:5]]
    x, y, _ = math_cases.hypot_pairs()
    bad = math_cases.mismatch(probe("hypot_cr", x, y), math_cases.ref_mpmath("hypot", x, y))
    assert bad.size == 0, [(x[i], y[i]) for i in bad[:5]]


def test_atan2_cr_device_correctly_rounded(probe):
    """fm3d_atan2_cr on the device against mpmath: the LM's range and every finite magnitude (2^+-500,
    2^+-900, 2^996 .. 2^1023, 1e-300, subnormals; all quadrants, both orders), where an unscaled Dekker
    split overflows or its error terms go subnormal"""
    import math
    y, x = math_cases.atan2_pairs()
    got = probe("atan2_cr", y, x)
    ref = math_cases.ref_mpmath("atan2", y, x)
    axes = (x == 0) | (y == 0)
    ref[axes] = [math.atan2(a, b) for a, b in zip(y[axes], x[axes])]
    bad = math_cases.mismatch(got, ref)
    assert bad.size == 0, [(y[i], x[i], got[i], ref[i]) for i in bad[:5]]
    y, x = math_cases.atan2_extremes()
    got = probe("atan2_cr", y, x)
    bad = math_cases.atan2_extremes_bad(got, math_cases.atan2_extremes_ref(y, x))
    assert bad.size == 0, [(float(y[i]).hex(), float(x[i]).hex(), got[i]) for i in bad[:5]]
    assert (np.signbit(got) == np.signbit(y)).all()


def test_sincos_sel_equals_sin_and_cos_on_device(probe):
    """the LM kernel's fm3d_sincos_sel_cr(x, 0 / 1) returns fm3d_sin_cr's / fm3d_cos_cr's bits on the
    device too, the sign of sin(-0) and the arguments beyond 2^19 included"""
    x = np.concatenate([math_cases.angles(np.random.default_rng(1), 3000), math_cases.angles_beyond()])
    _assert_same(probe("sincos_sel_cr0", x), probe("sin_cr", x), x)
    _assert_same(probe("sincos_sel_cr1", x), probe("cos_cr", x), x)
    z = probe("sincos_sel_cr0", np.array([-0.0, 0.0]))
    assert np.signbit(z[0]) and not np.signbit(z[1]) and (z == 0).all()


def _div(a, d):
    with np.errstate(all="ignore"):
        return a / d


def _mdiv_inside(a, d):
    return (np.abs(d) > 1e-200) & (np.abs(d) < 1e200) & (np.abs(a) < 1e100)


def test_mdiv_markstein_cases(probe):
    """mdiv / mdiv_fast return the IEEE quotient where it lies next to a rounding midpoint (the only
    inputs on which their single Markstein correction can round wrongly; the uncorrected q0 = RN(a
    RN(1/d)) is wrong on about half of them)"""
    a, d = math_cases.markstein_cases()
    assert _mdiv_inside(a, d).all()
    ref = _div(a, d)
    _assert_same(probe("mdiv", a, d), ref, a, d)
    _assert_same(probe("mdiv_fast", a, d), ref, a, d)


def test_mdiv_guard_edges(probe):
    """mdiv over every ordered pair of the guard bounds of fm3d_fastdiv.h, their neighbours, zeros,
    subnormals, infinities, NaN and a few ordinary values; mdiv_fast on the pairs inside the guard.
    a = -0 is left out (the documented exception, asserted below)."""
    a, d = math_cases.edge_pairs()
    keep = ~((a == 0) & np.signbit(a))
    a, d = a[keep], d[keep]
    ref = _div(a, d)
    _assert_same(probe("mdiv", a, d), ref, a, d)
    ins = _mdiv_inside(a, d)
    assert ins.sum() > 500 and (~ins).sum() > 500
    _assert_same(probe("mdiv_fast", a[ins], d[ins]), ref[ins], a[ins], d[ins])
    # fm3d_fastdiv.h: "a = -0 with d > 0 gives +0 (IEEE: -0)"; with d < 0 both give +0
    z = probe("mdiv", np.array([-0.0, -0.0, -0.0]), np.array([3.0, 1e150, -3.0]))
    assert (z == 0).all() and not np.signbit(z).any()


@pytest.mark.parametrize("case", range(len(math_cases.wave_patterns())), ids=[c[0] for c in math_cases.wave_patterns()])
def test_mdiv_wave_patterns(probe, case):
    """the ballot branch: waves with exactly one lane outside the guard (first, last and the two
    middle lanes), waves entirely inside (the fast sequence alone) and entirely outside, and partial
    last waves (inactive lanes while a helper ballots)"""
    name, a, d, ins = math_cases.wave_patterns()[case]
    ref = _div(a, d)
    _assert_same(probe("mdiv", a, d), ref, a, d)
    if ins.any():
        _assert_same(probe("mdiv_fast", a[ins], d[ins]), ref[ins], a[ins], d[ins])


def _recip_inputs():
    rng = np.random.default_rng(25)
    n = 1 << 16
    z = np.ldexp(rng.uniform(1, 2, n), rng.integers(-1074, 1024, n)) * rng.choice([-1.0, 1.0], n)
    near = np.ldexp(rng.uniform(1, 2, n), rng.integers(-702, 702, n)) * rng.choice([-1.0, 1.0], n)
    # 1 / z next to a midpoint: z = 2^106 / M rounded, M odd in [2^53, 2^54)
    M = rng.integers(2 ** 52, 2 ** 53, 4096) * 2 + 1
    mid = (2.0 ** 53 / M.astype(np.float64)) * 2.0 ** rng.integers(-600, 600, 4096)
    return np.concatenate([z, near, mid, math_cases.guard_edges(), math_cases.ORDINARY])


def test_recip_z(probe):
    """recip_z = z ? 1 / z : 1 everywhere; recip_z_lo the same for |z| <= 2^700 (its caller's
    promise), waves with single lanes below 2^-700 included"""
    z = _recip_inputs()
    ref = np.where(z == 0, 1.0, _div(1.0, z))
    _assert_same(probe("recip_z", z), ref, z)
    lo = ~(np.abs(z) > 2.0 ** 700)  # NaN stays in
    assert ((np.abs(z) < 2.0 ** -700) & lo).sum() > 1000
    _assert_same(probe("recip_z_lo", z[lo]), ref[lo], z[lo])


def test_div_nn_contract(probe):
    """div_nn (mok = div_nn_ok(mm), |nn| <= 2^60): the IEEE quotient where |mm / nn| < 2^100, NaN or
    at least 2^100 in magnitude otherwise -- fm3d_fastdiv.h's contract, which is what makes the
    ray-plane point leave the bounding box exactly when the IEEE quotient's does"""
    mm, nn = math_cases.div_nn_pairs()
    ea, eb = math_cases.edge_pairs()
    keep = np.abs(eb) <= 2.0 ** 60  # the contract's denominators (zeros and subnormals included, NaN not)
    mm, nn = np.concatenate([mm, ea[keep]]), np.concatenate([nn, eb[keep]])
    ref = _div(mm, nn)
    first = np.abs(ref) < 2.0 ** 100
    assert first.mean() >= 0.9, first.mean()  # a condition on the inputs
    fast = (np.abs(mm) >= 2.0 ** -600) & (np.abs(mm) <= 2.0 ** 60)
    assert (fast & first).sum() > 30000 and (fast & ~first).sum() > 1000
    got = probe("div_nn", mm, nn)
    _assert_same(got[first], ref[first], mm[first], nn[first])
    rest = got[~first]
    ok = np.isnan(rest) | (np.abs(rest) >= 2.0 ** 100)
    assert ok.all(), [(float(mm[~first][i]).hex(), float(nn[~first][i]).hex(), rest[i]) for i in np.flatnonzero(~ok)[:5]]


def test_double_operators(probe):
    """the compiler's fp64 / and sqrt on the device are IEEE's (numpy's): 2^20 random operand pairs
    over the whole exponent range plus the subnormal and overflow edges"""
    a, b = math_cases.operator_operands()
    _assert_same(probe("div_f64", a, b), _div(a, b), a, b)
    with np.errstate(all="ignore"):
        ref = np.sqrt(a)
    _assert_same(probe("sqrt_f64", a), ref, a)


def test_float_operators(probe):
    """the fp32 / and sqrtf are correctly rounded, subnormal results included: what
    -fhip-fp32-correctly-rounded-divide-sqrt buys the SIFT / SURF / ORB kernels (without it the
    device's / is a 2.5-ulp reciprocal sequence)"""
    a, b = math_cases.operator_operands(single=True)
    a32, b32 = a.astype(np.float32), b.astype(np.float32)
    assert ((a32 == a) | np.isnan(a)).all()
    with np.errstate(all="ignore"):
        q, r = (a32 / b32).astype(np.float64), np.sqrt(a32).astype(np.float64)
    _assert_same(probe("div_f32", a, b), q, a, b, same=_same32)
    _assert_same(probe("sqrt_f32", a), r, a, same=_same32)


def test_cvmath_device_equals_host(probe, orc):
    """fm3d_cvmath.h (OpenCV's float exp, fastAtan2, cvRound, cvFloor, powf(2, y) stand-ins): the
    device build returns the host build's bits on every 4093rd float.

    Left out, because C leaves the conversion of an out-of-range or NaN value to int undefined and
    x86 (INT_MIN) and the GPU (saturation, 0 for NaN) differ by design: for the integer-valued
    functions the values whose rounded result does not fit an int32; for fm3d_cv_exp_sse NaN (its
    rounded scaled argument is converted); for fm3d_cv_exp2f |y| >= 2^31 (floor(y) is converted)."""
    v = math_cases.float_sweep()
    finite = np.isfinite(v)
    for name, x in (("cv_exp_sse", v[~np.isnan(v)]), ("cv_exp_scalar", v),
                    ("cv_exp2f", v[~(np.abs(v) >= 2.0 ** 31)])):
        assert x.size > 600000
        _assert_same(probe(name, x), orc.math_eval(name, x), x, same=_same32)
    y, x = math_cases.float_sweep_pairs()
    _assert_same(probe("cv_atan2_deg", y, x), orc.math_eval("cv_atan2_deg", y, x), y, x, same=_same32)
    fits = finite & (np.abs(v) < 2.0 ** 31 - 128)  # floats: the largest below 2^31 is 2^31 - 128
    ties = np.concatenate([np.arange(-1000, 1000) + 0.5, [2.0 ** 31 - 1.5, np.nextafter(2.0 ** 31 - 0.5, 0.0), -2.0 ** 31 + 0.5,
                                                          -2.0 ** 31 - 0.5, 2.0 ** 31 - 1, -2.0 ** 31, 0.49999999999999994]])
    for name, x, rnd in (("cv_roundf", v[fits], np.rint), ("cv_floorf", v[fits], np.floor),
                         ("cv_round", np.concatenate([v[fits], ties]), np.rint)):
        want = rnd(x)  # round half to even / floor: the value must fit an int32 (a condition on the inputs)
        assert ((want >= -2.0 ** 31) & (want <= 2.0 ** 31 - 1)).all()
        ref = orc.math_eval(name, x)
        assert (ref == want).all()
        _assert_same(probe(name, x), ref, x)
    assert probe("cv_round", np.array([0.5, 1.5, 2.5, -0.5])).tolist() == [0.0, 2.0, 2.0, -0.0]


def test_probe_rejects_bad_arguments(fm3d, probe):
    """fm3d_math_probe: FM3D_ERR_INVALID for an unknown function, n < 0 or a null array (y only where
    the function takes two arguments); n == 0 returns at once"""
    import ctypes
    import math
    ctx = probe.ctx
    L, h = fm3d.lib(), ctx.handle
    buf = (ctypes.c_double * 4)(1.0, 2.0, 3.0, 4.0)
    out = (ctypes.c_double * 4)()
    nfn = len(fm3d.PROBE_FNS)
    assert L.fm3d_math_probe(h, nfn, buf, buf, 4, out) == fm3d.ERR_INVALID
    assert L.fm3d_math_probe(h, -1, buf, buf, 4, out) == fm3d.ERR_INVALID
    assert L.fm3d_math_probe(h, 0, buf, buf, -1, out) == fm3d.ERR_INVALID
    assert L.fm3d_math_probe(h, 0, None, buf, 4, out) == fm3d.ERR_INVALID
    assert L.fm3d_math_probe(h, 0, buf, buf, 4, None) == fm3d.ERR_INVALID
    assert L.fm3d_math_probe(h, fm3d.PROBE_FNS.index("mdiv"), buf, None, 4, out) == fm3d.ERR_INVALID
    assert L.fm3d_math_probe(h, 0, buf, None, 0, out) == 0
    assert L.fm3d_math_probe(h, fm3d.PROBE_FNS.index("sqrt_f64"), buf, None, 4, out) == 0
    assert list(out) == [1.0, math.sqrt(2.0), math.sqrt(3.0), 2.0]
    assert fm3d.math_probe(ctx, "div_f64", np.zeros(0), np.zeros(0)).size == 0
    with pytest.raises(fm3d.Fm3dError):
        fm3d.math_probe(ctx, "no_such_function", np.zeros(1))
