"""include/fm3d_crmath.h -- the correctly rounded sin, cos, atan2 and exp of the LM kernel and of the
oracle's DETMATH mode -- pinned against mpmath at 200 bits, through the oracle's
orc_math_eval (the same header the GPU compiles).  CPU only.

Inputs: the ranges the LM feeds them (angles of a few radians, exponents of the LM's weights),
the reduction's hard cases (multiples of pi/2 rounded to double, the Cody-Waite range's end 2^19),
signed zeros, subnormals and the axes of atan2, and for atan2 every magnitude a finite double takes
(tests/math_cases.py holds the sets; tests/test_gpu_math_probe.py runs them through the device build).
Every result must be mpmath's value rounded to nearest; the 1-ulp polynomials (fm3d_detmath.h,
DET_1ULP; the NCC hypotheses) within one ulp."""
import math

import numpy as np
import pytest

import math_cases

mpmath = pytest.importorskip("mpmath")
mp = mpmath.mp


_ref = math_cases.ref_mpmath
_mismatch = math_cases.mismatch


@pytest.mark.parametrize("fn", ["sin", "cos"])
def test_sin_cos_correctly_rounded(orc, fn):
    x = math_cases.angles(np.random.default_rng(1), 3000)
    got = orc.math_eval(fn, x)
    ref = _ref(fn, x)
    bad = _mismatch(got, ref)
    assert bad.size == 0, [(x[i], got[i], ref[i]) for i in bad[:5]]
    if fn == "sin":  # odd: the sign of zero kept
        assert np.signbit(orc.math_eval(fn, np.array([-0.0]))[0])
    # the 1-ulp polynomials: within one ulp, and they differ from the correctly rounded results
    # somewhere (which is why the LM moved to these)
    one = orc.math_eval(fn, x, mode=orc.DETMATH | orc.DET_1ULP)
    sel = np.abs(x) < 2.0 ** 19
    ulp = np.spacing(np.abs(ref[sel]))
    assert (np.abs(one[sel] - ref[sel]) <= ulp).all()


def test_atan2_correctly_rounded(orc):
    y, x = math_cases.atan2_pairs()
    got = orc.math_eval("atan2", y, x)
    ref = _ref("atan2", y, x)
    axes = (x == 0) | (y == 0)  # signed zeros: IEEE's special values (exact in libm), not mpmath's
    ref[axes] = [math.atan2(a, b) for a, b in zip(y[axes], x[axes])]
    bad = _mismatch(got, ref)
    assert bad.size == 0, [(y[i], x[i], got[i], ref[i]) for i in bad[:5]]
    assert math.copysign(1.0, orc.math_eval("atan2", np.array([-0.0]), np.array([1.0]))[0]) == -1.0
    # every finite magnitude: operands beyond 2^+-500 are scaled before the double-double division
    # (from 2^997 on an unscaled Dekker split overflows to a NaN quotient, which must not index the table)
    y, x = math_cases.atan2_extremes()
    got = orc.math_eval("atan2", y, x)
    ref = math_cases.atan2_extremes_ref(y, x)
    bad = math_cases.atan2_extremes_bad(got, ref)
    assert bad.size == 0, [(float(y[i]).hex(), float(x[i]).hex(), got[i], ref[i]) for i in bad[:5]]
    assert (np.signbit(got) == np.signbit(y)).all()  # underflowed results keep y's sign


def test_sincos_sel_is_sin_and_cos(orc):
    """fm3d_sincos_sel_cr -- the only sin / cos form the LM kernel calls -- returns fm3d_sin_cr's bits
    with cosine 0 and fm3d_cos_cr's with cosine 1, the sign of sin(-0) and the arguments beyond 2^19
    (where all three hand over to fm3d_detmath.h) included"""
    x = np.concatenate([math_cases.angles(np.random.default_rng(1), 3000), math_cases.angles_beyond()])
    for sel, fn in (("sincos_sel0", "sin"), ("sincos_sel1", "cos")):
        a, b = orc.math_eval(sel, x), orc.math_eval(fn, x)
        same = (a.view(np.int64) == b.view(np.int64)) | (np.isnan(a) & np.isnan(b))
        assert same.all(), [(x[i], a[i], b[i]) for i in np.flatnonzero(~same)[:5]]
    assert np.signbit(orc.math_eval("sincos_sel0", np.array([-0.0]))[0])


def test_exp_correctly_rounded(orc):
    x = math_cases.exp_args()
    got = orc.math_eval("exp", x)
    ref = _ref("exp", x)
    bad = _mismatch(got, ref)
    assert bad.size == 0, [(x[i], got[i], ref[i]) for i in bad[:5]]


def test_libm_differs_somewhere(orc):
    """This image's glibc is not what the GPU computes: over random angles its sin or cos differs
    from the correctly rounded value on some inputs (or agrees everywhere -- then the STRICT and
    DETMATH modes coincide for these functions and tools/full_parity.py's attribution says so)."""
    x = np.random.default_rng(4).uniform(-4, 4, 20000)
    d = sum(int((orc.math_eval(f, x, mode=orc.STRICT) != orc.math_eval(f, x)).sum()) for f in ("sin", "cos"))
    print(f"libm sin/cos differ from the correctly rounded value on {d} of {2 * len(x)} inputs")


def test_hypot_correctly_rounded(orc):
    """fm3d_hypot_cr -- the rotation's hypot in OpenCV's JacobiSVDImpl_ (include/fm3d_cvsvd.h, the DLT
    and the polar factor) -- is mpmath's sqrt(x^2 + y^2) rounded to nearest, over random pairs of
    mixed magnitudes (the DLT's p and beta span many decades), equal pairs, zeros, the 2^-60 cut,
    scaled extremes and non-finite values; glibc's hypot here is not correctly rounded everywhere."""
    x, y, n = math_cases.hypot_pairs()
    got = orc.math_eval("hypot", x, y)
    ref = _ref("hypot", x, y)
    bad = _mismatch(got, ref)
    assert bad.size == 0, [(x[i], y[i], got[i], ref[i]) for i in bad[:5]]
    inf, nan = float("inf"), float("nan")
    sp = orc.math_eval("hypot", np.array([inf, nan, -inf, nan]), np.array([nan, inf, 1.0, 1.0]))
    assert sp[0] == inf and sp[1] == inf and sp[2] == inf and np.isnan(sp[3])
    libm = orc.math_eval("hypot", x[:n], y[:n], mode=orc.STRICT)
    print(f"libm hypot differs from the correctly rounded value on {int((libm != got[:n]).sum())} of {n} pairs")
