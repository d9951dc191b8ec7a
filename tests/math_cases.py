"""Input sets of the math tests, shared by tests/test_crmath.py (the host build of include/fm3d_crmath.h
against mpmath) and tests/test_gpu_math_probe.py (the device build of the shared headers against the
host build, mpmath and IEEE arithmetic).  Every set is a pure function of fixed seeds."""
from fractions import Fraction

import numpy as np

# ---------------------------------------------------------------- references (mpmath, 200+ bits)


def ref_mpmath(fn, x, y=None):
    """mpmath's sin / cos / exp of x, atan2(x, y) or hypot(x, y), rounded to the nearest double"""
    import mpmath
    if fn == "hypot":
        with mpmath.workprec(300):
            return np.array([float(mpmath.sqrt(mpmath.mpf(a) ** 2 + mpmath.mpf(b) ** 2)) for a, b in zip(x, y)])
    with mpmath.workprec(200):
        if fn == "sin":
            return np.array([float(mpmath.sin(mpmath.mpf(v))) for v in x])
        if fn == "cos":
            return np.array([float(mpmath.cos(mpmath.mpf(v))) for v in x])
        if fn == "exp":
            return np.array([float(mpmath.exp(mpmath.mpf(v))) for v in x])
        return np.array([float(mpmath.atan2(mpmath.mpf(a), mpmath.mpf(b))) for a, b in zip(x, y)])


def mismatch(got, ref):
    """indices where the bits differ (mpmath has no signed zero: a zero matches either zero)"""
    return np.flatnonzero((got.view(np.int64) != ref.view(np.int64)) & ~((got == 0) & (ref == 0)))


def _nearest_double(v):
    """an mpf rounded once to the nearest double, subnormals included (float() of an mpf rounds to 53
    bits first): through the exact rational"""
    sign, man, exp, _ = v._mpf_
    f = Fraction(int(man)) * (Fraction(2) ** exp)
    return float(-f if sign else f)


def atan2_extremes_ref(y, x):
    """mpmath's atan2 of atan2_extremes() at 400 bits (its exponent range is unbounded, so the
    subnormal quotients keep all of them), each rounded once to the nearest double"""
    import mpmath
    with mpmath.workprec(400):
        return np.array([_nearest_double(mpmath.atan2(mpmath.mpf(a), mpmath.mpf(b))) for a, b in zip(y, x)])


def atan2_extremes_bad(got, ref):
    """indices not correctly rounded; where the true value is subnormal the last subnormal bit is
    allowed (an exact tie of the quotient rounds to even, atan of it lies just below)"""
    sub = np.abs(ref) < 2.0 ** -1022
    return np.flatnonzero(np.where(sub, ~(np.abs(got - ref) <= 5e-324), got.view(np.int64) != ref.view(np.int64)))


# ---------------------------------------------------------------- fm3d_crmath.h / fm3d_detmath.h


def angles(rng, n):
    """sin / cos arguments: the LM's range, the whole double-double range (|x| < 2^19), multiples of
    pi/2 rounded to double and their neighbours, zeros, subnormals, the range's last doubles"""
    k = np.arange(-40, 41)
    hard = np.concatenate([k * (np.pi / 2), np.nextafter(k * (np.pi / 2), np.inf), np.nextafter(k * (np.pi / 2), -np.inf)])
    return np.concatenate([
        rng.uniform(-4, 4, n), rng.uniform(-100, 100, n // 4), rng.uniform(-2.0 ** 19, 2.0 ** 19, n // 8),
        hard, [0.0, -0.0, 5e-324, -5e-324, 1e-300, 2.0 ** -30, 0.5, 1.0, 2.0, np.pi, 2.0 ** 19 - 1],
        np.nextafter(np.float64(2.0 ** 19), 0.0) * np.array([1.0, -1.0])])


def angles_beyond():
    """sin / cos arguments at and beyond 2^19 (fm3d_detmath.h's functions take over: accurate for a
    while, meaningless far out, but the same bits on host and device), infinities and NaN"""
    rng = np.random.default_rng(11)
    e = rng.uniform(19, 1023, 400)
    big = np.ldexp(rng.uniform(1, 2, 400), e.astype(np.int64)) * rng.choice([-1.0, 1.0], 400)
    return np.concatenate([big, [2.0 ** 19, -2.0 ** 19, np.nextafter(2.0 ** 19, np.inf), 2.0 ** 20, 2.0 ** 52, 2.0 ** 53,
                                 1e22, 1e300, np.finfo(np.float64).max, -np.finfo(np.float64).max,
                                 np.inf, -np.inf, np.nan]])


def atan2_pairs():
    """(y, x): the LM's range (unit-scale components, small y, large x), the axes and signed zeros"""
    rng = np.random.default_rng(2)
    y = np.concatenate([rng.normal(size=3000), rng.normal(size=500) * 1e-8, [0.0, -0.0, 0.0, -0.0, 1.0, -1.0, 0.0, 5e-324],
                        rng.uniform(-1, 1, 500)])
    x = np.concatenate([rng.normal(size=3000), rng.normal(size=500), [0.0, 0.0, -0.0, -0.0, 0.0, 0.0, 1.0, -1.0],
                        rng.uniform(-1, 1, 500) * 1e6])
    return y, x


def atan2_extremes():
    """(y, x): every ordered pair of magnitudes at 2^+-500, 2^+-900, 2^996, 2^997 (where the Dekker
    split of an unscaled operand overflows), 2^1023, the largest double, 1e-300, the smallest normal,
    subnormals and 1, each also with a full mantissa, in all four quadrants"""
    m = [2.0 ** -500, 2.0 ** 500, 2.0 ** -900, 2.0 ** 900, 2.0 ** 996, 2.0 ** 997, 2.0 ** 1023, 1e-300,
         2.0 ** -1022, 5e-324, 2.0 ** -1040, 1.0]
    full = 1.0 + 0xB5C4A37E91D2F / 2.0 ** 52  # 1.71..., 52 fraction bits in use
    mags = np.array(m + [v * full for v in m if v * full < np.inf and v > 5e-324] +
                    [np.finfo(np.float64).max, 3e-310, np.nextafter(2.0 ** 500, np.inf), np.nextafter(2.0 ** -500, 0.0)])
    a, b = [g.ravel() for g in np.meshgrid(mags, mags, indexing="ij")]
    y = np.concatenate([a, -a, a, -a])
    x = np.concatenate([b, b, -b, -b])
    return y, x


def exp_args():
    rng = np.random.default_rng(3)
    return np.concatenate([rng.uniform(-40, 40, 3000), rng.uniform(-1e-3, 1e-3, 300), rng.uniform(-700, 700, 300),
                           [0.0, -0.0, 1.0, -1.0, 1e-300, -1e-300, 709.0, -700.0]])


def exp_beyond():
    """exp arguments whose results are subnormal (ldexp to a subnormal), overflow, or special"""
    rng = np.random.default_rng(12)
    return np.concatenate([rng.uniform(-746, -707, 400), rng.uniform(709, 711, 50),
                           [-708.0, np.nextafter(-708.0, -np.inf), -708.3964185322641, -744.44, -745.13, -745.14, -746.0,
                            709.782712893384, np.nextafter(709.782712893384, np.inf), 710.0, 1e300, -1e300,
                            np.inf, -np.inf, np.nan]])


def hypot_pairs():
    """(x, y, n): n random pairs of mixed magnitudes, then the hard cases (equal pairs, zeros, the
    2^-60 cut, scaled extremes)"""
    rng = np.random.default_rng(6)
    n = 6000
    x = rng.normal(size=n) * 10.0 ** rng.uniform(-12, 12, n)
    y = rng.normal(size=n) * 10.0 ** rng.uniform(-12, 12, n)
    hard = np.array([[3.0, 4.0], [1.0, 1.0], [0.0, 0.0], [-0.0, 5.0], [1.0, 2.0 ** -61], [1.0, 2.0 ** -59],
                     [1e300, 1e300], [1e-300, 3e-300], [5e-324, 5e-324], [1.5e308, 1.5e308], [2.0 ** 500, 1.0]])
    return np.concatenate([x, hard[:, 0]]), np.concatenate([y, hard[:, 1]]), n


def hypot_specials():
    inf, nan = np.inf, np.nan
    return np.array([inf, nan, -inf, nan, 0.0, -0.0, 1.7e308]), np.array([nan, inf, 1.0, 1.0, -0.0, 0.0, 1.7e308])


def acos_args():
    rng = np.random.default_rng(13)
    return np.concatenate([rng.uniform(-1, 1, 4000), 1.0 - 10.0 ** rng.uniform(-16, -1, 300), -1.0 + 10.0 ** rng.uniform(-16, -1, 300),
                           [1.0, -1.0, 0.0, -0.0, np.nextafter(1.0, 0.0), np.nextafter(-1.0, 0.0), 5e-324, 1.5, -1.5, np.nan]])


# ---------------------------------------------------------------- csrc/fm3d_fastdiv.h

# the guard bounds of fm3d_fastdiv.h: mdiv_ok's 1e-200 < |d| < 1e200, mdiv's |a| < 1e100, recip_z's
# 2^-700 <= |z| <= 2^700, div_nn_ok's 2^-600 <= |mm| <= 2^60
GUARD_BOUNDS = (1e-200, 1e200, 1e100, 2.0 ** -700, 2.0 ** 700, 2.0 ** -600, 2.0 ** 60)


def markstein_cases(n=4096, seed=20):
    """(a, d) whose quotient lies next to a rounding midpoint, the only inputs on which a one-step
    Markstein correction of q0 = RN(a RN(1/d)) can round wrongly.  For an odd 53-bit D, delta in
    {+-1, +-3} and k in {53, 54}: M = (-delta / D) mod 2^k; kept when 2^53 <= M < 2^54 (M is odd: the
    midpoint of two 53-bit neighbours) and A = (M D + delta) / 2^k (an integer by construction) lies in
    [2^52, 2^53).  Then A 2^k / D = M + delta / D.  Half of the D uniform, half 2^53 - 1 - 2 r with
    r < 2^40 (the largest error terms).  a = +-A 2^ea, d = +-D 2^ed inside mdiv's guard: |a| in
    [2^-200, 2^300], |d| in (1e-200, 1e200)."""
    rng = np.random.default_rng(seed)
    a = np.empty(n)
    d = np.empty(n)
    got = 0
    while got < n:
        if rng.integers(2):
            D = int(rng.integers(2 ** 51, 2 ** 52)) * 2 + 1
        else:
            D = 2 ** 53 - 1 - 2 * int(rng.integers(0, 2 ** 40))
        for delta in (1, -1, 3, -3):
            for k in (53, 54):
                M = (-delta * pow(D, -1, 2 ** k)) % 2 ** k
                if not 2 ** 53 <= M < 2 ** 54:
                    continue
                A, rem = divmod(M * D + delta, 2 ** k)
                assert rem == 0
                if not 2 ** 52 <= A < 2 ** 53 or got >= n:
                    continue
                ea = int(rng.integers(-252, 248))   # |a| = A 2^ea in [2^-200, 2^300)
                ed = int(rng.integers(-716, 612))   # |d| = D 2^ed in [2^-664, 2^664], inside (1e-200, 1e200)
                sa, sd = rng.choice([-1.0, 1.0], 2)
                a[got] = sa * np.ldexp(float(A), ea)
                d[got] = sd * np.ldexp(float(D), ed)
                got += 1
    assert (np.abs(a) >= 2.0 ** -200).all() and (np.abs(a) <= 2.0 ** 300).all()
    assert (np.abs(d) > 1e-200).all() and (np.abs(d) < 1e200).all()
    return a, d


def guard_edges():
    """every guard bound, its two neighbours, both signs; zeros, subnormals, infinities, NaN"""
    v = []
    for b in GUARD_BOUNDS:
        for u in (b, np.nextafter(b, 0.0), np.nextafter(b, np.inf)):
            v += [u, -u]
    v += [0.0, -0.0, 5e-324, -5e-324, 2.2e-310, -2.2e-310, 2.0 ** -1022, np.inf, -np.inf, np.nan]
    return np.array(v)


ORDINARY = np.array([1.0, -3.0, 1.5e-60, 7e59, 0.1, -1e10])


def edge_pairs():
    """(a, b): every ordered pair of guard_edges() and a few ordinary values"""
    v = np.concatenate([guard_edges(), ORDINARY])
    a, b = [g.ravel() for g in np.meshgrid(v, v, indexing="ij")]
    return a, b


def _inside(rng, n):
    """n (a, d) well inside mdiv's guard, full random mantissas"""
    a = np.ldexp(rng.uniform(1, 2, n), rng.integers(-150, 250, n)) * rng.choice([-1.0, 1.0], n)
    d = np.ldexp(rng.uniform(1, 2, n), rng.integers(-600, 600, n)) * rng.choice([-1.0, 1.0], n)
    return a, d


def wave_patterns(seed=21):
    """list of (name, a, d, inside): arrays of 64 m elements all inside mdiv's guard but one lane per
    wave at position 0, 31, 32 or 63 (alternately |d| >= 1e200, |d| <= 1e-200, |a| >= 1e100: the
    ballot branch with exactly one lane in it), all inside (the fast path only), all outside, and
    lengths with a partial last wave or block.  inside marks the lanes inside the guard."""
    rng = np.random.default_rng(seed)
    out = []
    for pos in (0, 31, 32, 63):
        m = 6
        a, d = _inside(rng, 64 * m)
        for w in range(m):
            i = 64 * w + pos
            if w % 3 == 0:
                d[i] = np.ldexp(d[i] / np.abs(d[i]) * 1.25, 700 + w)
            elif w % 3 == 1:
                d[i] = np.ldexp(d[i] / np.abs(d[i]) * 1.25, -700 - w)
            else:
                a[i] = np.ldexp(a[i] / np.abs(a[i]) * 1.25, 340 + w)
        out.append((f"one lane outside at {pos}", a, d))
    a, d = _inside(rng, 64 * 5)
    out.append(("all inside", a, d))
    a, d = _inside(rng, 64 * 5)
    e = rng.integers(700, 760, d.size) * np.where(np.arange(d.size) % 2 == 0, 1, -1)  # |d| >= 2^700 or < 2^-699
    d = np.ldexp(rng.uniform(1, 2, d.size), e) * rng.choice([-1.0, 1.0], d.size)
    out.append(("all outside", a, d))
    for n in (1, 63, 65, 257, 4097):
        a, d = _inside(rng, n)
        a[-1] = np.ldexp(1.25, 340)  # the last lane of the partial wave outside the guard
        out.append((f"length {n}", a, d))
        a, d = _inside(rng, n)
        out.append((f"length {n}, all inside", a, d))
    res = []
    for name, a, d in out:
        inside = (np.abs(d) > 1e-200) & (np.abs(d) < 1e200) & (np.abs(a) < 1e100)
        res.append((name, a, d, inside))
    return res


def div_nn_pairs(n=1 << 16, seed=22):
    """(mm, nn) for div_nn: numerators inside and around [2^-600, 2^60], denominators up to 2^60 and
    down to subnormals, the exponents drawn so that most quotients stay below 2^100"""
    rng = np.random.default_rng(seed)
    em = np.concatenate([rng.integers(-40, 40, n // 2), rng.integers(-600, 61, n // 4), rng.integers(-700, 100, n // 4)])
    mm = np.ldexp(rng.uniform(1, 2, n), em) * rng.choice([-1.0, 1.0], n)
    en = np.clip(em - rng.integers(-120, 96, n), -1074, 59)  # |nn| < 2^60
    en[::16] = rng.integers(-1074, 60, en[::16].size)  # anywhere, subnormal denominators included
    nn = np.ldexp(rng.uniform(1, 2, n), en) * rng.choice([-1.0, 1.0], n)
    return mm, nn


def operator_operands(n=1 << 20, seed=23, single=False):
    """(a, b) for the plain / and sqrt, n random pairs plus the subnormal and overflow edges: a of
    any exponent (subnormals included), b within 2^+-1100 (float: 2^+-160) of it, so that the
    quotients cover the normal range, the subnormals and both overflows; a negative now and then
    (sqrt's NaN).  Floats come widened exactly to double."""
    rng = np.random.default_rng(seed)
    emin, emax, gap = (-149, 127, 160) if single else (-1074, 1023, 1100)
    ea = rng.integers(emin, emax + 1, n)
    eb = np.clip(ea - rng.integers(-gap, gap + 1, n), emin, emax)
    a = np.ldexp(rng.uniform(1, 2, n), ea) * rng.choice([-1.0, 1.0, 1.0, 1.0], n)
    b = np.ldexp(rng.uniform(1, 2, n), eb) * rng.choice([-1.0, 1.0], n)
    if single:
        with np.errstate(over="ignore"):
            a, b = a.astype(np.float32), b.astype(np.float32)
        tiny, big, eps = np.float32(1.1754944e-38), np.finfo(np.float32).max, np.float32(1e-45)
        edges = np.array([0.0, -0.0, eps, -eps, tiny, np.nextafter(tiny, np.float32(0)), big, -big, np.inf, -np.inf, np.nan,
                          1.0, 3.0, np.float32(2) ** -126, np.float32(2) ** 127, np.float32(2) ** -75, np.float32(2) ** 64],
                         dtype=np.float32)
    else:
        tiny, big = 2.0 ** -1022, np.finfo(np.float64).max
        edges = np.array([0.0, -0.0, 5e-324, -5e-324, tiny, np.nextafter(tiny, 0.0), big, -big, np.inf, -np.inf, np.nan,
                          1.0, 3.0, 2.0 ** -1074, 2.0 ** 1023, 2.0 ** -537, 2.0 ** 512])
    ea, eb = [g.ravel() for g in np.meshgrid(edges, edges, indexing="ij")]
    a = np.concatenate([a, ea])
    b = np.concatenate([b, eb])
    return a.astype(np.float64), b.astype(np.float64)


# ---------------------------------------------------------------- fm3d_cvmath.h


def float_sweep():
    """every 4093rd bit pattern of the 2^32 floats (about 1.05 M values), widened exactly to double"""
    bits = np.arange(0, 2 ** 32, 4093, dtype=np.uint64).astype(np.uint32)
    with np.errstate(invalid="ignore"):  # the signalling NaN patterns
        return bits.view(np.float32).astype(np.float64)


def float_sweep_pairs():
    """(y, x) for the two-argument atan2 in degrees: the sweep against a shuffled copy, then the axes
    and signed zeros"""
    v = float_sweep()
    w = np.random.default_rng(24).permutation(v)
    ax = np.array([0.0, -0.0, 1.0, -1.0, np.float32(1e-45), np.float32(3e38), np.inf, -np.inf])
    ay, axx = [g.ravel() for g in np.meshgrid(ax, ax, indexing="ij")]
    return np.concatenate([v, ay]), np.concatenate([w, axx])
