"""Where fm3d_sin / fm3d_cos (include/fm3d_detmath.h) stop being accurate: the largest error in ulps
against mpmath per binade [2^e, 2^(e+1)), over random arguments of both signs, through the oracle's
host build (orc_math_eval, DETMATH | DET_1ULP).  fm3d_sin_cr / fm3d_cos_cr hand over to these
functions from |x| = 2^19 on.  The figures are recorded in DESIGN.md §4, not asserted.  CPU only.

    make -C oracle && python tools/micro/sincos_range.py [--per-binade 2000] [--from 0] [--to 64]
"""
import argparse
import os
import sys

import mpmath
import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
import oracle as orc  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--per-binade", type=int, default=2000)
    ap.add_argument("--from", dest="lo", type=int, default=0)
    ap.add_argument("--to", dest="hi", type=int, default=64)
    a = ap.parse_args()
    rng = np.random.default_rng(5)
    first, cliff = {}, {}
    print("binade        max ulp error sin   cos")
    for e in range(a.lo, a.hi):
        x = np.ldexp(rng.uniform(1, 2, a.per_binade), e) * rng.choice([-1.0, 1.0], a.per_binade)
        row = []
        for fn, f in (("sin", mpmath.sin), ("cos", mpmath.cos)):
            got = orc.math_eval(fn, x, mode=orc.DETMATH | orc.DET_1ULP)
            with mpmath.workprec(max(200, 2 * e + 120)):
                err = max(float(abs(mpmath.mpf(float(g)) - f(mpmath.mpf(float(v)))) / mpmath.mpf(float(np.spacing(abs(float(f(mpmath.mpf(float(v)))))))))
                          for g, v in zip(got, x))
            row.append(err)
            if err > 1.0 and fn not in first:
                first[fn] = e
            if err > 4.0 and fn not in cliff:
                cliff[fn] = e
        print(f"[2^{e}, 2^{e + 1})   {row[0]:14.3g} {row[1]:10.3g}")
    for fn in ("sin", "cos"):
        print(f"{fn}: first binade with an error above one ulp:", f"2^{first[fn]}" if fn in first else "none in range",
              "; above four ulps:", f"2^{cliff[fn]}" if fn in cliff else "none in range")


if __name__ == "__main__":
    main()
