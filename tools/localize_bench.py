"""Times the 2D-3D localisation (fm3d_localize_points) on one GPU: 90,000 matches between
a model of 90,000 points and an image's 90,000 keypoints (30 % of the matches given a random keypoint,
0.5 px noise, maxPx 2) against 256 and 1,024 samples (1,024 and 4,096 hypotheses), without and with the
normals' test.

    python tools/localize_bench.py [--out profiles/localize_points.json] [--runs 20] [--repeats 3]
                                   [--warmup 3] [--samples 256,1024] [--normals 0,1] [--refine 0]
                                   [--fold S:N=STATS.csv ... [--align-stats H=STATS.csv] [--verify-stats H=STATS.csv]]

Per sample count and variant the tool warms up, then takes `repeats` blocks of `runs` calls and reports
each block's median wall time of the whole call (one allocation, the uploads, the launches, the
downloads), the median of those and their spread, with the best model's counts.  The kernels are split
by runs of their own under the profiler, one per sample count (the two variants' kernels differ in
name),

    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -o localize -- \\
        python tools/localize_bench.py --samples 256 --repeats 1 --out DIR/tool.json

whose kernel statistics are then folded into the file of the unprofiled run (no GPU needed):

    python tools/localize_bench.py --out profiles/localize_points.json --fold 256:0=DIR/localize_kernel_stats.csv ...

per kernel the calls and the average, their sum, and for the scoring kernel the residual rate against
its arithmetic.  A residual is one match under one hypothesis (4 per sample, the invalid slots' zero
models included: the kernel scores them all): 27 fp64 operations as written (15 multiplies, 12
additions: three rows of R X + t, x - u z, y - v z, their squares' sum, tau^2 (z z)), 54 with the normals
(32 multiplies, 22 additions: R n, its dot product with Xc, d d, |Xc|^2 and its product with c^2 on top),
none of which the compiler may fuse (-ffp-contract=off); the vector units issue 39.3e12 unfused fp64
operations/s.  --align-stats and --verify-stats add align_score_kernel's and verify_score_kernel's rates
from profiled runs of tools/align_bench.py and tools/verify_bench.py in the same session (26 and 33
operations per residual), the yardsticks."""
import argparse
import csv
import importlib
import json
import math
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
fm3d = importlib.import_module("3dfeaturematcher_amd")

SAMPLES = (256, 1024)
FLOPS_PER_RESIDUAL = {0: 27, 1: 54}
YARDSTICK_FLOPS = {"align_score_kernel": 26, "verify_score_kernel": 33}
UNFUSED_FP64_PEAK = 39.3e12
MAX_PX = 2.0
FX, FY, CX, CY = 520.0, 520.0, 320.0, 240.0
STAGE_KERNELS = ("localize_", "scan_count_kernel", "scan_blocks_kernel", "scatter_kernel", "compact_small_kernel")
SHARED = ("localize_gather_kernel", "localize_hypothesis_kernel", "localize_argmax_kernel", "localize_refine_init_kernel",
          "localize_refit_solve_kernel", "localize_adopt_kernel")


def inputs(n=90_000, seed=11, wrong_frac=0.3, sigma_px=0.5):
    """a model of n points seen by a camera 12 degrees and up to 0.3 m away: (X, normals, kpts, matches, true)"""
    rng = np.random.default_rng(seed)
    px = np.stack([rng.uniform(20.0, 620.0, n), rng.uniform(20.0, 460.0, n)], axis=1)
    depth = rng.uniform(1.6, 2.3, n)
    Xc = np.stack([(px[:, 0] - CX) / FX * depth, (px[:, 1] - CY) / FY * depth, depth], axis=1)
    ax = rng.normal(size=3)
    ax /= np.linalg.norm(ax)
    K = np.array([[0, -ax[2], ax[1]], [ax[2], 0, -ax[0]], [-ax[1], ax[0], 0]])
    ang = math.radians(12.0)
    R = np.eye(3) + math.sin(ang) * K + (1 - math.cos(ang)) * (K @ K)
    t = rng.uniform(-0.3, 0.3, 3)
    X = (Xc - t) @ R
    nrm = (Xc / np.linalg.norm(Xc, axis=1)[:, None]) @ R
    perm = rng.permutation(n)
    kpts = np.zeros((n, 2), dtype=np.float32)
    kpts[perm] = (px + rng.normal(0.0, sigma_px, (n, 2))).astype(np.float32)
    wrong = rng.random(n) < wrong_frac
    query = perm.copy()
    query[wrong] = rng.integers(0, n, int(wrong.sum()))
    m = np.zeros(n, dtype=fm3d.DMATCH)
    m["queryIdx"], m["trainIdx"] = query, np.arange(n)
    return X, nrm, kpts, m, query == perm


def kernel_stats(path, prefixes=STAGE_KERNELS):
    """rocprofv3's kernel statistics: {short kernel name: calls, average} of the stage's kernels"""
    out = {}
    with open(path, newline="") as f:
        for row in csv.DictReader(f):
            name = row.get("Name", "")
            if not any(k in name for k in prefixes):
                continue
            short = name.split("(anonymous namespace)::")[-1].split("(")[0]
            short = short.replace("void ", "").replace("<true>", "<normals>").replace("<false>", "")
            out[short] = {"calls": int(row["Calls"]), "average_us": float(row["AverageNs"]) / 1e3}
    return out


def fold(path, specs, yardsticks):
    with open(path) as f:
        out = json.load(f)
    out["kernels"] = {}
    for spec in specs:
        key, csv_path = spec.split("=", 1)
        S, N = (int(v) for v in key.split(":"))
        ks = kernel_stats(csv_path)
        # one profiled run may hold both variants: this one's instances, and the kernels they share
        ks = {k: v for k, v in ks.items() if ("<normals>" in k) == bool(N) or not k.startswith("localize_") or k in SHARED}
        score = ks["localize_score_kernel<normals>" if N else "localize_score_kernel"]
        rate = out["matches"] * 4 * S / (score["average_us"] * 1e-6)
        ops = FLOPS_PER_RESIDUAL[N]
        out["kernels"][key] = {"per_kernel": ks, "hypotheses": 4 * S, "score_residuals_per_s": rate,
                               "fp64_ops_per_residual": ops, "score_fp64_ops_per_s": rate * ops,
                               "share_of_unfused_fp64_peak": rate * ops / UNFUSED_FP64_PEAK}
    for kernel, spec in yardsticks.items():
        if not spec:
            continue
        H, csv_path = spec.split("=", 1)
        ys = kernel_stats(csv_path, (kernel,))[kernel]
        rate = out["matches"] * int(H) / (ys["average_us"] * 1e-6)
        out[kernel] = {"hypotheses": int(H), "average_us": ys["average_us"], "residuals_per_s": rate,
                       "fp64_ops_per_residual": YARDSTICK_FLOPS[kernel],
                       "share_of_unfused_fp64_peak": rate * YARDSTICK_FLOPS[kernel] / UNFUSED_FP64_PEAK}
    with open(path, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps({k: out[k] for k in ("kernels",) + tuple(YARDSTICK_FLOPS) if k in out}))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="profiles/localize_points.json")
    ap.add_argument("--runs", type=int, default=20)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--samples", default=",".join(str(s) for s in SAMPLES))
    ap.add_argument("--normals", default="0,1")
    ap.add_argument("--refine", type=int, default=0)
    ap.add_argument("--fold", nargs="+", default=None, metavar="S:N=CSV",
                    help="add rocprofv3 kernel statistics (one profiled run per sample count) to --out and stop")
    ap.add_argument("--align-stats", default=None, metavar="H=CSV",
                    help="with --fold: a profiled tools/align_bench.py run's statistics (90,000 matches, H hypotheses)")
    ap.add_argument("--verify-stats", default=None, metavar="H=CSV",
                    help="with --fold: a profiled tools/verify_bench.py run's statistics (90,000 matches, H hypotheses)")
    args = ap.parse_args()
    if args.fold:
        return fold(args.out, args.fold, {"align_score_kernel": args.align_stats, "verify_score_kernel": args.verify_stats})
    if args.runs < 20:
        ap.error("--runs: at least 20")
    X, nrm, kpts, m, true = inputs()
    s = fm3d.Settings.default()
    s.Fx, s.Fy, s.Cx, s.Cy = FX, FY, CX, CY
    s.k0 = s.k1 = s.k2 = s.p1 = s.p2 = 0.0
    ctx = fm3d.Context(s, device=0)
    out = {"library": fm3d.lib().fm3d_version().decode(), "matches": int(len(m)), "true_matches": int(true.sum()),
           "max_px": MAX_PX, "refine": args.refine, "runs": []}
    try:
        loc = fm3d.ModelLocalizer(ctx)
        for N in (int(v) for v in args.normals.split(",")):
            for S in (int(v) for v in args.samples.split(",")):
                call = lambda: loc.localize(X, kpts, m, MAX_PX, nrm if N else None, 0.5, samples=S, refine=args.refine)
                for _ in range(args.warmup):
                    call()
                blocks = []
                for _ in range(args.repeats):
                    ms = []
                    for _ in range(args.runs):
                        t0 = time.perf_counter()
                        g, mask, inl, best = call()
                        ms.append((time.perf_counter() - t0) * 1e3)
                    blocks.append({"median_ms": statistics.median(ms), "min_ms": min(ms), "max_ms": max(ms)})
                meds = [b["median_ms"] for b in blocks]
                res = {"samples": S, "hypotheses": 4 * S, "normals": N, "call_ms": statistics.median(meds),
                       "repeat_spread_ms": max(meds) - min(meds), "repeats": blocks, "runs_per_repeat": args.runs,
                       "best": int(best), "inliers": int(mask.sum()), "true_kept": int((mask & true).sum()),
                       "wrong_kept": int((mask & ~true).sum())}
                out["runs"].append(res)
                print(json.dumps(res), flush=True)
    finally:
        ctx.close()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
