"""Times the 3D-3D alignment (fm3d_align_points) on one GPU: 90,000 matches between
two models of 90,000 points (30 % of the matches given a random train index, 1 mm noise, maxDist 5 mm)
against 1,024 and 4,096 hypotheses, without and with the normals' test.

    python tools/align_bench.py [--out profiles/align_points.json] [--runs 20] [--repeats 3]
                                [--warmup 3] [--hypotheses 1024,4096] [--normals 0,1]
                                [--fold H:N=STATS.csv ... [--verify-stats STATS.csv]]

Per hypothesis count and variant the tool warms up, then takes `repeats` blocks of `runs` calls and
reports each block's median wall time of the whole call (one allocation, the uploads, the launches,
the downloads), the median of those and their spread, with the best model's counts.  The kernels are
split by runs of their own under the profiler, one per hypothesis count (the two variants' kernels
differ in name),

    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -o align -- \\
        python tools/align_bench.py --hypotheses 1024 --repeats 1 --out DIR/tool.json

whose kernel statistics are then folded into the file of the unprofiled run (no GPU needed):

    python tools/align_bench.py --out profiles/align_points.json --fold 1024:0=DIR/align_kernel_stats.csv 1024:1=DIR/align_kernel_stats.csv ...

per kernel the calls and the average, their sum, and for the scoring kernel the residual rate against
its arithmetic.  A residual is 26 fp64 operations as written (12 multiplies, 14 additions: three rows
of R a + t - b, then the squared norm), 46 with the normals (24 multiplies, 22 additions: R n_a and its
dot product with n_b on top), none of which the compiler may fuse (-ffp-contract=off); the vector
units issue 39.3e12 unfused fp64 operations/s.  --verify-stats adds verify_score_kernel's rate from a
profiled run of tools/verify_bench.py in the same session (33 operations per residual), the yardstick."""
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

HYPOTHESES = (1024, 4096)
FLOPS_PER_RESIDUAL = {0: 26, 1: 46}
VERIFY_FLOPS_PER_RESIDUAL = 33
UNFUSED_FP64_PEAK = 39.3e12
MAX_DIST = 0.005
STAGE_KERNELS = ("align_", "scan_count_kernel", "scan_blocks_kernel", "scatter_kernel", "compact_small_kernel")


def inputs(n=90_000, seed=11, wrong_frac=0.3, sigma=0.001):
    """two models of n points under a 20 degree rotation: (A, nA, B, nB, matches, true)"""
    rng = np.random.default_rng(seed)
    A = np.stack([rng.uniform(-1.0, 1.0, n), rng.uniform(-0.75, 0.75, n), rng.uniform(1.5, 2.4, n)], axis=1)
    nA = rng.normal(size=(n, 3))
    nA /= np.linalg.norm(nA, axis=1)[:, None]
    ax = rng.normal(size=3)
    ax /= np.linalg.norm(ax)
    K = np.array([[0, -ax[2], ax[1]], [ax[2], 0, -ax[0]], [-ax[1], ax[0], 0]])
    ang = math.radians(20.0)
    R = np.eye(3) + math.sin(ang) * K + (1 - math.cos(ang)) * (K @ K)
    t = rng.uniform(-0.3, 0.3, 3)
    perm = rng.permutation(n)
    B, nB = np.zeros((n, 3)), np.zeros((n, 3))
    B[perm] = A @ R.T + t + rng.normal(0.0, sigma, (n, 3))
    nB[perm] = nA @ R.T
    wrong = rng.random(n) < wrong_frac
    train = perm.copy()
    train[wrong] = rng.integers(0, n, int(wrong.sum()))
    m = np.zeros(n, dtype=fm3d.DMATCH)
    m["queryIdx"], m["trainIdx"] = np.arange(n), train
    return A, nA, B, nB, m, train == perm


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


def fold(path, specs, verify_stats):
    with open(path) as f:
        out = json.load(f)
    out["kernels"] = {}
    for spec in specs:
        key, csv_path = spec.split("=", 1)
        H, N = (int(v) for v in key.split(":"))
        ks = kernel_stats(csv_path)
        # one profiled run may hold both variants: this one's instances, and the kernels they share
        ks = {k: v for k, v in ks.items() if ("<normals>" in k) == bool(N) or not k.startswith("align_") or
              k in ("align_gather_kernel", "align_hypothesis_kernel", "align_argmax_kernel")}
        score = ks["align_score_kernel<normals>" if N else "align_score_kernel"]
        rate = out["matches"] * H / (score["average_us"] * 1e-6)
        ops = FLOPS_PER_RESIDUAL[N]
        out["kernels"][key] = {"per_kernel": ks, "score_residuals_per_s": rate, "fp64_ops_per_residual": ops,
                               "score_fp64_ops_per_s": rate * ops,
                               "share_of_unfused_fp64_peak": rate * ops / UNFUSED_FP64_PEAK}
    if verify_stats:
        H, csv_path = verify_stats.split("=", 1)
        vs = kernel_stats(csv_path, ("verify_score_kernel",))["verify_score_kernel"]
        rate = out["matches"] * int(H) / (vs["average_us"] * 1e-6)
        out["verify_score_kernel"] = {"hypotheses": int(H), "average_us": vs["average_us"], "residuals_per_s": rate,
                                      "fp64_ops_per_residual": VERIFY_FLOPS_PER_RESIDUAL,
                                      "share_of_unfused_fp64_peak": rate * VERIFY_FLOPS_PER_RESIDUAL / UNFUSED_FP64_PEAK}
    with open(path, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps({k: out[k] for k in ("kernels", "verify_score_kernel") if k in out}))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="profiles/align_points.json")
    ap.add_argument("--runs", type=int, default=20)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--hypotheses", default=",".join(str(h) for h in HYPOTHESES))
    ap.add_argument("--normals", default="0,1")
    ap.add_argument("--refine", type=int, default=0)
    ap.add_argument("--fold", nargs="+", default=None, metavar="H:N=CSV",
                    help="add rocprofv3 kernel statistics (one profiled run per hypothesis count) to --out and stop")
    ap.add_argument("--verify-stats", default=None, metavar="H=CSV",
                    help="with --fold: a profiled tools/verify_bench.py run's statistics (90,000 matches, H hypotheses)")
    args = ap.parse_args()
    if args.fold:
        return fold(args.out, args.fold, args.verify_stats)
    if args.runs < 20:
        ap.error("--runs: at least 20")
    A, nA, B, nB, m, true = inputs()
    ctx = fm3d.Context(fm3d.Settings.default(), device=0)
    out = {"library": fm3d.lib().fm3d_version().decode(), "matches": int(len(m)), "true_pairs": int(true.sum()),
           "max_dist": MAX_DIST, "refine": args.refine, "runs": []}
    try:
        al = fm3d.ModelAligner(ctx)
        for N in (int(v) for v in args.normals.split(",")):
            na, nb = (nA, nB) if N else (None, None)
            for H in (int(v) for v in args.hypotheses.split(",")):
                call = lambda: al.align(A, B, m, MAX_DIST, na, nb, 0.9, hypotheses=H, refine=args.refine)
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
                res = {"hypotheses": H, "normals": N, "call_ms": statistics.median(meds),
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
