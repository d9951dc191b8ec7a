"""Times the geometric verification (fm3d_verify_matches) on one GPU: 90,000 matches
(the C4 pair's count: the true pairs of a 100,000-keypoint synthetic pair, 30 % of them given a random
train index) against 1,024 and 4,096 hypotheses at 1 px.

    python tools/verify_bench.py [--out profiles/verify_matches.json] [--runs 20] [--repeats 3]
                                 [--warmup 3] [--hypotheses 1024,4096] [--fold H=STATS.csv ...]

Per hypothesis count the tool warms up, then takes `repeats` blocks of `runs` calls and reports each
block's median wall time of the whole call (one allocation, the uploads, eight launches, the
downloads), the median of those and their spread, with the best model's counts.  The kernels are
split by runs of their own under the profiler, one per hypothesis count,

    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -o verify -- \\
        python tools/verify_bench.py --hypotheses 1024 --repeats 1 --out DIR/tool.json

whose kernel statistics are then folded into the file of the unprofiled run (no GPU needed):

    python tools/verify_bench.py --out profiles/verify_matches.json --fold 1024=DIR/verify_kernel_stats.csv ...

per kernel the calls and the average, their sum, and for the scoring kernel the residual rate against
its arithmetic.  A residual is 33 fp64 operations as written (18 multiplies, 15 additions), none of
which the compiler may fuse (-ffp-contract=off); the vector units issue 39.3e12 unfused fp64
operations/s (half the 78.6 TFLOPS that count an FMA as two)."""
import argparse
import csv
import importlib
import json
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
fm3d = importlib.import_module("3dfeaturematcher_amd")
synth = importlib.import_module("3dfeaturematcher_amd.synth")

HYPOTHESES = (1024, 4096)
FLOPS_PER_RESIDUAL = 33  # 18 multiplies + 15 additions, none fused
UNFUSED_FP64_PEAK = 39.3e12
STAGE_KERNELS = ("verify_", "scan_count_kernel", "scan_blocks_kernel", "scatter_kernel", "compact_small_kernel")


def inputs(n=100_000, seed=11, wrong_frac=0.3):
    cam = synth.Camera.reference(640)
    cam = synth.Camera(cam.fx, cam.fy, cam.cx, cam.cy, (0.0, 0.0, 0.0, 0.0, 0.0))
    pair = synth.make_frame_pair(n, seed=seed, cam=cam)
    q = np.nonzero(pair.true_train >= 0)[0]
    t = pair.true_train[q].copy()
    rng = np.random.default_rng(5)
    wrong = rng.random(q.size) < wrong_frac
    t[wrong] = rng.integers(0, pair.kp2.shape[0], int(wrong.sum()))
    m = np.zeros(q.size, dtype=fm3d.DMATCH)
    m["queryIdx"], m["trainIdx"] = q, t
    return pair, m, t == pair.true_train[q]


def kernel_stats(path):
    """rocprofv3's kernel statistics: {short kernel name: calls, average} of the stage's kernels"""
    out = {}
    with open(path, newline="") as f:
        for row in csv.DictReader(f):
            name = row.get("Name", "")
            if not any(k in name for k in STAGE_KERNELS):
                continue
            short = name.split("(anonymous namespace)::")[-1].split("(")[0].split("<")[0]
            out[short] = {"calls": int(row["Calls"]), "average_us": float(row["AverageNs"]) / 1e3}
    return out


def fold(path, specs):
    with open(path) as f:
        out = json.load(f)
    out["kernels"] = {}
    for spec in specs:
        H, csv_path = spec.split("=", 1)
        ks = kernel_stats(csv_path)
        rate = out["matches"] * int(H) / (ks["verify_score_kernel"]["average_us"] * 1e-6)
        out["kernels"][H] = {"per_kernel": ks, "kernels_total_us": sum(v["average_us"] for v in ks.values()),
                             "score_residuals_per_s": rate, "score_fp64_ops_per_s": rate * FLOPS_PER_RESIDUAL,
                             "share_of_unfused_fp64_peak": rate * FLOPS_PER_RESIDUAL / UNFUSED_FP64_PEAK}
    with open(path, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps(out["kernels"]))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="profiles/verify_matches.json")
    ap.add_argument("--runs", type=int, default=20)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--hypotheses", default=",".join(str(h) for h in HYPOTHESES))
    ap.add_argument("--fold", nargs="+", default=None, metavar="H=CSV",
                    help="add rocprofv3 kernel statistics (one profiled run per hypothesis count) to --out and stop")
    args = ap.parse_args()
    if args.fold:
        return fold(args.out, args.fold)
    if args.runs < 20:
        ap.error("--runs: at least 20")
    pair, m, true = inputs()
    s = fm3d.Settings.default()
    s.set_camera(pair.cam)
    ctx = fm3d.Context(s, device=0)
    out = {"library": fm3d.lib().fm3d_version().decode(), "matches": int(len(m)), "true_pairs": int(true.sum()),
           "max_px": 1.0, "runs": []}
    try:
        sct = fm3d.SingleCameraTriangulator(ctx)
        for H in (int(v) for v in args.hypotheses.split(",")):
            for _ in range(args.warmup):
                sct.verifyMatches(pair.kp1, pair.kp2, m, 1.0, hypotheses=H)
            blocks = []
            for _ in range(args.repeats):
                ms = []
                for _ in range(args.runs):
                    t0 = time.perf_counter()
                    E, mask, inl, best = sct.verifyMatches(pair.kp1, pair.kp2, m, 1.0, hypotheses=H)
                    ms.append((time.perf_counter() - t0) * 1e3)
                blocks.append({"median_ms": statistics.median(ms), "min_ms": min(ms), "max_ms": max(ms)})
            meds = [b["median_ms"] for b in blocks]
            res = {"hypotheses": H, "call_ms": statistics.median(meds), "repeat_spread_ms": max(meds) - min(meds),
                   "repeats": blocks, "runs_per_repeat": args.runs, "best": int(best), "inliers": int(mask.sum()),
                   "true_kept": int((mask & true).sum()), "wrong_kept": int((mask & ~true).sum())}
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
