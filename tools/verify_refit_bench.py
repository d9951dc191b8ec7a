"""Times the geometric verification with the refit on the inliers (fm3d_verify_matches_refined, DESIGN.md
§3.1d) on one GPU: tools/verify_bench.py's workload -- 90,000 matches against 1,024 hypotheses at 1 px --
with refineIters 0, 1 and 3.

    python tools/verify_refit_bench.py [--out profiles/verify_refit.json] [--runs 20] [--repeats 3]
                                       [--warmup 3] [--plain-only] [--fold R=STATS.csv ...]
                                       [--parent A.json B.json ...]

Per level the tool warms up, then takes `repeats` blocks of `runs` calls and reports each block's median
wall time of the whole call, the median of those and their spread, with the rounds' counts.
--plain-only times refineIters = 0 alone (a library without the entry point, e.g. the parent commit's
through FM3D_LIB); run it and this build's alternately and hand the parent's files to --parent, which
adds their medians and spread to --out (no GPU needed).  The kernels are split by runs of their own under
the profiler, one per level,

    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -o refit -- \\
        python tools/verify_refit_bench.py --levels 3 --repeats 1 --out DIR/tool.json

whose kernel statistics --fold then adds (no GPU needed): per kernel the calls and the average, and the
kernel time of one call (the sum of calls x average over the profiled calls, counted by the
coordinate kernel's launches: one per call)."""
import argparse
import importlib
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
fm3d = importlib.import_module("3dfeaturematcher_amd")
import verify_bench  # the workload and the statistics reader

LEVELS = (0, 1, 3)
HYPOTHESES = 1024


def fold(path, specs):
    with open(path) as f:
        out = json.load(f)
    out["kernels"] = {}
    for spec in specs:
        R, csv_path = spec.split("=", 1)
        ks = verify_bench.kernel_stats(csv_path)
        total = sum(v["calls"] * v["average_us"] for v in ks.values())
        calls = ks["verify_coords_kernel"]["calls"]  # one launch per call
        out["kernels"][R] = {"per_kernel": ks, "profiled_calls": calls, "kernel_us_per_call": total / calls}
    with open(path, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps(out["kernels"]))


def parent(path, files):
    with open(path) as f:
        out = json.load(f)
    meds = []
    for p in files:
        with open(p) as f:
            meds.append(json.load(f)["runs"][0]["call_ms"])
    out["parent"] = {"files": [os.path.basename(p) for p in files], "call_ms": meds,
                     "median_ms": statistics.median(meds), "spread_ms": max(meds) - min(meds)}
    with open(path, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps(out["parent"]))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="profiles/verify_refit.json")
    ap.add_argument("--runs", type=int, default=20)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--levels", default=",".join(str(r) for r in LEVELS))
    ap.add_argument("--plain-only", action="store_true")
    ap.add_argument("--fold", nargs="+", default=None, metavar="R=CSV")
    ap.add_argument("--parent", nargs="+", default=None, metavar="JSON")
    args = ap.parse_args()
    if args.fold:
        return fold(args.out, args.fold)
    if args.parent:
        return parent(args.out, args.parent)
    if args.runs < 20:
        ap.error("--runs: at least 20")
    pair, m, true = verify_bench.inputs()
    s = fm3d.Settings.default()
    s.set_camera(pair.cam)
    ctx = fm3d.Context(s, device=0)
    out = {"library": fm3d.lib().fm3d_version().decode(), "lib_path": os.path.basename(fm3d.LIB_PATH),
           "matches": int(len(m)), "true_pairs": int(true.sum()), "hypotheses": HYPOTHESES, "max_px": 1.0, "runs": []}
    try:
        sct = fm3d.SingleCameraTriangulator(ctx)
        for R in (0,) if args.plain_only else [int(v) for v in args.levels.split(",")]:
            call = lambda: sct.verifyMatches(pair.kp1, pair.kp2, m, 1.0, hypotheses=HYPOTHESES, refine=R)
            for _ in range(args.warmup):
                call()
            blocks = []
            for _ in range(args.repeats):
                ms = []
                for _ in range(args.runs):
                    t0 = time.perf_counter()
                    E, mask, inl, best = call()
                    ms.append((time.perf_counter() - t0) * 1e3)
                blocks.append({"median_ms": statistics.median(ms), "min_ms": min(ms), "max_ms": max(ms)})
            meds = [b["median_ms"] for b in blocks]
            res = {"refineIters": R, "call_ms": statistics.median(meds), "repeat_spread_ms": max(meds) - min(meds),
                   "repeats": blocks, "runs_per_repeat": args.runs, "best": int(best), "inliers": int(mask.sum()),
                   "true_kept": int((mask & true).sum()), "wrong_kept": int((mask & ~true).sum())}
            if R:
                dbg = sct.verifyMatches(pair.kp1, pair.kp2, m, 1.0, hypotheses=HYPOTHESES, refine=R, debug=True)
                res["round_counts"], res["rounds_adopted"] = [int(c) for c in dbg[6]], int(dbg[8])
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
