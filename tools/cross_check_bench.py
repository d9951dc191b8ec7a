"""Times the pipeline's match stage (match_ms: row constants, both knn2 searches, NNDR, the mutual
test and the compaction, HIP events on the context stream) with the cross-check off and on
(Fm3d.crossCheck 0, 1, 2), each with the epipolar gate off and on (Fm3d.guidedMatchPx), on a resident
frame pair, one pair at a time.

    python tools/cross_check_bench.py [--out profiles/cross_check.json] [--max-px 2] [--runs 20]
                                      [--repeats 3] [--warmup 3] [--off-only]

Workloads: 100k x 100k u8-128 (SIFT-like) and 10k x 10k ORB (synth.make_frame_pair).  Per mode the
tool uploads the pair once, warms up, then takes `repeats` blocks of `runs` run_dlt() calls and
reports each block's median match_ms, the median of those and their spread, with the kept-match
and inlier counts.  --off-only times crossCheck = 0 alone (a library without the setting, e.g. the
parent commit's through FM3D_LIB)."""
import argparse
import importlib
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
fm3d = importlib.import_module("3dfeaturematcher_amd")
synth = importlib.import_module("3dfeaturematcher_amd.synth")

WORKLOADS = (("sift128_u8_100k", 100_000, "sift"), ("orb256_bits_10k", 10_000, "orb"))


def time_mode(pair, binary, cross, px, args):
    s = fm3d.Settings.default()
    s.set_camera(pair.cam)
    s.guidedMatchPx = px
    s.crossCheck = cross
    ctx = fm3d.Context(s, device=0)
    try:
        fm3d.SingleCameraTriangulator(ctx).set_g12(pair.g12)
        pipe = fm3d.Pipeline(ctx)
        pipe.upload(pair.desc1, pair.desc2, pair.kp1, pair.kp2, None, None, binary=binary)
        for _ in range(args.warmup):
            inl, st = pipe.run_dlt()
        blocks = []
        for _ in range(args.repeats):
            ms = []
            for _ in range(args.runs):
                inl, st = pipe.run_dlt()
                ms.append(st["match_ms"])
            blocks.append({"median_ms": statistics.median(ms), "min_ms": min(ms), "max_ms": max(ms)})
        meds = [b["median_ms"] for b in blocks]
        return {"crossCheck": cross, "guidedMatchPx": px, "match_ms": statistics.median(meds),
                "repeat_spread_ms": max(meds) - min(meds), "repeats": blocks, "runs_per_repeat": args.runs,
                "matches": int(st["matches"]), "inliers": int(inl)}
    finally:
        ctx.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="profiles/cross_check.json")
    ap.add_argument("--max-px", type=float, default=2.0)
    ap.add_argument("--runs", type=int, default=20)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--off-only", action="store_true")
    ap.add_argument("--workloads", default=",".join(w[0] for w in WORKLOADS))
    args = ap.parse_args()
    if args.runs < 20:
        ap.error("--runs: at least 20")
    out = {"library": fm3d.lib().fm3d_version().decode(), "max_px": args.max_px, "workloads": {}}
    for name, n, desc in WORKLOADS:
        if name not in args.workloads.split(","):
            continue
        pair = synth.make_frame_pair(n, seed=11, desc=desc)
        res = {"queries": n, "trains": n, "modes": []}
        for px in (0.0,) if args.off_only else (0.0, args.max_px):
            for cross in (0,) if args.off_only else (0, 1, 2):
                res["modes"].append(time_mode(pair, desc == "orb", cross, px, args))
        if not args.off_only:
            base = {m["guidedMatchPx"]: m["match_ms"] for m in res["modes"] if m["crossCheck"] == 0}
            for m in res["modes"]:
                m["over_one_way"] = m["match_ms"] / base[m["guidedMatchPx"]]
        out["workloads"][name] = res
        print(name, json.dumps(res), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
