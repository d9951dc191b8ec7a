"""Times the verified DLT leg of the pipeline (fm3d_pipeline_run_dlt_verified, DESIGN.md §3.1d "In the
pipeline") on one GPU against what it replaces: the §3.1d cost workload -- a 100,000-keypoint synthetic
pair under the zero-distortion camera -- at 1,024 hypotheses and 1 px, the pose taken from the model.

    python tools/verify_pipeline_bench.py [--out profiles/verify_pipeline.json] [--runs 20] [--repeats 3]
                                          [--warmup 3] [--only verified] [--fold STATS.csv]

Three things are timed, each as the median of `repeats` blocks' medians over `runs` calls (wall time of
the whole call or chain, the spread of the blocks' medians beside it):

  verified   fm3d_pipeline_run_dlt_verified on the staged pair (pose_from_model);
  composed   the seven calls it replaces, from host arrays: fm3d_match_nndr, fm3d_verify_matches,
             fm3d_undistort on both point sets, fm3d_pose_from_epipolar, fm3d_set_g12,
             fm3d_pipeline_upload (no images), fm3d_pipeline_run_dlt;
  plain      fm3d_pipeline_run_dlt on the staged pair under the composed pose (no verification).

The two new kernels are split by a run of their own under the profiler,

    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -o vp -- \\
        python tools/verify_pipeline_bench.py --only verified --repeats 1 --out DIR/tool.json

whose kernel statistics --fold then adds (no GPU needed)."""
import argparse
import ctypes
import importlib
import json
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
fm3d = importlib.import_module("3dfeaturematcher_amd")
import verify_bench  # the workload and the statistics reader

HYPOTHESES = 1024
MAX_PX = 1.0
WHAT = ("verified", "composed", "plain")


def undistort(ctx, xy):
    xy = np.ascontiguousarray(xy, dtype=np.float64)
    out = np.zeros_like(xy)
    ctx.check(fm3d.lib().fm3d_undistort(ctx.handle, xy.ctypes.data_as(ctypes.POINTER(ctypes.c_double)), len(xy),
                                        out.ctypes.data_as(ctypes.POINTER(ctypes.c_double))))
    return out


def timed(call, warmup, repeats, runs):
    for _ in range(warmup):
        res = call()
    blocks = []
    for _ in range(repeats):
        ms = []
        for _ in range(runs):
            t0 = time.perf_counter()
            res = call()
            ms.append((time.perf_counter() - t0) * 1e3)
        blocks.append({"median_ms": statistics.median(ms), "min_ms": min(ms), "max_ms": max(ms)})
    meds = [b["median_ms"] for b in blocks]
    return res, {"call_ms": statistics.median(meds), "repeat_spread_ms": max(meds) - min(meds), "repeats": blocks,
                 "runs_per_repeat": runs}


def fold(path, csv_path):
    with open(path) as f:
        out = json.load(f)
    ks = verify_bench.kernel_stats(csv_path)
    calls = ks["verify_coords_kernel"]["calls"]  # one launch per verified run
    out["kernels"] = {"per_kernel": ks, "profiled_calls": calls,
                      "verify_kernels_us_per_call": sum(v["calls"] * v["average_us"] for v in ks.values()) / calls,
                      "pose_kernels_us_per_call": sum(ks[k]["calls"] * ks[k]["average_us"] for k in ks
                                                      if k.startswith("verify_pose_")) / calls}
    with open(path, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps(out["kernels"]))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="profiles/verify_pipeline.json")
    ap.add_argument("--runs", type=int, default=20)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--only", default=",".join(WHAT))
    ap.add_argument("--fold", default=None, metavar="CSV")
    args = ap.parse_args()
    if args.fold:
        return fold(args.out, args.fold)
    if args.runs < 20:
        ap.error("--runs: at least 20")
    what = args.only.split(",")
    pair, _, _ = verify_bench.inputs()
    base = float(np.linalg.norm(pair.g12[:3, 3]))
    s = fm3d.Settings.default()
    s.set_camera(pair.cam)
    out = {"library": fm3d.lib().fm3d_version().decode(), "lib_path": os.path.basename(fm3d.LIB_PATH),
           "keypoints": int(len(pair.kp1)), "hypotheses": HYPOTHESES, "max_px": MAX_PX, "nndrEpsilon": s.nndrEpsilon}
    ctx, ctx2 = fm3d.Context(s, device=0), fm3d.Context(s, device=0)
    try:
        dm, sct, pipe2 = fm3d.DescriptorsMatcher(ctx2), fm3d.SingleCameraTriangulator(ctx2), fm3d.Pipeline(ctx2)

        def composed():
            m = dm.compareWithNNDR(s.nndrEpsilon, pair.desc1, pair.desc2)
            E, mask, inl, best = sct.verifyMatches(pair.kp1, pair.kp2, m, MAX_PX, hypotheses=HYPOTHESES)
            x1 = undistort(ctx2, pair.kp1[inl["queryIdx"]])
            x2 = undistort(ctx2, pair.kp2[inl["trainIdx"]])
            g, votes, ok = fm3d.pose_from_epipolar(E, x1, x2, base)
            sct.set_g12(g)
            pipe2.upload(pair.desc1, pair.desc2, pair.kp1, pair.kp2, None, None)
            P, st = pipe2.run_dlt()
            return dict(matches=len(m), verified=int(mask.sum()), best=int(best), votes=votes.tolist(), g12=g,
                        rerun_matches=st["matches"], inliers=P)

        pipe = fm3d.Pipeline(ctx)
        pipe.upload(pair.desc1, pair.desc2, pair.kp1, pair.kp2, None, None)
        P, st, rep = pipe.run_dlt_verified(MAX_PX, hypotheses=HYPOTHESES, pose_from_model=True, baseline=base)
        true = pair.true_train >= 0
        out["result"] = {"matches": rep["matches"], "verified": rep["verified"], "best": rep["best"],
                         "votes": rep["votes"].tolist(), "inliers": P, "true_pairs": int(true.sum())}
        if "verified" in what:
            (P, st, rep), t = timed(lambda: pipe.run_dlt_verified(MAX_PX, hypotheses=HYPOTHESES, pose_from_model=True,
                                                                  baseline=base), args.warmup, args.repeats, args.runs)
            t.update(verify_ms=rep["verify_ms"], match_ms=st["match_ms"], total_ms=st["total_ms"], inliers=P)
            out["verified"] = t
            print("verified", json.dumps(t), flush=True)
        if "composed" in what:
            res, t = timed(composed, args.warmup, args.repeats, args.runs)
            t.update({k: v for k, v in res.items() if k != "g12"})
            t["same_as_verified"] = bool(res["g12"].tobytes() == rep["g12"].tobytes() and res["inliers"] == P and
                                         res["verified"] == rep["verified"])
            out["composed"] = t
            print("composed", json.dumps(t), flush=True)
        if "plain" in what:
            (P0, st0), t = timed(pipe.run_dlt, args.warmup, args.repeats, args.runs)  # under the installed pose
            t.update(match_ms=st0["match_ms"], total_ms=st0["total_ms"], matches=st0["matches"], inliers=P0)
            out["plain"] = t
            print("plain", json.dumps(t), flush=True)
    finally:
        ctx.close()
        ctx2.close()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
