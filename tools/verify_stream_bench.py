"""Times the verified DLT leg as a stream of frame pairs (fm3d_pipeline_submit_dlt_verified /
fm3d_pipeline_wait_dlt_verified, DESIGN.md §3.1d "Submit / wait") on one GPU: the §3.1d cost workload -- a
100,000-keypoint synthetic pair under the zero-distortion camera -- at 1,024 hypotheses and 1 px, in
filter mode under the pair's true pose.

    python tools/verify_stream_bench.py [--out profiles/verify_stream.json] [--pairs 100] [--repeats 3]
                                        [--warmup 8] [--only sync,queued,plain] [--merge-parent JSON[,JSON]]

Per pair, wall time of a loop of `pairs` pairs that ends with every result on the host, over `pairs`;
each figure is the median of `repeats` such loops, the spread of the loops beside it:

  sync       (a) fm3d_pipeline_run_dlt_verified called in a loop on one context: the only form a build
             from before the submit / wait calls has (FM3D_LIB=<that build> ... --only sync times it;
             --merge-parent adds its JSON to this build's as "parent_sync");
  queued_N   (b), (c) submit_dlt_verified / wait_dlt_verified round-robin over N = 1, 2, 4 contexts, each
             holding the staged pair: a context's pair is waited for just before its next submit;
  plain_N    (d) submit_dlt / wait_dlt the same way: the floor, no verification.

The queued forms must return the synchronous call's counts and E; the tool fails otherwise."""
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
import verify_bench  # the workload

HYPOTHESES = 1024
MAX_PX = 1.0
IN_FLIGHT = (1, 2, 4)


def stream(pipes, submit, wait, pairs):
    """`pairs` pairs round-robin over the contexts -> (seconds, the last result of each context)"""
    pending = [False] * len(pipes)
    last = [None] * len(pipes)
    t0 = time.perf_counter()
    for i in range(pairs):
        k = i % len(pipes)
        if pending[k]:
            last[k] = wait(pipes[k])
        submit(pipes[k])
        pending[k] = True
    for k in range(len(pipes)):
        if pending[k]:
            last[k] = wait(pipes[k])
    return time.perf_counter() - t0, last


def timed(loop, warmup, repeats, pairs):
    loop(warmup)
    ms = []
    for _ in range(repeats):
        sec, last = loop(pairs)
        ms.append(sec * 1e3 / pairs)
    return last, {"pair_ms": statistics.median(ms), "repeat_spread_ms": max(ms) - min(ms), "repeats_ms": ms,
                  "pairs_per_repeat": pairs}


def summary(P, st, rep):
    return {"matches": rep["matches"], "verified": rep["verified"], "best": rep["best"],
            "roundsAdopted": rep["roundsAdopted"], "stats_matches": st["matches"], "inliers": P,
            "E": rep["E"].ravel().tolist()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="profiles/verify_stream.json")
    ap.add_argument("--pairs", type=int, default=100)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=8)
    ap.add_argument("--only", default="sync,queued,plain")
    ap.add_argument("--merge-parent", default=None, metavar="JSON[,JSON]")
    args = ap.parse_args()
    if args.merge_parent:
        with open(args.out) as f:
            out = json.load(f)
        for i, path in enumerate(args.merge_parent.split(",")):  # runs before and after this build's
            with open(path) as f:
                par = json.load(f)
            out["parent_sync" + ("" if i == 0 else f"_{i + 1}")] = dict(par["sync"], lib_path=par["lib_path"],
                                                                         result=par["result"])
        with open(args.out, "w") as f:
            json.dump(out, f, indent=1)
            f.write("\n")
        return
    if args.pairs < 20:
        ap.error("--pairs: at least 20")
    what = args.only.split(",")
    have_queued = hasattr(fm3d.lib(), "fm3d_pipeline_submit_dlt_verified")
    if "queued" in what and not have_queued:
        ap.error("this library has no fm3d_pipeline_submit_dlt_verified: --only sync[,plain]")
    pair, _, _ = verify_bench.inputs()
    s = fm3d.Settings.default()
    s.set_camera(pair.cam)
    out = {"library": fm3d.lib().fm3d_version().decode(), "lib_path": os.path.basename(fm3d.LIB_PATH),
           "keypoints": int(len(pair.kp1)), "hypotheses": HYPOTHESES, "max_px": MAX_PX, "nndrEpsilon": s.nndrEpsilon,
           "mode": "filter (poseFromModel = 0) under the pair's true pose"}
    ctxs = [fm3d.Context(s, device=0) for _ in range(max(IN_FLIGHT))]
    try:
        pipes = []
        for c in ctxs:
            fm3d.SingleCameraTriangulator(c).set_g12(pair.g12)
            p = fm3d.Pipeline(c)
            p.upload(pair.desc1, pair.desc2, pair.kp1, pair.kp2, None, None)
            pipes.append(p)
        run = lambda p: p.run_dlt_verified(MAX_PX, hypotheses=HYPOTHESES)
        want = summary(*run(pipes[0]))
        out["result"] = want
        if "sync" in what:
            def sync_loop(n):
                t0 = time.perf_counter()
                for _ in range(n):
                    res = run(pipes[0])
                return time.perf_counter() - t0, [res]
            last, t = timed(sync_loop, args.warmup, args.repeats, args.pairs)
            t.update(verify_ms=last[0][2]["verify_ms"], total_ms=last[0][1]["total_ms"])
            out["sync"] = t
            print("sync", json.dumps(t), flush=True)
        for n in IN_FLIGHT:
            if "queued" in what:
                sub = lambda p: p.submit_dlt_verified(MAX_PX, hypotheses=HYPOTHESES)
                wait = lambda p: p.wait_dlt_verified()
                last, t = timed(lambda k: stream(pipes[:n], sub, wait, k), args.warmup, args.repeats, args.pairs)
                same = all(summary(*r) == want for r in last)
                t.update(verify_ms=last[0][2]["verify_ms"], total_ms=last[0][1]["total_ms"], same_as_sync=same)
                out[f"queued_{n}"] = t
                print(f"queued_{n}", json.dumps(t), flush=True)
                if not same:
                    raise SystemExit(f"queued_{n}: not the synchronous call's counts and E")
            if "plain" in what:
                last, t = timed(lambda k: stream(pipes[:n], lambda p: p.submit_dlt(), lambda p: p.wait_dlt(), k),
                                args.warmup, args.repeats, args.pairs)
                t.update(total_ms=last[0][1]["total_ms"], matches=last[0][1]["matches"], inliers=last[0][0])
                out[f"plain_{n}"] = t
                print(f"plain_{n}", json.dumps(t), flush=True)
    finally:
        for c in ctxs:
            c.close()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
