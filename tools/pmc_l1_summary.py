"""Summarise the texture-addresser / vector-L1 counter passes of one resident C4 launch (separate
rocprofv3 --pmc passes of `bench.py --mode resident --steps 2 --warmup 1 --no-cpu`, no tracing) for
lm2_kernel: counters per launch, L1 requests and L2->L1 bytes per pixel evaluation.

    python tools/pmc_l1_summary.py DIR --layout rows|cols [--levels level_share.json] [--out profiles/x.json]

DIR holds pmc*/run_counter_collection.csv and log.txt (the bench lines); level_share.json is the
output of tools/lm_level_share.py (evaluations per pyramid level, pixel evaluations of the launch).
"""
import csv
import glob
import json
import os
import re
import sys

L1_LINE = 128  # bytes per vector-L1 line and per TCP -> TCC read request on gfx950 (MI355X_MICROARCH.md)


def main():
    d = sys.argv[1]
    arg = lambda k: sys.argv[sys.argv.index(k) + 1] if k in sys.argv else None
    agg, n = {}, {}
    for f in sorted(glob.glob(os.path.join(d, "pmc*", "*counter_collection.csv"))):
        for r in csv.DictReader(open(f)):
            if "lm2_kernel" in r["Kernel_Name"]:
                c = r["Counter_Name"]
                agg[c] = agg.get(c, 0.0) + float(r["Counter_Value"])
                n.setdefault(c, set()).add(r["Dispatch_Id"])
                kernel = r["Kernel_Name"]
    agg = {c: v / len(n[c]) for c, v in agg.items()}
    log = open(os.path.join(d, "log.txt")).read()
    # the launch's pixel evaluations: the same points and counts in every run of the workload (--levels:
    # the per-level evaluation counts and the LM counters of the same points through fm3d_optimize_normals)
    levels = json.load(open(arg("--levels"))) if arg("--levels") else None
    pix = [float(levels["lm_stats"]["pixel_evaluations"])] if levels else []
    lm_ms = [float(x) for x in re.findall(r'"lm_ms": ([0-9.e+]+)', log)]
    res = {"kernel": kernel, "img2_layout": arg("--layout"), "launches": max(len(v) for v in n.values()),
           "counters_per_launch": agg, "pixel_evaluations_per_launch": pix[-1] if pix else None,
           "lm_ms_under_the_profiler": lm_ms}
    if pix:
        p = pix[-1]
        res["per_pixel_evaluation"] = {
            "l1_requests": agg.get("TCP_TOTAL_CACHE_ACCESSES_sum", 0) / p,
            "l2_to_l1_read_requests": agg.get("TCP_TCC_READ_REQ_sum", 0) / p,
            "l2_to_l1_bytes": agg.get("TCP_TCC_READ_REQ_sum", 0) * L1_LINE / p,
        }
    if "SQ_BUSY_CYCLES" in agg and "TA_TA_BUSY_sum" in agg:
        # SQ_BUSY_CYCLES sums 32 shader engines' busy cycles; TA_TA_BUSY_sum the 256 CUs' texture addressers
        cyc = agg["SQ_BUSY_CYCLES"] / 32
        res["busy_cycles"] = cyc
        res["ta_busy_frac"] = agg["TA_TA_BUSY_sum"] / (256 * cyc)
        for k in ("TA_ADDR_STALLED_BY_TC_CYCLES_sum", "TA_DATA_STALLED_BY_TC_CYCLES_sum", "TCP_PENDING_STALL_CYCLES_sum",
                  "TCP_TCP_TA_DATA_STALL_CYCLES_sum", "TCP_READ_TAGCONFLICT_STALL_CYCLES_sum"):
            if k in agg:
                res[k[:-4].lower() + "_frac"] = agg[k] / (256 * cyc)
        if "TCP_TOTAL_CACHE_ACCESSES_sum" in agg:
            res["l1_requests_per_cu_cycle"] = agg["TCP_TOTAL_CACHE_ACCESSES_sum"] / (256 * cyc)
    if levels:
        res["evaluations_per_level"] = levels
    res["command"] = ("bench.py --mode resident --steps 2 --warmup 1 --no-cpu under rocprofv3 --pmc, one pass per counter "
                      "group, FM3D_LM_IMG2=" + str(arg("--layout")))
    print(json.dumps(res, indent=1))
    if arg("--out"):
        with open(arg("--out"), "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
