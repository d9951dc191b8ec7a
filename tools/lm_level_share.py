"""Share of the LM's residual evaluations per pyramid level on the C4 frame pair: the front half
through the pipeline, the inliers through fm3d_optimize_normals, nfev summed per level.

    python tools/lm_level_share.py [--out level_share.json]

The output feeds tools/pmc_l1_summary.py --levels (pixel evaluations of the launch, level weights)."""
import importlib
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402  (the workload table)


def main():
    fm3d = importlib.import_module("3dfeaturematcher_amd")
    synth = importlib.import_module("3dfeaturematcher_amd.synth")
    wl, df = bench.WORKLOADS["c4"], bench.WORKLOAD_DEFAULTS["c4"]
    pair = synth.make_frame_pair(wl["keypoints"], wl["width"], wl["height"], seed=df["seed"], desc="sift")
    s = fm3d.Settings.default()
    s.set_camera(pair.cam)
    s.pixelsRay, s.nndrEpsilon, s.pyramids = df["ray"], df["nndr"], 3
    ctx = fm3d.Context(s, device=0)
    try:
        sct = fm3d.SingleCameraTriangulator(ctx)
        sct.set_g12(pair.g12)
        pipe = fm3d.Pipeline(ctx)
        pipe.upload(pair.desc1, pair.desc2, pair.kp1, pair.kp2, pair.img1, pair.img2)
        n, st = pipe.run_dlt()
        pts = pipe.dlt_results(st["matches"], n)[1]
        no = fm3d.NormalOptimizer(ctx, sct)
        no.setImages(pair.img1, pair.img2)
        kept, _ = no.computeOptimizedNormals(pts)
        tot = no.last_nfev.astype(np.int64).sum(axis=0)[:s.pyramids + 1]
        out = {"points": int(len(pts)), "kept": int(len(kept)), "nfev_per_level": tot.tolist(),
               "share_per_level": (tot / tot.sum()).round(4).tolist(),
               "lm_stats": {k: no.last_stats[k] for k in ("evaluations", "pixel_evaluations", "kernel_ms")}}
    finally:
        ctx.close()
    print(json.dumps(out))
    if "--out" in sys.argv:
        with open(sys.argv[sys.argv.index("--out") + 1], "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
