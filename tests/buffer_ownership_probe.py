"""Free device memory around repeated library calls and context life cycles, printed as one JSON line
(run as a script by tests/test_gpu_buffer_ownership.py; not a test module).

A process of its own, and torch initialised in it before libfm3d: torch brings its own HIP runtime,
which finds no GPU in a process where libfm3d has initialised the one it is linked to first, as
every earlier test of a suite run has.  Free memory is hipMemGetInfo's, device-wide, so it sees the
library's own hipMalloc."""
import importlib
import json
import os
import sys

import numpy as np
import torch

MIB = 1 << 20
CYCLES = (10, 100)  # context life cycles after the warm-up one at which free memory is read


def free():
    torch.cuda.synchronize(0)
    return torch.cuda.mem_get_info(0)[0]


def temporaries(fm3d):
    """fm3d_square_neighborhoods holds its frames and its output in two local device buffers; the
    frames' output is under the function's 512 MiB chunk bound, so one buffer of that size per call."""
    s = fm3d.Settings.default()
    gen = fm3d.NeighborhoodsGenerator(s)
    P = (256 * MIB) // (gen.size() ** 2 * 24)
    frames = np.tile(np.eye(4).reshape(1, 16), (P, 1))  # identity frames: the values do not matter here
    ctx = fm3d.Context(s, device=0)
    try:
        gen.computeSquareNeighborhoodsByNormals(ctx, frames)  # warm-up: code objects, the runtime's own blocks
        before = free()
        for _ in range(6):
            out = gen.computeSquareNeighborhoodsByNormals(ctx, frames)
        after = free()
    finally:
        ctx.close()
    return {"size": gen.size(), "P": P, "shape": list(out.shape), "before": before, "after": after}


def contexts(fm3d, synth):
    """create -> set_g12 -> upload -> run -> close, over and over on one frame pair"""
    pair = synth.make_frame_pair(400, seed=2)
    s = fm3d.Settings.default()
    s.set_camera(pair.cam)
    s.pixelsRay = 16

    def cycle():
        ctx = fm3d.Context(s, device=0)
        try:
            fm3d.SingleCameraTriangulator(ctx).set_g12(pair.g12)
            pipe = fm3d.Pipeline(ctx)
            pipe.upload(pair.desc1, pair.desc2, pair.kp1, pair.kp2, pair.img1, pair.img2)
            return pipe.run()[0]
        finally:
            ctx.close()

    kept = [cycle()]  # warm-up
    before = free()
    after = {}
    for n in range(1, max(CYCLES) + 1):
        kept.append(cycle())
        if n in CYCLES:
            after[str(n)] = free()
    return {"kept": kept, "before": before, "after": after}


if __name__ == "__main__":
    torch.cuda.init()
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    pkg = importlib.import_module("3dfeaturematcher_amd")
    print(json.dumps({"temporaries": temporaries(pkg),
                      "contexts": contexts(pkg, importlib.import_module("3dfeaturematcher_amd.synth"))}))
