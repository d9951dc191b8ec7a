"""Times fm3d_pipeline_describe against the four-call chain it replaces (fm3d_records_download ->
fm3d_features_frames -> fm3d_export_patches -> fm3d_extract_descriptors_from_patches) on identical
records in a device buffer, and the chunk sizes against each other.  DESIGN.md §3.5b quotes the file
this writes, profiles/describe_tail.json.

    python tools/time_describe.py [--points 10000 36143] [--repeats 15] [--chunks 1024 4096 16384]
                                  [--extractor SURF|SIFT] [--out profiles/describe_tail.json]

Inputs: synthetic records -- points in front of the 640 x 480 camera of the synthetic frame pair at
1.5 .. 2.4 m, each normal the viewing ray turned back at the camera and jittered -- written to a torch
tensor on the device; image 1 of that pair; the default settings (128 x 128 patches, SURF Extended 1,
Upright 1).

What is measured: the host clock around the C calls themselves (through ctypes; every one ends in a
device synchronise), after one warm-up of each, the two alternating, `repeats` times; median, minimum
and maximum.  Every host buffer is allocated once per size and reused by both sides: a large pageable
array that the runtime pinned for a copy and the caller then freed costs the next GPU call, whichever
it is, tens of milliseconds on some hosts, which belongs to neither side.  describe_device_ms is the
call's own stats.total_ms (HIP events).  desc_d2h_ms is a copy of the descriptor rows' byte count from
the device to pageable host memory timed on its own (torch), and d2h_share its share of the median
call.  The outputs of the two are compared as bytes at every timed size.  Needs a GPU: there is no
fall-back."""
import argparse
import ctypes
import importlib
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
fm3d = importlib.import_module("3dfeaturematcher_amd")
synth = importlib.import_module("3dfeaturematcher_amd.synth")


def make_records(cam, n, seed):
    """n records: pixel uniform in the image, depth 1.5 .. 2.4 m along the pinhole ray; the normal is the
    ray reversed plus N(0, 0.15) per component, normalised"""
    rng = np.random.default_rng(seed)
    u = rng.uniform(40, 600, n)
    v = rng.uniform(40, 440, n)
    z = rng.uniform(1.5, 2.4, n)
    pts = np.stack([(u - cam.cx) / cam.fx * z, (v - cam.cy) / cam.fy * z, z], axis=1)
    nrm = -pts / np.linalg.norm(pts, axis=1, keepdims=True) + rng.normal(0, 0.15, (n, 3))
    nrm /= np.linalg.norm(nrm, axis=1, keepdims=True)
    rec = np.zeros(n, dtype=fm3d.RECORD)
    rec["queryIdx"] = rec["trainIdx"] = np.arange(n)
    rec["point"], rec["normal"] = pts, nrm
    return rec


def spread(ms):
    return {"median": statistics.median(ms), "min": min(ms), "max": max(ms)}


def timed(fn):
    t0 = time.perf_counter()
    out = fn()
    return 1e3 * (time.perf_counter() - t0), out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--points", type=int, nargs="+", default=[10_000, 36_143])
    ap.add_argument("--repeats", type=int, default=15)
    ap.add_argument("--chunks", type=int, nargs="+", default=[1024, 4096, 16384])
    ap.add_argument("--extractor", choices=("SURF", "SIFT"), default="SURF")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "describe_tail.json"))
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        sys.exit("time_describe: no GPU")
    torch.cuda.init()  # before libfm3d initialises its own HIP runtime: torch's finds no GPU afterwards
    os.environ.pop("FM3D_DESCRIBE_CHUNK", None)

    pair = synth.make_frame_pair(8, seed=11)
    s = fm3d.Settings.default()
    s.set_camera(pair.cam)
    s.extractorType = getattr(fm3d, "FEAT_" + args.extractor)
    ctx = fm3d.Context(s, device=0)
    result = {"device": torch.cuda.get_device_name(0), "extractor": args.extractor, "repeats": args.repeats,
              "patchSize": fm3d.NeighborhoodsGenerator(s).size(), "sizes": []}
    try:
        feat = fm3d.Features(ctx)
        fm3d.NormalOptimizer(ctx).setImages(pair.img1, pair.img2)
        for n in args.points:
            rec = make_records(pair.cam, n, seed=n)
            dev = torch.from_numpy(np.frombuffer(rec.tobytes(), dtype=np.uint8).copy()).to("cuda:0")
            torch.cuda.synchronize()
            ptr = dev.data_ptr()

            L, h, chk = fm3d.lib(), ctx.handle, ctx.check
            size, cols = result["patchSize"], feat.descriptor_info()[0]
            vp = lambda a: ctypes.c_void_p(a.ctypes.data)
            rec_h, pts, nrm = np.zeros(n, dtype=fm3d.RECORD), np.zeros((n, 3)), np.zeros((n, 3))
            frames_h, patches_h = np.zeros((n, 16)), np.zeros((n, size, size), dtype=np.uint8)
            ref, got = np.zeros((n, cols), dtype=np.float32), np.zeros((n, cols), dtype=np.float32)
            st = fm3d.DescribeStats()

            def chain():
                chk(L.fm3d_records_download(h, ctypes.c_void_p(ptr), n, vp(rec_h)))
                pts[:], nrm[:] = rec_h["point"], rec_h["normal"]  # the one-shot calls take rows, not records
                chk(L.fm3d_features_frames(h, vp(pts), vp(nrm), n, vp(frames_h)))
                chk(L.fm3d_export_patches(h, vp(frames_h), n, vp(patches_h), None))
                chk(L.fm3d_extract_descriptors_from_patches(h, vp(patches_h), n, size, vp(ref)))

            def describe():
                chk(L.fm3d_pipeline_describe(h, 0, ctypes.c_void_p(ptr), n, vp(got), None, None, ctypes.byref(st)))

            chain(), describe()  # the warm-up of both, and the comparison
            row = {"points": n, "chunks": st.chunks, "equal": got.tobytes() == ref.tobytes()}
            tc, td, dev_ms = [], [], []
            for _ in range(args.repeats):
                tc.append(timed(chain)[0])
                td.append(timed(describe)[0])
                dev_ms.append(st.total_ms)
            row["chain_ms"], row["describe_ms"] = spread(tc), spread(td)
            row["describe_device_ms"] = statistics.median(dev_ms)
            row["chain_over_describe"] = row["chain_ms"]["median"] / row["describe_ms"]["median"]
            # the final D2H on its own: the same bytes, device -> pageable host
            src = torch.zeros(got.nbytes, dtype=torch.uint8, device="cuda:0")
            dst = torch.from_numpy(np.zeros(got.nbytes, dtype=np.uint8))
            dst.copy_(src)
            cp = []
            for _ in range(args.repeats):
                torch.cuda.synchronize()
                cp.append(timed(lambda: (dst.copy_(src), torch.cuda.synchronize()))[0])
            row["desc_bytes"] = int(got.nbytes)
            row["desc_d2h_ms"] = statistics.median(cp)
            row["d2h_share"] = row["desc_d2h_ms"] / row["describe_ms"]["median"]
            # the chunk sizes, alternating, each warmed up first (the first call at a size grows the buffers)
            times = {c: [] for c in args.chunks}
            for c in args.chunks:
                os.environ["FM3D_DESCRIBE_CHUNK"] = str(c)
                got[:] = 0
                describe()
                assert got.tobytes() == ref.tobytes(), c
            for _ in range(args.repeats):
                for c in args.chunks:
                    os.environ["FM3D_DESCRIBE_CHUNK"] = str(c)
                    times[c].append(timed(describe)[0])
            os.environ.pop("FM3D_DESCRIBE_CHUNK", None)
            row["chunks_ms"] = {str(c): spread(t) for c, t in times.items()}
            result["sizes"].append(row)
            print(json.dumps(row), flush=True)
            del dev, src
    finally:
        ctx.close()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    print("wrote", args.out)


if __name__ == "__main__":
    main()
