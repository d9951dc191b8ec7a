"""Times fm3d_pipeline_describe against the four-call chain it replaces (fm3d_records_download ->
fm3d_features_frames -> fm3d_export_patches -> fm3d_extract_descriptors_from_patches) on identical
records in a device buffer, and the chunk sizes against each other.  DESIGN.md §3.5b quotes the file
this writes, profiles/describe_tail.json.

    python tools/time_describe.py [--points 10000 36143] [--repeats 15] [--chunks 1024 4096 16384]
                                  [--extractor SURF|SIFT|ORB] [--out profiles/describe_tail.json]

--extractor ORB (profiles/describe_tail_orb.json, default points 1000 10000) times three ways to the same
ORB rows, alternating: the chain with one fm3d_orb_compute per patch (what
fm3d_extract_descriptors_from_patches_any did for ORB before it was batched), the chain ending in the
batched fm3d_extract_descriptors_from_patches_any, and fm3d_pipeline_describe_any; and beside them
fm3d_pipeline_describe with SURF Extended 1, Upright 1 on a second context and the same records.

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


def orb_main(args, torch):
    """the three ORB paths and the SURF tail on the same records"""
    pair = synth.make_frame_pair(8, seed=11)
    s = fm3d.Settings.default()
    s.set_camera(pair.cam)
    s.extractorType = fm3d.FEAT_ORB
    ctx = fm3d.Context(s, device=0)
    s2 = fm3d.Settings.default()
    s2.set_camera(pair.cam)
    surf = fm3d.Context(s2, device=0)
    size = fm3d.NeighborhoodsGenerator(s).size()
    result = {"device": torch.cuda.get_device_name(0), "extractor": "ORB", "repeats": args.repeats, "patchSize": size,
              "sizes": []}
    try:
        for c in (ctx, surf):
            fm3d.NormalOptimizer(c).setImages(pair.img1, pair.img2)
        L, h, chk = fm3d.lib(), ctx.handle, ctx.check
        vp = lambda a: ctypes.c_void_p(a.ctypes.data)
        kp = np.zeros(1, dtype=fm3d.KEYPOINT)
        kp["x"] = kp["y"] = size // 2
        kp["size"], kp["angle"], kp["response"] = size, -1, 1
        ko, m = np.zeros(1, dtype=fm3d.KEYPOINT), ctypes.c_int(0)
        for n in args.points:
            rec = make_records(pair.cam, n, seed=n)
            dev = torch.from_numpy(np.frombuffer(rec.tobytes(), dtype=np.uint8).copy()).to("cuda:0")
            torch.cuda.synchronize()
            ptr = dev.data_ptr()
            rec_h, pts, nrm = np.zeros(n, dtype=fm3d.RECORD), np.zeros((n, 3)), np.zeros((n, 3))
            frames_h, patches_h = np.zeros((n, 16)), np.zeros((n, size, size), dtype=np.uint8)
            loop, one, got = (np.zeros((n, 32), dtype=np.uint8) for _ in range(3))
            fsurf = np.zeros((n, 128), dtype=np.float32)
            st, st2 = fm3d.DescribeStats(), fm3d.DescribeStats()

            def front():
                chk(L.fm3d_records_download(h, ctypes.c_void_p(ptr), n, vp(rec_h)))
                pts[:], nrm[:] = rec_h["point"], rec_h["normal"]
                chk(L.fm3d_features_frames(h, vp(pts), vp(nrm), n, vp(frames_h)))
                chk(L.fm3d_export_patches(h, vp(frames_h), n, vp(patches_h), None))

            def chain_loop():
                front()
                for p in range(n):
                    chk(L.fm3d_orb_compute(h, vp(patches_h[p]), size, size, vp(kp), 1, vp(ko), None, ctypes.byref(m),
                                           vp(loop[p])))
                    assert m.value == 1

            def chain_one():
                front()
                chk(L.fm3d_extract_descriptors_from_patches_any(h, vp(patches_h), n, size, vp(one)))

            def describe():
                chk(L.fm3d_pipeline_describe_any(h, 0, ctypes.c_void_p(ptr), n, vp(got), None, None, ctypes.byref(st)))

            def describe_surf():
                surf.check(L.fm3d_pipeline_describe(surf.handle, 0, ctypes.c_void_p(ptr), n, vp(fsurf), None, None,
                                                    ctypes.byref(st2)))

            sides = {"chain_loop_ms": chain_loop, "chain_one_shot_ms": chain_one, "describe_any_ms": describe,
                     "describe_surf_ms": describe_surf}
            for fn in sides.values():
                fn()  # the warm-up of each, and the comparison
            row = {"points": n, "chunks": st.chunks,
                   "equal": loop.tobytes() == one.tobytes() == got.tobytes() and bool(got.any())}
            t, dev_ms, surf_dev_ms = {k: [] for k in sides}, [], []
            for _ in range(args.repeats):
                for k, fn in sides.items():
                    t[k].append(timed(fn)[0])
                dev_ms.append(st.total_ms)
                surf_dev_ms.append(st2.total_ms)
            for k in sides:
                row[k] = spread(t[k])
            row["describe_any_device_ms"] = statistics.median(dev_ms)
            row["describe_surf_device_ms"] = statistics.median(surf_dev_ms)
            row["loop_over_one_shot"] = row["chain_loop_ms"]["median"] / row["chain_one_shot_ms"]["median"]
            row["loop_over_describe_any"] = row["chain_loop_ms"]["median"] / row["describe_any_ms"]["median"]
            result["sizes"].append(row)
            print(json.dumps(row), flush=True)
            del dev
    finally:
        ctx.close()
        surf.close()
    return result


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--points", type=int, nargs="+", default=None)
    ap.add_argument("--repeats", type=int, default=15)
    ap.add_argument("--chunks", type=int, nargs="+", default=[1024, 4096, 16384])
    ap.add_argument("--extractor", choices=("SURF", "SIFT", "ORB"), default="SURF")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    orb = args.extractor == "ORB"
    args.points = args.points or ([1_000, 10_000] if orb else [10_000, 36_143])
    args.out = args.out or os.path.join(ROOT, "profiles", "describe_tail_orb.json" if orb else "describe_tail.json")
    import torch
    if not torch.cuda.is_available():
        sys.exit("time_describe: no GPU")
    torch.cuda.init()  # before libfm3d initialises its own HIP runtime: torch's finds no GPU afterwards
    os.environ.pop("FM3D_DESCRIBE_CHUNK", None)
    if orb:
        return write(orb_main(args, torch), args.out)

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
    write(result, args.out)


def write(result, out):
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    with open(out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    print("wrote", out)


if __name__ == "__main__":
    main()
