#!/usr/bin/env python3
"""Cost of emitter sampling on the GPU (rt_set_emitter_sampling).

  list build   the default terrain at [scene] chunkDim 1 and 4 (60,800 and 958,720 triangles), a quarter of
               the triangles on an emitting id (hashed over the mesh): --builds LBVH builds enqueued back to
               back and waited for once, with sampling off and on in turn in ONE context, --repeats times;
               medians of ms per build, and their difference: the list's five launches behind the build
  frame        pipelined 1080p 4-spp frames on bench.py's terrain camera under that table, sampling off and
               on (q = 0.5) in turn in one context; medians of ms per frame

Neither has a pass mark: they are the feature's cost, stated.  Writes profiles/emitter_sampling.json.

Usage: python tools/emitter_probe.py [--builds 200] [--frames 100] [--repeats 5] [--out PATH]"""
import argparse
import json
import os
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "real-time-ray-tracing_amd")]

TERRAIN_CAM = dict(pos=(8.0, 15.0, -6.0), yaw=0.0, pitch=-0.7)  # bench.py's
EMISSION = (1.0, 0.8, 0.6)


def hashed(n, palette):
    k = (np.arange(n, dtype=np.uint64) * np.uint64(2654435761)) >> np.uint64(7)
    return np.asarray(palette, np.uint8)[(k % np.uint64(len(palette))).astype(np.int64)]


def context(rtx, w, h, spp, chunk):
    rt = rtx.RayTracer(w, h, rtx.write_config(os.path.join(tempfile.mkdtemp(), "e.toml"), w, h, spp=spp, chunk_dim=chunk)).init()
    rt.set_delta_time(16.667)
    cam = rt.camera
    cam.pos[:] = TERRAIN_CAM["pos"]
    cam.yaw, cam.pitch = TERRAIN_CAM["yaw"], TERRAIN_CAM["pitch"]
    rt.camera = cam
    n = int(rt.info().triCount)
    rt.set_triangle_materials(hashed(n, (3, 3, 3, 0)))
    m = rtx.default_material(0)
    m.emission[:] = EMISSION
    rt.set_materials(0, [m])
    return rt, n


def list_build(rtx, chunk, builds, repeats):
    rt, n = context(rtx, 256, 144, 1, chunk)
    try:
        series = {False: [], True: []}
        for _ in range(repeats):
            for on in (False, True):
                rt.set_emitter_sampling(on, 0.5)
                for _ in range(10):
                    rt.build_bvh()
                rt.sync()
                t0 = time.perf_counter()
                for _ in range(builds):
                    rt.build_bvh()
                rt.sync()
                series[on].append((time.perf_counter() - t0) * 1e3 / builds)
        emitters = int(rt.download("EMITTER_TRIS", np.uint32).size)
        cdf_len = int(rt.download("EMITTER_CDF", np.float32).size)
    finally:
        rt.cleanup()
    off, on = float(np.median(series[False])), float(np.median(series[True]))
    return dict(chunk_dim=chunk, triangles=n, emitters=emitters, cdf_length=cdf_len, builds=builds,
                build_ms_off=off, build_ms_on=on, list_ms=on - off, series_off=series[False], series_on=series[True])


def frame(rtx, frames, repeats, warmup=20):
    import torch

    from rtx.frames import FramePipeline

    rt, n = context(rtx, 1920, 1080, 4, 1)
    try:
        fp = FramePipeline(rt, torch.device("cuda", 0), pipelined=True)
        state = dict(f=0)

        def run(k):
            for _ in range(k):
                state["f"] += 1
                fp.frame(state["f"])
            fp.finish()

        series = {False: [], True: []}
        for _ in range(repeats):
            for on in (False, True):
                rt.set_emitter_sampling(on, 0.5)
                run(warmup)
                t0 = time.perf_counter()
                run(frames)
                series[on].append((time.perf_counter() - t0) * 1e3 / frames)
        queue = rt.download("PT_QUEUE", np.uint32)
    finally:
        rt.cleanup()
    off, on = float(np.median(series[False])), float(np.median(series[True]))
    return dict(width=1920, height=1080, spp=4, triangles=n, q=0.5, frames=frames, frame_ms_off=off, frame_ms_on=on,
                series_off=series[False], series_on=series[True], queue3_on=int(queue[0]), queue4_on=int(queue[1]))


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--builds", type=int, default=200)
    ap.add_argument("--frames", type=int, default=100)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "emitter_sampling.json"))
    a = ap.parse_args()
    import rtx

    out = dict(list_build=[list_build(rtx, c, a.builds, a.repeats) for c in (1, 4)], frame=frame(rtx, a.frames, a.repeats))
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
