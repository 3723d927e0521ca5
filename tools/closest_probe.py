#!/usr/bin/env python3
"""Throughput of closest-point queries: 2^20 points against the default terrain at
[scene] chunkDim 1 and 4 (60,800 and 958,720 triangles), timed by HIP events on the context stream around
rt_closest_points_device (k_closest_points alone: the call enqueues nothing else).

Two point sets: `near`, points of random triangles moved by up to 1 % of the scene's extent (a collider
or a foot near the ground), and `box`, uniform in the scene's box grown by its extent on every side (a
distance-field sample).  Each with max_distance infinite and 1 % of the extent.  Each figure is the median
of --samples launches, taken --repeats times; the variants run in turn inside every sample, so that a
drift of the machine meets them alike.  Writes Mpoints/s to profiles/closest_points.json.

Usage: python tools/closest_probe.py [--points 1048576] [--samples 10] [--repeats 3] [--out PATH]"""
import argparse
import json
import os
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "real-time-ray-tracing_amd")]


def point_sets(tris, n, seed=29):
    rng = np.random.default_rng(seed)
    flat = tris.reshape(-1, 3).astype(np.float64)
    lo, hi = flat.min(0), flat.max(0)
    ext = float(np.linalg.norm(hi - lo))
    pick = tris[rng.integers(0, len(tris), n)].astype(np.float64)
    w = rng.dirichlet((1.0, 1.0, 1.0), n)
    near = np.einsum("nk,nkc->nc", w, pick) + rng.uniform(-0.01, 0.01, (n, 3)) * ext
    box = rng.uniform(lo - ext, hi + ext, (n, 3))
    return dict(near=near.astype(np.float32), box=box.astype(np.float32)), ext


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--points", type=int, default=1 << 20)
    ap.add_argument("--samples", type=int, default=10)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "closest_points.json"))
    a = ap.parse_args()

    import torch

    import rtx

    n = a.points
    dev = torch.device("cuda", 0)
    out = dict(points=n, samples=a.samples, repeats=a.repeats, device=torch.cuda.get_device_name(0), scenes={})
    for chunk_dim in (1, 4):
        w, h = 640, 360
        cfg = rtx.write_config(os.path.join(tempfile.mkdtemp(), "c.toml"), w, h, chunk_dim=chunk_dim)
        rt = rtx.RayTracer(w, h, cfg).init()
        stream = torch.cuda.Stream(dev)
        torch.cuda.set_stream(stream)
        rt.set_stream(stream.cuda_stream)
        rt.build_bvh()
        tri_count = rt.info().triCount
        tris = rt.download("TRI_POS", np.float32).reshape(-1, 3, 4)[:tri_count, :, :3]
        sets, ext = point_sets(tris, n)
        dpts = {k: torch.from_numpy(v).to(dev) for k, v in sets.items()}
        rec = torch.empty((n, 8), dtype=torch.float32, device=dev)
        torch.cuda.synchronize()

        def timed(fn):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(stream)
            fn()
            e1.record(stream)
            stream.synchronize()
            return e0.elapsed_time(e1)

        variants = {}
        for k in ("near", "box"):
            for name, md in (("inf", float("inf")), ("1pct", 0.01 * ext)):
                variants["%s_%s" % (k, name)] = (dpts[k], md)
        runs = {k: [] for k in variants}
        found = {}
        for _ in range(a.repeats):
            ms = {k: [] for k in variants}
            for s in range(a.samples + 2):
                for k, (p, md) in variants.items():
                    t = timed(lambda: rt.closest_points_device(p.data_ptr(), n, rec.data_ptr(), max_distance=md))
                    if s >= 2:
                        ms[k].append(t)
                    if s == 0:
                        found[k] = float(((rec.view(torch.int32)[:, 7] & (1 << 17)) != 0).float().mean())
            for k in variants:
                runs[k].append(float(np.median(ms[k])))
        rt.cleanup()
        scene = dict(triangles=int(tri_count), extent=ext)
        for k in variants:
            med = float(np.median(runs[k]))
            scene[k] = dict(ms_runs=runs[k], ms=med, mpoints_s=n / med / 1e3, found_share=found[k])
            print("%7d triangles  %-9s %8.3f ms  %8.1f Mpoints/s  (runs %s; found %.3f)" % (
                tri_count, k, med, scene[k]["mpoints_s"], ", ".join("%.3f" % x for x in runs[k]), found[k]))
        out["scenes"][str(int(tri_count))] = scene
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
