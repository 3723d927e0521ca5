#!/usr/bin/env python3
"""Cost of signed distance queries on the default terrain at [scene] chunkDim 1 and 4
(60,800 and 958,720 triangles), timed by HIP events on the context stream around the calls.

  build_off / build_on   rt_build_bvh with rt_set_signed_distance off and on: the difference is the table
                         (k_sdf_triangles + k_sdf_gather) per LBVH build
  closest                rt_closest_points_device, 2^20 points
  distance               rt_signed_distance_device, the same points: the descent and the sign pass
  sign_pass              ... with RT_DISTANCE_FROM_RECORDS: k_sdf_sign alone

The points are those of tools/closest_probe.py's `near` set: points of random triangles moved by up to 1 %
of the scene's extent.  Each figure is the median of --samples launches, taken --repeats times; the variants
run in turn inside every sample, so that a drift of the machine meets them alike.  Writes
profiles/signed_distance.json.

Usage: python tools/sdf_probe.py [--points 1048576] [--samples 10] [--repeats 3] [--out PATH]"""
import argparse
import json
import os
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "real-time-ray-tracing_amd"), os.path.join(ROOT, "tools")]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--points", type=int, default=1 << 20)
    ap.add_argument("--samples", type=int, default=10)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "signed_distance.json"))
    a = ap.parse_args()

    import torch

    import rtx
    from closest_probe import point_sets

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
        rt.signed_distance = True
        rt.build_bvh()
        tri_count = rt.info().triCount
        tris = rt.download("TRI_POS", np.float32).reshape(-1, 3, 4)[:tri_count, :, :3]
        sets, ext = point_sets(tris, n)
        pts = torch.from_numpy(sets["near"]).to(dev)
        rec = torch.empty((n, 8), dtype=torch.float32, device=dev)
        sd = torch.empty((n, 4), dtype=torch.float32, device=dev)
        torch.cuda.synchronize()

        def timed(fn):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(stream)
            fn()
            e1.record(stream)
            stream.synchronize()
            return e0.elapsed_time(e1)

        def build(on):
            def run():
                if rt.signed_distance != on:
                    rt.signed_distance = on  # waits for the streams, outside the events
                return timed(rt.build_bvh)
            return run

        def query(**kw):
            return lambda: timed(lambda: rt.signed_distance_device(pts.data_ptr(), n, rec.data_ptr(), sd.data_ptr(), **kw))

        def closest():
            return timed(lambda: rt.closest_points_device(pts.data_ptr(), n, rec.data_ptr()))

        # build_on last: the queries of the next sample need the table of the current build
        variants = dict(closest=closest, distance=query(), sign_pass=query(from_records=True), build_off=build(False),
                        build_on=build(True))
        runs = {k: [] for k in variants}
        for _ in range(a.repeats):
            ms = {k: [] for k in variants}
            for s in range(a.samples + 2):
                for k, fn in variants.items():
                    t = fn()
                    if s >= 2:
                        ms[k].append(t)
            for k in variants:
                runs[k].append(float(np.median(ms[k])))
        inside = float((sd[:, 3] < 0).float().mean())
        rt.cleanup()
        scene = dict(triangles=int(tri_count), extent=ext, inside_share=inside)
        for k in variants:
            scene[k] = dict(ms_runs=runs[k], ms=float(np.median(runs[k])))
            print("%7d triangles  %-10s %8.3f ms  (runs %s)" % (tri_count, k, scene[k]["ms"], ", ".join("%.3f" % x for x in runs[k])))
        scene["table_ms"] = scene["build_on"]["ms"] - scene["build_off"]["ms"]
        print("%7d triangles  table per build %.3f ms" % (tri_count, scene["table_ms"]))
        out["scenes"][str(int(tri_count))] = scene
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
