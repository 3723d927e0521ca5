#!/usr/bin/env python3
"""Cost of a surface query: 2^20 rays of the query tests' recipe (tools/query_probe.py)
on the default scene, on the 1920x1080 4-spp context of that probe, timed by HIP events on the context
stream around

  trace     rt_trace_rays_device, closest hit (the 512-B counter memset and k_trace_rays);
  surface   rt_trace_surfaces_device with RT_SURFACE_FROM_HITS: k_ray_surface alone, over the records
            of the trace; with and without RT_SURFACE_MOTION;
  fused     rt_trace_surfaces_device: the trace and the pass behind it.

The three are taken in turn inside every sample, so that a drift of the machine meets them alike.  Each
figure is the median of --samples rounds, taken --repeats times; the spread of the repeats is what a
difference has to exceed.  Bytes per ray are the bytes the pass needs, counted from the shapes: 40 B of
rays and record in, 48 B (64 B) out, and per hit the gathered 48 B triangle record, 48 B of normals, the
id byte when a table is set, 48 B of displacements with motion; the bandwidth is those bytes over the
pass's time (gathers of triangles that several rays hit are counted once per ray).
Writes profiles/surface_query.json.

Usage: python tools/surface_probe.py [--rays 1048576] [--samples 10] [--repeats 3] [--out PATH]"""
import argparse
import json
import os
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "real-time-ray-tracing_amd"), os.path.join(ROOT, "tools")]

from query_probe import make_rays  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rays", type=int, default=1 << 20)
    ap.add_argument("--samples", type=int, default=10)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "surface_query.json"))
    a = ap.parse_args()

    import torch

    import rtx

    w, h, n = 1920, 1080, a.rays
    cfg = rtx.write_config(os.path.join(tempfile.mkdtemp(), "s.toml"), w, h, spp=4, geometry_motion=True)
    rt = rtx.RayTracer(w, h, cfg).init()
    dev = torch.device("cuda", 0)
    stream = torch.cuda.Stream(dev)
    torch.cuda.set_stream(stream)
    rt.set_stream(stream.cuda_stream)
    rt.build_bvh()
    verts = rt.download("VERTICES", np.float32).reshape(-1, 3).copy()
    rt.update_vertices(verts)  # a second build, which records a displacement (of zeros): the motion quad gathers
    rt.build_bvh()
    org, d = make_rays(verts, n)
    dorg, ddir = torch.from_numpy(org).to(dev), torch.from_numpy(d).to(dev)
    hits = torch.empty((n, 4), dtype=torch.float32, device=dev)
    hits2 = torch.empty((n, 4), dtype=torch.float32, device=dev)
    surf = {m: torch.empty((n, 16 if m else 12), dtype=torch.float32, device=dev) for m in (False, True)}
    surf2 = torch.empty((n, 12), dtype=torch.float32, device=dev)
    torch.cuda.synchronize()
    ptr = (dorg.data_ptr(), ddir.data_ptr(), n)

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(stream)
        fn()
        e1.record(stream)
        stream.synchronize()
        return e0.elapsed_time(e1)

    variants = dict(
        trace=lambda: rt.trace_rays_device(*ptr, hits.data_ptr()),
        surface=lambda: rt.trace_surfaces_device(*ptr, hits.data_ptr(), surf[False].data_ptr(), from_hits=True),
        surface_motion=lambda: rt.trace_surfaces_device(*ptr, hits.data_ptr(), surf[True].data_ptr(), from_hits=True,
                                                        motion=True),
        fused=lambda: rt.trace_surfaces_device(*ptr, hits2.data_ptr(), surf2.data_ptr()),
    )
    runs = {k: [] for k in variants}
    for _ in range(a.repeats):
        ms = {k: [] for k in variants}
        for s in range(a.samples + 2):
            for k, fn in variants.items():  # in turn: trace first, its records feed the pass
                t = timed(fn)
                if s >= 2:
                    ms[k].append(t)
        for k in variants:
            runs[k].append(float(np.median(ms[k])))

    tri = hits.cpu().numpy()[:, 1].view(np.int32)
    share = float((tri >= 0).mean())
    same = bool(torch.equal(hits.view(torch.int32), hits2.view(torch.int32))
                and torch.equal(surf[False].view(torch.int32), surf2.view(torch.int32))
                and torch.equal(surf[True].view(torch.int32)[:, :12], surf2.view(torch.int32)))
    rt.cleanup()
    out = dict(rays=n, samples=a.samples, repeats=a.repeats, device=torch.cuda.get_device_name(0), hit_share=share,
               distinct_triangles=int(len(np.unique(tri[tri >= 0]))), fused_equals_two_calls=same)
    for k in variants:
        out[k] = dict(ms_runs=runs[k], ms=float(np.median(runs[k])))
    for k, motion in (("surface", False), ("surface_motion", True)):
        per_ray = 40.0 + (64.0 if motion else 48.0) + share * (96.0 + (48.0 if motion else 0.0))
        out[k].update(bytes_per_ray=per_ray, gb_s=per_ray * n / out[k]["ms"] / 1e6)
    out["fused_minus_trace_ms"] = out["fused"]["ms"] - out["trace"]["ms"]
    for k in variants:
        r = out[k]
        print("%-15s %.3f ms (runs %s)%s" % (k, r["ms"], ", ".join("%.3f" % x for x in r["ms_runs"]),
                                             "  %.1f B/ray  %.0f GB/s" % (r["bytes_per_ray"], r["gb_s"]) if "gb_s" in r else ""))
    print("hit share %.3f, %d distinct triangles, fused equals the two calls: %s" % (share, out["distinct_triangles"], same))
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
    if not same:
        sys.exit("the fused call and trace + RT_SURFACE_FROM_HITS disagree")


if __name__ == "__main__":
    main()
