#!/usr/bin/env python3
"""Cost of a batch ray query: 1 M rays of the query tests' recipe (origins uniform
in [-40, 100]^3 aimed at points of the vertex AABB, the first eighth with one direction component
zeroed) on the default scene, traced

  (a) by rt_trace_rays: host arrays, repacked and staged in the path tracer's queue 3, on a
      1920x1080 4-spp context (whose queue capacity allows 1 M rays); kernel time from its kernel_ms
      (k_trace_queue<3> alone), wall time of the whole call;
  (b) by rt_trace_rays_device, closest hit and any hit: device tensors, HIP events around the call
      on the context stream (the 512-B counter memset and k_trace_rays), wall time from the call to
      the end of a stream synchronisation.

Each figure is the median of --samples calls, taken --repeats times; the spread of the repeats is
what a difference between (a) and (b) has to exceed.  The records of (a) and (b) are compared.
Writes profiles/query_probe.json.

Usage: python tools/query_probe.py [--rays 1048576] [--samples 10] [--repeats 3] [--out PATH]"""
import argparse
import json
import os
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "real-time-ray-tracing_amd")]


def make_rays(vertices, n, seed=11):
    rng = np.random.default_rng(seed)
    org = rng.uniform(-40.0, 100.0, (n, 3)).astype(np.float32)
    tgt = rng.uniform(vertices.min(0), vertices.max(0), (n, 3)).astype(np.float32)
    d = tgt - org
    k = n // 8
    d[np.arange(k), rng.integers(0, 3, k)] = 0.0
    d /= np.linalg.norm(d, axis=1, keepdims=True).astype(np.float32)
    return org, d


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rays", type=int, default=1 << 20)
    ap.add_argument("--samples", type=int, default=10)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "query_probe.json"))
    a = ap.parse_args()

    import torch

    import rtx

    w, h, n = 1920, 1080, a.rays
    rt = rtx.RayTracer(w, h, rtx.write_config(os.path.join(tempfile.mkdtemp(), "q.toml"), w, h, spp=4)).init()
    dev = torch.device("cuda", 0)
    stream = torch.cuda.Stream(dev)
    torch.cuda.set_stream(stream)
    rt.set_stream(stream.cuda_stream)
    rt.build_bvh()
    verts = rt.download("VERTICES", np.float32).reshape(-1, 3)
    org, d = make_rays(verts, n)
    dorg, ddir = torch.from_numpy(org).to(dev), torch.from_numpy(d).to(dev)
    hits = torch.empty((n, 4), dtype=torch.float32, device=dev)
    torch.cuda.synchronize()

    def host_call():
        t0 = time.perf_counter()
        t, tri, u, v, ms = rt.trace_rays(org, d)
        return ms, (time.perf_counter() - t0) * 1e3, (t, tri, u, v)

    def device_call(any_hit):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0 = time.perf_counter()
        e0.record(stream)
        rt.trace_rays_device(dorg.data_ptr(), ddir.data_ptr(), n, hits.data_ptr(), any_hit=any_hit)
        e1.record(stream)
        stream.synchronize()
        wall = (time.perf_counter() - t0) * 1e3
        return e0.elapsed_time(e1), wall, None

    def series(fn):
        runs = []
        for _ in range(a.repeats):
            ms, wall = [], []
            for k in range(a.samples + 2):
                m, wl, _ = fn()
                if k >= 2:
                    ms.append(m)
                    wall.append(wl)
            runs.append((float(np.median(ms)), float(np.median(wall))))
        k = [r[0] for r in runs]
        wl = [r[1] for r in runs]
        return dict(kernel_ms_runs=k, wall_ms_runs=wl, kernel_ms=float(np.median(k)), wall_ms=float(np.median(wl)),
                    mray_s=n / float(np.median(k)) / 1e3)

    out = dict(rays=n, samples=a.samples, repeats=a.repeats, device=torch.cuda.get_device_name(0))
    _, _, ref = host_call()
    device_call(False)
    got = hits.cpu().numpy()
    same = (np.array_equal(got[:, 0].view(np.uint32), ref[0].view(np.uint32)) and np.array_equal(got[:, 1].view(np.int32), ref[1])
            and np.array_equal(got[:, 2].view(np.uint32), ref[2].view(np.uint32))
            and np.array_equal(got[:, 3].view(np.uint32), ref[3].view(np.uint32)))
    out["records_equal"] = bool(same)
    out["hit_share"] = float((ref[1] >= 0).mean())
    out["rt_trace_rays"] = series(host_call)
    out["device_closest"] = series(lambda: device_call(False))
    out["device_any_hit"] = series(lambda: device_call(True))
    rt.cleanup()
    for k in ("rt_trace_rays", "device_closest", "device_any_hit"):
        r = out[k]
        print("%-16s kernel %.3f ms (runs %s)  %.0f Mray/s  wall %.2f ms per call" % (
            k, r["kernel_ms"], ", ".join("%.3f" % x for x in r["kernel_ms_runs"]), r["mray_s"], r["wall_ms"]))
    print("records equal: %s, hit share %.3f" % (out["records_equal"], out["hit_share"]))
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
    if not same:
        sys.exit("rt_trace_rays and rt_trace_rays_device disagree")


if __name__ == "__main__":
    main()
