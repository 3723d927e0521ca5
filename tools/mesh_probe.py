#!/usr/bin/env python3
"""Cost of a run-time mesh replacement on the GPU: for the default scene and the
config-4 scene, HIP-event medians of

  (a) rt_time_stage(6): a whole-mesh set (rt_set_mesh_device fed the current mesh from a copy), and
      its split into index ingest, adjacency kernels and normals update (rt_time_mesh_set, events
      between the launches),
  (b) rt_time_stage(5): the whole-mesh vertex update on the same mesh, the floor (a) builds on;
      (a) - (b) is the price of a topology change,

one launch per sample in the same process, (a) and (b) interleaved, and

  (c) the wall clock of rt_destroy + rt_create + rt_init for the same mesh in the same process, the
      only way to change topology without rt_set_mesh,
  (h) the host side of rt_init's adjacency for comparison with (a)'s adjacency part: the wall clock
      of rt_mesh_adjacency (rt_init's CSR loop) and of the three host-to-device copies of its result.

Writes profiles/mesh_set.json.

Usage: python tools/mesh_probe.py [--samples 40] [--repeats 5] [--out PATH]"""
import argparse
import json
import os
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "real-time-ray-tracing_amd")]


def scene_times(rtx, torch, chunk, samples, repeats):
    w, h = 256, 144
    cfg = rtx.write_config(os.path.join(tempfile.mkdtemp(), "m.toml"), w, h, chunk_dim=chunk)
    rt = rtx.RayTracer(w, h, cfg).init()
    info = rt.info()
    nv, ntri, NP = int(info.vertexCount), int(info.triCount), int(info.triCountPadded)
    before = {k: rt.download(k).copy() for k in ("INDICES", "NORMALS", "ADJ_OFFSETS", "CORNER_SLOTS")}
    idx = before["INDICES"].view(np.uint32)

    def median(fn):
        return float(np.median([fn() for _ in range(samples + 5)][5:]))

    med_a, med_b, parts = [], [], []
    for _ in range(repeats):  # interleaved, so both see the same clocks
        med_a.append(median(lambda: rt.time_stage(6, 1)))
        med_b.append(median(lambda: rt.time_stage(5, 1)))
        p = np.asarray([rt.time_mesh_set(1) for _ in range(samples + 5)][5:])
        parts.append([float(x) for x in np.median(p, axis=0)])
    same = all(np.array_equal(rt.download(k), before[k]) for k in before)
    b2b_a, b2b_b = rt.time_stage(6, 50) / 50, rt.time_stage(5, 50) / 50
    # (h) rt_init's host loop and its copies
    host, copies = [], []
    dev = torch.device("cuda", 0)
    for _ in range(repeats):
        t0 = time.perf_counter()
        off, corners, slots = rtx.mesh_adjacency(idx, nv)
        t1 = time.perf_counter()
        d = [torch.from_numpy(a.view(np.int32)).to(dev) for a in (off, corners, slots)]
        torch.cuda.synchronize()
        t2 = time.perf_counter()
        del d
        host.append((t1 - t0) * 1e3)
        copies.append((t2 - t1) * 1e3)
    # (c) destroy + create + init
    reinit = []
    for _ in range(repeats):
        t0 = time.perf_counter()
        rt.cleanup()
        rt = rtx.RayTracer(w, h, cfg).init()
        reinit.append((time.perf_counter() - t0) * 1e3)
    rt.cleanup()
    a, b = float(np.median(med_a)), float(np.median(med_b))
    pm = np.median(np.asarray(parts), axis=0)
    hm, cm = float(np.median(host)), float(np.median(copies))
    return dict(chunk_dim=chunk, triangles=ntri, triangles_padded=NP, vertices=nv,
                a_mesh_set_ms=a, a_medians_ms=med_a, a_spread_ms=max(med_a) - min(med_a),
                a_ingest_ms=float(pm[0]), a_adjacency_ms=float(pm[1]), a_normals_ms=float(pm[2]), a_parts_medians_ms=parts,
                b_vertex_update_ms=b, b_medians_ms=med_b, topology_price_ms=a - b, ratio_a_over_b=a / b,
                a_back_to_back_ms=b2b_a, b_back_to_back_ms=b2b_b, arrays_unchanged=bool(same),
                c_destroy_create_init_ms=float(np.median(reinit)), c_series_ms=reinit, ratio_c_over_a=float(np.median(reinit)) / a,
                h_host_adjacency_ms=hm, h_host_copies_ms=cm, h_series_ms=dict(adjacency=host, copies=copies),
                adjacency_device_over_host=float(pm[1]) / (hm + cm), samples_per_median=samples)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--samples", type=int, default=40)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mesh_set.json"))
    a = ap.parse_args()
    if a.samples < 20:
        ap.error("--samples: at least 20 launches per median")
    import torch

    import rtx
    res = dict(device=torch.cuda.get_device_name(0),
               method="HIP events around one launch sequence per sample, median of --samples after 5 warm-up samples, "
                      "repeated --repeats times with (a), (b) and the split interleaved; (c) and (h) are host wall "
                      "clocks (time.perf_counter), medians of --repeats",
               scenes=[scene_times(rtx, torch, c, a.samples, a.repeats) for c in (1, 4)])
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
