#!/usr/bin/env python3
"""Cost of animated geometry on the GPU: for the default scene and the config-4
scene, HIP-event medians of

  (a) k_smooth_normals (rtk_launch_smooth_normals, the init-time kernel, untouched) on that mesh and
  (b) rt_time_stage(5): a whole-mesh vertex update with its normals (csrc/geometry.hip),

one launch per sample in the same process, the compulsory bytes of (b) against the HBM peak, and the
pipelined 1080p 4-spp frame time with a whole-mesh update every frame (with a ready event, without
one) beside the same loop without updates.  Writes profiles/geom_update.json.

Usage: python tools/geom_probe.py [--samples 40] [--repeats 5] [--frames 200] [--out PATH]"""
import argparse
import ctypes as C
import json
import os
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "real-time-ray-tracing_amd")]

HBM_PEAK = 8.0e12  # bytes / s (MI355X, HBM3E)


def csr(indices, nv):
    """Vertex -> corner CSR in triangle order, as rt_init builds it."""
    flat = indices.reshape(-1).astype(np.int64)
    off = np.zeros(nv + 1, np.uint32)
    off[1:] = np.cumsum(np.bincount(flat, minlength=nv))
    corners = np.argsort(flat, kind="stable").astype(np.uint32)
    return off, corners


def stage_times(rtx, torch, chunk, samples, repeats):
    """Medians of (a) and (b) on the scene of [scene] chunkDim `chunk`, `repeats` times each."""
    w, h = 256, 144
    rt = rtx.RayTracer(w, h, rtx.write_config(os.path.join(tempfile.mkdtemp(), "g.toml"), w, h, chunk_dim=chunk)).init()
    info = rt.info()
    nv, NP = int(info.vertexCount), int(info.triCountPadded)
    v = rt.download("VERTICES", np.float32)
    idx = rt.download("INDICES", np.uint32)
    want = rt.download("NORMALS", np.uint32)
    off, corners = csr(idx, nv)
    dev = torch.device("cuda", 0)
    dv, di, doff, dcor = (torch.from_numpy(a).to(dev) for a in (v, idx.view(np.int32), off.view(np.int32), corners.view(np.int32)))
    dn = torch.zeros(nv * 3, dtype=torch.float32, device=dev)
    lib = rt.lib
    launch = lib.rtk_launch_smooth_normals
    launch.restype = C.c_int
    launch.argtypes = [C.c_void_p] * 4 + [C.c_uint32, C.c_void_p, C.c_void_p]
    stream = torch.cuda.Stream(dev)

    def run_a():
        return launch(dv.data_ptr(), doff.data_ptr(), dcor.data_ptr(), di.data_ptr(), nv, dn.data_ptr(), stream.cuda_stream)

    def median_a():
        ms = []
        for k in range(samples + 5):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(stream)
            assert run_a() == 0
            e1.record(stream)
            e1.synchronize()
            if k >= 5:
                ms.append(e0.elapsed_time(e1))
        return float(np.median(ms))

    def median_b():
        ms = [rt.time_stage(5, 1) for _ in range(samples + 5)][5:]
        return float(np.median(ms))

    med_a, med_b = [], []
    for _ in range(repeats):  # interleaved, so both see the same clocks
        med_a.append(median_a())
        med_b.append(median_b())
    stream.synchronize()
    same_a = bool(np.array_equal(dn.cpu().numpy().view(np.uint32), want))
    same_b = bool(np.array_equal(rt.download("NORMALS", np.uint32), want))
    # back to back, 50 launches between two events: what a stream of them costs each
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record(stream)
    for _ in range(50):
        run_a()
    e1.record(stream)
    e1.synchronize()
    b2b_a = e0.elapsed_time(e1) / 50
    b2b_b = rt.time_stage(5, 50) / 50
    rt.cleanup()
    # compulsory traffic of (b): positions in, vertices and normals out, indices, corner slots, CSR
    # offsets, and the contribution array written once and read once (its second read hits the cache)
    parts = dict(positions_in=nv * 12, vertices_out=nv * 12, normals_out=nv * 12, indices=NP * 12, corner_slots=NP * 12,
                 csr_offsets=(nv + 1) * 4, contributions_written=NP * 36, contributions_read=NP * 36)
    total = sum(parts.values())
    a, b = float(np.median(med_a)), float(np.median(med_b))
    return dict(chunk_dim=chunk, triangles=int(info.triCount), triangles_padded=NP, vertices=nv,
                a_smooth_normals_ms=a, a_medians_ms=med_a, a_spread_ms=max(med_a) - min(med_a),
                b_update_ms=b, b_medians_ms=med_b, ratio_b_over_a=b / a, b_not_slower=bool(b <= a + (max(med_a) - min(med_a))),
                a_back_to_back_ms=b2b_a, b_back_to_back_ms=b2b_b, a_bits_equal_init=same_a, b_bits_equal_init=same_b,
                b_bytes=parts, b_bytes_total=total, b_fraction_of_hbm_peak=total / (b * 1e-3) / HBM_PEAK,
                samples_per_median=samples)


def frame_times(rtx, torch, chunk, frames, warmup=30):
    """ms per pipelined 1080p 4-spp frame: no updates / an update per frame with a ready event / without."""
    from rtx.frames import FramePipeline

    w, h = 1920, 1080
    dev = torch.device("cuda", 0)
    out = {}
    for mode in ("none", "ready_event", "null_event"):
        rt = rtx.RayTracer(w, h, rtx.write_config(os.path.join(tempfile.mkdtemp(), "f.toml"), w, h, spp=4, chunk_dim=chunk)).init()
        rt.set_delta_time(16.667)
        v = rt.download("VERTICES", np.float32).reshape(-1, 3)
        v2 = v.copy()
        v2[:, 1] += np.float32(0.05) * np.sin(np.float32(3) * v[:, 0] + np.float32(2) * v[:, 2])
        pos = [torch.from_numpy(a).to(dev) for a in (v, v2)]
        anim = torch.cuda.Stream(dev)
        ev = torch.cuda.Event()
        ev.record(anim)  # the host's animation stream has produced both arrays
        torch.cuda.synchronize()
        prev = torch.cuda.current_stream(0)
        fp = FramePipeline(rt, dev, pipelined=True)
        try:
            t0 = 0.0
            for f in range(1, warmup + frames + 1):
                if f == warmup + 1:
                    fp.finish()
                    t0 = time.perf_counter()
                if mode == "none":
                    fp.frame(f)
                else:
                    fp.frame(f, vertices=pos[f & 1], vertices_ready=ev if mode == "ready_event" else None)
            fp.finish()
            out[mode + "_ms_per_frame"] = (time.perf_counter() - t0) * 1e3 / frames
        finally:
            rt.cleanup()
            torch.cuda.set_stream(prev)
    out["animation_cost_ready_event_ms"] = out["ready_event_ms_per_frame"] - out["none_ms_per_frame"]
    out["animation_cost_null_event_ms"] = out["null_event_ms_per_frame"] - out["none_ms_per_frame"]
    out.update(chunk_dim=chunk, frames=frames, config="1920x1080, 4 spp, pipelined FramePipeline, whole-mesh update per frame")
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--samples", type=int, default=40)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--frames", type=int, default=200)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "geom_update.json"))
    a = ap.parse_args()
    if a.samples < 20:
        ap.error("--samples: at least 20 launches per median")
    import torch

    import rtx
    res = dict(device=torch.cuda.get_device_name(0), hbm_peak_bytes_per_s=HBM_PEAK,
               method="HIP events around one launch per sample, median of --samples after 5 warm-up launches, "
                      "repeated --repeats times with (a) and (b) interleaved; the margin is the spread of (a)'s medians",
               stages=[stage_times(rtx, torch, c, a.samples, a.repeats) for c in (1, 4)],
               frames=[frame_times(rtx, torch, c, a.frames) for c in (1, 4)])
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
