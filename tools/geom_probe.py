#!/usr/bin/env python3
"""Cost of animated geometry on the GPU: for the default scene and the config-4
scene, HIP-event medians of

  (a) k_smooth_normals (rtk_launch_smooth_normals, the init-time kernel, untouched) on that mesh and
  (b) rt_time_stage(5): a whole-mesh vertex update with its normals (csrc/geometry.hip),

one launch per sample in the same process, the compulsory bytes of (b) against the HBM peak, and the
pipelined 1080p 4-spp frame time with a whole-mesh update every frame (with a ready event, without
one) beside the same loop without updates.  Geometry motion vectors (rt_set_geometry_motion) add

  (c) k_geom_displacement alone (rtk_launch_geometry_displacement on the context's own arrays),
  (d) the shade kernel's mark slot of a serial 1080p frame on moved geometry with the feature on and
      off, same process, frame by frame in turn: k_pt_geom_motion has no slot of its own, it is the
      difference, and
  (e) the pipelined loop with a ready event again with the feature on, beside the run with it off.

Writes profiles/geom_update.json.

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


class GeomDispParams(C.Structure):  # csrc/bvh_kernels.h
    _fields_ = [("vertices", C.c_void_p), ("prevVerts", C.c_void_p), ("indices", C.c_void_p), ("triDisp", C.c_void_p),
                ("triCountPadded", C.c_uint32)]


def motion_times(rtx, torch, chunk, samples, repeats):
    """(c) and (d) on the scene of [scene] chunkDim `chunk`."""
    dev = torch.device("cuda", 0)
    w, h = 1920, 1080
    cfg = lambda name, on: rtx.write_config(os.path.join(tempfile.mkdtemp(), name), w, h, spp=4, chunk_dim=chunk,
                                            geometry_motion=on)
    rts = {on: rtx.RayTracer(w, h, cfg("m%d.toml" % on, on)).init() for on in (True, False)}
    rt = rts[True]
    info = rt.info()
    nv, NP = int(info.vertexCount), int(info.triCountPadded)
    v = rt.download("VERTICES", np.float32).reshape(-1, 3)
    v2 = v.copy()
    v2[:, 1] += np.float32(0.05) * np.sin(np.float32(3) * v[:, 0] + np.float32(2) * v[:, 2])
    idx = rt.download("INDICES", np.uint32)
    dcur, dprev, di = (torch.from_numpy(a).to(dev) for a in (v2, v, idx.view(np.int32)))
    ddisp = torch.zeros(NP * 12, dtype=torch.float32, device=dev)
    launch = rt.lib.rtk_launch_geometry_displacement
    launch.restype = C.c_int
    launch.argtypes = [C.POINTER(GeomDispParams), C.c_void_p]
    prm = GeomDispParams(dcur.data_ptr(), dprev.data_ptr(), di.data_ptr(), ddisp.data_ptr(), NP)
    stream = torch.cuda.Stream(dev)
    med_c = []
    for _ in range(repeats):
        ms = []
        for k in range(samples + 5):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(stream)
            assert launch(C.byref(prm), stream.cuda_stream) == 0
            e1.record(stream)
            e1.synchronize()
            if k >= 5:
                ms.append(e0.elapsed_time(e1))
        med_c.append(float(np.median(ms)))
    d = ddisp.cpu().numpy().reshape(NP, 3, 4)
    want = (v2[idx.reshape(-1, 3)] - v[idx.reshape(-1, 3)])
    disp_ok = bool(np.array_equal(d[:, :, :3], want) and not d[:, :, 3].any())
    # (d): serial frames, the geometry alternating between v and v2, the shade slot marked
    pos = [torch.from_numpy(a).to(dev) for a in (v, v2)]
    torch.cuda.synchronize()
    slot = {True: [], False: []}
    for f in range(1, samples + 6):
        for on in (True, False):
            r = rts[on]
            r.set_delta_time(16.667)
            r.update_vertices_device(pos[f & 1].data_ptr(), nv, 0, None)
            r.build_bvh()
            r.frame_marks_begin(1, ["k_pt_shade0"])
            r.path_trace(f)
            r.denoise_post(f)
            ms, n = r.frame_marks_read()
            assert n == 1
            if f > 5:
                slot[on].append(ms["k_pt_shade0"])
    same = bool(np.array_equal(rts[True].get_buffer("RENDER_COLOR"), rts[False].get_buffer("RENDER_COLOR")))
    for r in rts.values():
        r.cleanup()
    on_ms, off_ms = float(np.median(slot[True])), float(np.median(slot[False]))
    c = float(np.median(med_c))
    nbytes = NP * 12 + 2 * 3 * NP * 12 + NP * 48  # indices, two gathered positions per corner, the records
    return dict(chunk_dim=chunk, triangles_padded=NP, vertices=nv, c_displacement_ms=c, c_medians_ms=med_c,
                c_bytes=nbytes, c_fraction_of_hbm_peak=nbytes / (c * 1e-3) / HBM_PEAK, c_bits_equal_numpy=disp_ok,
                d_shade_slot_motion_on_ms=on_ms, d_shade_slot_motion_off_ms=off_ms, d_motion_kernel_ms=on_ms - off_ms,
                d_config="1920x1080, 4 spp, serial staged frames, whole-mesh update per frame, median of %d frames" % samples,
                d_denoised_frames_differ=not same, samples_per_median=samples)


def frame_times(rtx, torch, chunk, frames, warmup=30, repeats=5):
    """ms per pipelined 1080p 4-spp frame: no updates / an update per frame with a ready event / without /
    with a ready event and geometry motion vectors on.  One context per mode in the same process, the
    modes timed in turn `repeats` times (`frames` frames each, after `warmup` frames once): medians, so
    that a drift of the box's clocks falls on every mode alike."""
    from rtx.frames import FramePipeline

    w, h = 1920, 1080
    dev = torch.device("cuda", 0)
    modes = ("none", "ready_event", "null_event", "ready_event_motion")
    prev = torch.cuda.current_stream(0)
    ctx, series = {}, {m: [] for m in modes}
    try:
        for mode in modes:
            rt = rtx.RayTracer(w, h, rtx.write_config(os.path.join(tempfile.mkdtemp(), "f.toml"), w, h, spp=4, chunk_dim=chunk,
                                                      geometry_motion=mode == "ready_event_motion")).init()
            rt.set_delta_time(16.667)
            v = rt.download("VERTICES", np.float32).reshape(-1, 3)
            v2 = v.copy()
            v2[:, 1] += np.float32(0.05) * np.sin(np.float32(3) * v[:, 0] + np.float32(2) * v[:, 2])
            pos = [torch.from_numpy(a).to(dev) for a in (v, v2)]
            anim = torch.cuda.Stream(dev)
            ev = torch.cuda.Event()
            ev.record(anim)  # the host's animation stream has produced both arrays
            torch.cuda.synchronize()
            ctx[mode] = dict(rt=rt, pos=pos, ev=ev, fp=FramePipeline(rt, dev, pipelined=True), f=0)

        def run(mode, n):
            c = ctx[mode]
            for _ in range(n):
                c["f"] += 1
                if mode == "none":
                    c["fp"].frame(c["f"])
                else:
                    c["fp"].frame(c["f"], vertices=c["pos"][c["f"] & 1], vertices_ready=None if mode == "null_event" else c["ev"])
            c["fp"].finish()

        for mode in modes:
            run(mode, warmup)
        for _ in range(repeats):
            for mode in modes:
                t0 = time.perf_counter()
                run(mode, frames)
                series[mode].append((time.perf_counter() - t0) * 1e3 / frames)
    finally:
        for c in ctx.values():
            c["rt"].cleanup()
        torch.cuda.set_stream(prev)
    out = {m + "_ms_per_frame": float(np.median(series[m])) for m in modes}
    out.update({m + "_series_ms": series[m] for m in modes})
    out["animation_cost_ready_event_ms"] = out["ready_event_ms_per_frame"] - out["none_ms_per_frame"]
    out["animation_cost_null_event_ms"] = out["null_event_ms_per_frame"] - out["none_ms_per_frame"]
    out["motion_cost_ready_event_ms"] = out["ready_event_motion_ms_per_frame"] - out["ready_event_ms_per_frame"]
    out.update(chunk_dim=chunk, frames=frames, repeats=repeats,
               config="1920x1080, 4 spp, pipelined FramePipeline, whole-mesh update per frame")
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
               motion=[motion_times(rtx, torch, c, a.samples, a.repeats) for c in (1, 4)],
               frames=[frame_times(rtx, torch, c, a.frames) for c in (1, 4)])
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
