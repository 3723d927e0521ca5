#!/usr/bin/env python3
"""Cost of per-triangle materials on the GPU (rt_set_triangle_materials): pipelined
1080p 4-spp frames on bench.py's terrain camera under six tables,

  none        no table (the null pointer: today's launches)
  all3        an explicit table of 3 everywhere
  lambert     the Lambertian ids 3 / 7 / 8 / 9 scattered over the mesh
  mirror1     1 % of the triangles mirror (id 5), the rest 3
  mirror50    50 % mirror
  mix8        the eight-way mix of the tests: 3 3 3 5 4 1 0 7 by a hash of the triangle index
  none_again  no table again, at the end of each turn: the control, what two series of the same
              launches differ by

in ONE context whose table changes between the timed series (the setter drains the pipeline), the
tables timed in turn --repeats times (--frames frames each, after --warmup frames under the new
table), medians of ms per frame, so that a drift of the box's clocks falls on every table alike.
One context per table, as tools/geom_probe.py times its modes, does not work for seven of them: the
same launches ran 4.32 ms per frame in the context created first and 5.29 in the one created last
(DESIGN.md §4.1.2), a context's place among the process's streams outweighing what is measured.  Whether the first three ran the same kernels is read from the launches, not from
the times: rt_info.lastChain, the length of the queue-3 shading list (kept by the split plan only)
and which kernel slots of marked frames are empty.  The mirror and mix rows carry no threshold: they
are what a whole frame on the glossy plan costs today, the baseline for sorting surface pixels by
material class.

Writes profiles/materials.json.

With --device-sets: the table re-set ahead of every frame through rt_set_triangle_materials_device,
through the host setter, and not at all (device_sets below); writes profiles/materials_device.json.

With --material-table: the cost of the table-reading kernel variant of rt_set_materials
(material_table below); writes profiles/material_table.json.

With --texture-sets: the cost of per-material texture sets (texture_sets below); writes
profiles/texture_sets.json.

Usage: python tools/material_probe.py [--device-sets | --material-table | --texture-sets] [--frames 100] [--repeats 5] [--out PATH]"""
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
MIX8 = (3, 3, 3, 5, 4, 1, 0, 7)
EMPTY_SLOT_MS = 0.002  # two events with nothing between them


def hashed(n, palette):
    k = (np.arange(n, dtype=np.uint64) * np.uint64(2654435761)) >> np.uint64(7)
    return np.asarray(palette, np.uint8)[(k % np.uint64(len(palette))).astype(np.int64)]


def tables(n):
    """name -> uint8[n] (None: no table)."""
    h = (np.arange(n, dtype=np.uint64) * np.uint64(2654435761) >> np.uint64(7)) % np.uint64(100)
    return dict(none=None, none_again=None, all3=np.full(n, 3, np.uint8), lambert=hashed(n, (3, 7, 8, 9)),
                mirror1=np.where(h < 1, 5, 3).astype(np.uint8), mirror50=np.where(h < 50, 5, 3).astype(np.uint8),
                mix8=hashed(n, MIX8))


def device_sets(a):
    """--device-sets: what re-setting the whole table every frame costs a pipelined 1080p frame, four
    ways in ONE context, timed in turn --repeats times (medians of ms per frame):

      device   rt_set_triangle_materials_device ahead of every frame, two tables of the same classes
               (mix8 and its reverse) alternating, the ids resident on the device, with the ready
               event of their upload (the set runs beside the previous frame's trace chain)
      device_no_event  the same with ready_event NULL: the read follows the context stream's work,
               the previous frame's trace chain included
      host     the same through rt_set_triangle_materials, which drains the pipeline every frame
      none     no set at all: the frames under the table the last series left

    Writes profiles/materials_device.json."""
    import torch

    import rtx
    from rtx.frames import FramePipeline

    w, h, spp = 1920, 1080, 4
    dev = torch.device("cuda", 0)
    prev = torch.cuda.current_stream(0)
    rt = rtx.RayTracer(w, h, rtx.write_config(os.path.join(tempfile.mkdtemp(), "m.toml"), w, h, spp=spp)).init()
    try:
        rt.set_delta_time(16.667)
        cam = rt.camera
        cam.pos[:] = TERRAIN_CAM["pos"]
        cam.yaw, cam.pitch = TERRAIN_CAM["yaw"], TERRAIN_CAM["pitch"]
        rt.camera = cam
        n = int(rt.info().triCount)
        host = [hashed(n, MIX8), hashed(n, MIX8)[::-1].copy()]
        classes = rtx.material_classes(host[0])
        assert classes == rtx.material_classes(host[1])
        resident = [torch.from_numpy(t).to(dev) for t in host]
        ready = torch.cuda.Event()
        ready.record(prev)
        torch.cuda.synchronize()
        fp = FramePipeline(rt, dev, pipelined=True)
        state = dict(f=0)

        def run(mode, frames):
            for _ in range(frames):
                state["f"] += 1
                k = state["f"] & 1
                if mode == "device":
                    rt.set_triangle_materials_device(resident[k].data_ptr(), n, 0, classes, ready.cuda_event)
                elif mode == "device_no_event":
                    rt.set_triangle_materials_device(resident[k].data_ptr(), n, 0, classes)
                elif mode == "host":
                    rt.set_triangle_materials(host[k])
                fp.frame(state["f"])
            fp.finish()

        modes = ("device", "device_no_event", "host", "none")
        series = {m: [] for m in modes}
        for _ in range(a.repeats):
            for m in modes:
                run(m, a.warmup)
                t0 = time.perf_counter()
                run(m, a.frames)
                series[m].append((time.perf_counter() - t0) * 1e3 / a.frames)
        run("device", 3)
        assert np.array_equal(rt.download("TRI_MATERIALS"), host[state["f"] & 1])
        assert np.array_equal(rt.download("TRI_MATERIAL_CENSUS", np.uint32), np.bincount(host[0], minlength=256))
        errors = int(rt.download("PT_QUEUE", np.uint32)[10])
    finally:
        rt.cleanup()
        torch.cuda.set_stream(prev)
    rows = {m: dict(ms_per_frame=float(np.median(series[m])), series_ms=series[m]) for m in modes}
    for m in modes:
        rows[m]["over_none_ms"] = rows[m]["ms_per_frame"] - rows["none"]["ms_per_frame"]
    res = dict(device=torch.cuda.get_device_name(0),
               config="%dx%d, %d spp, terrain camera %r, pipelined FramePipeline, LBVH rebuild every frame, %d triangles, "
                      "the whole table (mix8 / its reverse, classes %d) set ahead of every frame" % (w, h, spp, TERRAIN_CAM, n, classes),
               method="one context; the four modes timed in turn %d times, %d frames each after %d warm-up frames; "
                      "ms_per_frame is the median of the series, host time per frame with one wait at the end of a series"
                      % (a.repeats, a.frames, a.warmup),
               internal_errors=errors, modes=rows,
               host_minus_device_ms=rows["host"]["ms_per_frame"] - rows["device"]["ms_per_frame"])
    out = a.out if a.out != DEFAULT_OUT else os.path.join(ROOT, "profiles", "materials_device.json")
    os.makedirs(os.path.dirname(out), exist_ok=True)
    with open(out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res))


def material_table(a):
    """--material-table: what the table-reading kernel variant costs (rt_set_materials, DESIGN.md
    §4.1.4): pipelined 1080p 4-spp frames of the terrain under hashed(MIX8), in ONE context, timed in
    turn --repeats times (medians of ms per frame):

      mix8        no custom table: the all-classes kernels on the reference's constants
      mix8_table  the same ids with the defaults passed through rt_set_materials: the same pixels from
                  the table-reading variant
      mix8_again  no custom table again: the control

    and per-kernel times of marked frames of the first two.  Writes profiles/material_table.json."""
    import torch

    import rtx
    from rtx.frames import FramePipeline

    w, h, spp = 1920, 1080, 4
    dev = torch.device("cuda", 0)
    prev = torch.cuda.current_stream(0)
    names = ("mix8", "mix8_table", "mix8_again")
    rt = rtx.RayTracer(w, h, rtx.write_config(os.path.join(tempfile.mkdtemp(), "m.toml"), w, h, spp=spp)).init()
    try:
        rt.set_delta_time(16.667)
        cam = rt.camera
        cam.pos[:] = TERRAIN_CAM["pos"]
        cam.yaw, cam.pitch = TERRAIN_CAM["yaw"], TERRAIN_CAM["pitch"]
        rt.camera = cam
        rt.set_triangle_materials(hashed(int(rt.info().triCount), MIX8))
        defaults = [rtx.default_material(i) for i in range(256)]
        fp = FramePipeline(rt, dev, pipelined=True)
        state = dict(f=0)

        def use(name):  # both calls are setters: they drain the pipeline first
            if name == "mix8_table":
                rt.set_materials(0, defaults)
            else:
                rt.reset_materials()

        def run(n):
            for _ in range(n):
                state["f"] += 1
                fp.frame(state["f"])
            fp.finish()

        series = {name: [] for name in names}
        for _ in range(a.repeats):
            for name in names:
                use(name)
                run(a.warmup)
                t0 = time.perf_counter()
                run(a.frames)
                series[name].append((time.perf_counter() - t0) * 1e3 / a.frames)
        rows = {}
        for name in names:
            use(name)
            # the blue-noise sequence repeats with the frame index: every marked series starts at the same
            # phase of it, so that the queue lengths of the last frame compare (equal: the same paths)
            run((-state["f"]) % 256)
            run(a.warmup)
            rt.frame_marks_begin(a.marked)
            run(a.marked)
            ms, n = rt.frame_marks_read()
            q = rt.download("PT_QUEUE", np.uint32)
            rows[name] = dict(ms_per_frame=float(np.median(series[name])), series_ms=series[name],
                              last_chain=int(rt.info().lastChain), queue3_entries=int(q[0]), queue4_entries=int(q[1]),
                              internal_errors=int(q[10]), marked_frames=n,
                              kernel_ms={k: round(v, 4) for k, v in ms.items()})
    finally:
        rt.cleanup()
        torch.cuda.set_stream(prev)
    res = dict(device=torch.cuda.get_device_name(0),
               config="%dx%d, %d spp, terrain camera %r, pipelined FramePipeline, LBVH rebuild every frame, ids hashed(MIX8)"
                      % (w, h, spp, TERRAIN_CAM),
               method="one context, the material table set / reset between series; the three timed in turn %d times, %d "
                      "frames each after %d warm-up frames; ms_per_frame is the median of the series; kernel_ms from %d "
                      "frames bracketed by events" % (a.repeats, a.frames, a.warmup, a.marked),
               tables=rows,
               same_queue_lengths=len({(r["queue3_entries"], r["queue4_entries"]) for r in rows.values()}) == 1,
               table_cost_ms=rows["mix8_table"]["ms_per_frame"] - rows["mix8"]["ms_per_frame"],
               control_ms=rows["mix8_again"]["ms_per_frame"] - rows["mix8"]["ms_per_frame"])
    out = a.out if a.out != DEFAULT_OUT else os.path.join(ROOT, "profiles", "material_table.json")
    os.makedirs(os.path.dirname(out), exist_ok=True)
    with open(out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res))


def texture_sets(a):
    """--texture-sets: what sampling per-material texture sets costs (rt_set_material_textures, DESIGN.md
    §4.1.5): pipelined 1080p 4-spp frames of the terrain under hashed(MIX8), in ONE context with four
    texture sets, timed in turn --repeats times (medians of ms per frame).  Sets 1..3 are what rt_init
    made them, device copies of the soil atlas in memory of their own: every series renders the same
    pixels along the same paths (the queue lengths are compared), so the series differ by the addressing
    and by the texture footprint alone.  (Other images change the shading normals and with them the
    paths: a first version with random images traced 22 % fewer bounce rays and measured that instead.)

      table         the defaults through rt_set_materials, no binding: the table-reading kernels at set 0
      table_set1    the same with every id bound to set 1: one other atlas
      table_4sets   id k bound to set k % 4: neighbouring hits sample different atlases
      table_again   the first series again: the control

    Writes profiles/texture_sets.json."""
    import torch

    import rtx
    from rtx.frames import FramePipeline

    w, h, spp, sets = 1920, 1080, 4, 4
    dev = torch.device("cuda", 0)
    prev = torch.cuda.current_stream(0)
    names = ("table", "table_set1", "table_4sets", "table_again")
    bind = dict(table=[0] * 256, table_set1=[1] * 256, table_4sets=[k % sets for k in range(256)], table_again=[0] * 256)
    cfg = rtx.write_config(os.path.join(tempfile.mkdtemp(), "m.toml"), w, h, spp=spp, texture_sets=sets)
    rt = rtx.RayTracer(w, h, cfg).init()
    try:
        rt.set_delta_time(16.667)
        cam = rt.camera
        cam.pos[:] = TERRAIN_CAM["pos"]
        cam.yaw, cam.pitch = TERRAIN_CAM["yaw"], TERRAIN_CAM["pitch"]
        rt.camera = cam
        rt.set_triangle_materials(hashed(int(rt.info().triCount), MIX8))
        rt.set_materials(0, [rtx.default_material(i) for i in range(256)])
        fp = FramePipeline(rt, dev, pipelined=True)
        state = dict(f=0)

        def run(n):
            for _ in range(n):
                state["f"] += 1
                fp.frame(state["f"])
            fp.finish()

        series = {name: [] for name in names}
        for _ in range(a.repeats):
            for name in names:
                rt.set_material_textures(0, bind[name])  # a setter: it drains the pipeline first
                run(a.warmup)
                t0 = time.perf_counter()
                run(a.frames)
                series[name].append((time.perf_counter() - t0) * 1e3 / a.frames)
        rows = {}
        for name in names:
            rt.set_material_textures(0, bind[name])
            run((-state["f"]) % 256)  # every marked series at the same phase of the blue-noise sequence
            run(a.warmup)
            rt.frame_marks_begin(a.marked)
            run(a.marked)
            ms, n = rt.frame_marks_read()
            q = rt.download("PT_QUEUE", np.uint32)
            rows[name] = dict(ms_per_frame=float(np.median(series[name])), series_ms=series[name],
                              sets_bound=sorted(set(bind[name])), last_chain=int(rt.info().lastChain),
                              queue3_entries=int(q[0]), queue4_entries=int(q[1]), internal_errors=int(q[10]),
                              marked_frames=n, kernel_ms={k: round(v, 4) for k, v in ms.items()})
    finally:
        rt.cleanup()
        torch.cuda.set_stream(prev)
    base = rows["table"]["ms_per_frame"]
    res = dict(device=torch.cuda.get_device_name(0),
               config="%dx%d, %d spp, terrain camera %r, pipelined FramePipeline, LBVH rebuild every frame, ids hashed(MIX8), "
                      "%d texture sets, the material table the defaults" % (w, h, spp, TERRAIN_CAM, sets),
               method="one context, the binding set between series; the four timed in turn %d times, %d frames each after "
                      "%d warm-up frames; ms_per_frame is the median of the series; kernel_ms from %d frames bracketed by "
                      "events" % (a.repeats, a.frames, a.warmup, a.marked),
               series=rows,
               same_queue_lengths=len({(r["queue3_entries"], r["queue4_entries"]) for r in rows.values()}) == 1,
               set1_cost_ms=rows["table_set1"]["ms_per_frame"] - base,
               four_sets_cost_ms=rows["table_4sets"]["ms_per_frame"] - base,
               control_ms=rows["table_again"]["ms_per_frame"] - base)
    out = a.out if a.out != DEFAULT_OUT else os.path.join(ROOT, "profiles", "texture_sets.json")
    os.makedirs(os.path.dirname(out), exist_ok=True)
    with open(out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res))


DEFAULT_OUT = os.path.join(ROOT, "profiles", "materials.json")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=100)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--marked", type=int, default=20, help="frames whose kernels are bracketed by events")
    ap.add_argument("--device-sets", action="store_true",
                    help="time the table re-set every frame: device call, host setter, no set (profiles/materials_device.json)")
    ap.add_argument("--material-table", action="store_true",
                    help="time the table-reading kernel variant against the same ids without a custom table "
                         "(profiles/material_table.json)")
    ap.add_argument("--texture-sets", action="store_true",
                    help="time the table-reading kernels under texture-set bindings (profiles/texture_sets.json)")
    ap.add_argument("--out", default=DEFAULT_OUT)
    a = ap.parse_args()
    if a.texture_sets:
        return texture_sets(a)
    if a.device_sets:
        return device_sets(a)
    if a.material_table:
        return material_table(a)
    import torch

    import rtx
    from rtx.frames import FramePipeline

    w, h, spp = 1920, 1080, 4
    dev = torch.device("cuda", 0)
    prev = torch.cuda.current_stream(0)
    names = ("none", "all3", "lambert", "mirror1", "mirror50", "mix8", "none_again")
    rt = rtx.RayTracer(w, h, rtx.write_config(os.path.join(tempfile.mkdtemp(), "m.toml"), w, h, spp=spp)).init()
    try:
        rt.set_delta_time(16.667)
        cam = rt.camera
        cam.pos[:] = TERRAIN_CAM["pos"]
        cam.yaw, cam.pitch = TERRAIN_CAM["yaw"], TERRAIN_CAM["pitch"]
        rt.camera = cam
        tabs = tables(int(rt.info().triCount))
        fp = FramePipeline(rt, dev, pipelined=True)
        state = dict(f=0)

        def use(name):  # both calls are setters: they drain the pipeline first
            if tabs[name] is None:
                rt.reset_triangle_materials()
            else:
                rt.set_triangle_materials(tabs[name])
                assert np.array_equal(rt.download("TRI_MATERIALS"), tabs[name])

        def run(n):
            for _ in range(n):
                state["f"] += 1
                fp.frame(state["f"])
            fp.finish()

        series = {name: [] for name in names}
        for _ in range(a.repeats):
            for name in names:
                use(name)
                run(a.warmup)
                t0 = time.perf_counter()
                run(a.frames)
                series[name].append((time.perf_counter() - t0) * 1e3 / a.frames)
        rows = {}
        for name in names:  # what was launched: marked frames, the plan, the shading list
            use(name)
            run(a.warmup)
            rt.frame_marks_begin(a.marked)  # all 15: the path trace and the denoise / post kernels
            run(a.marked)
            ms, n = rt.frame_marks_read()
            q = rt.download("PT_QUEUE", np.uint32)
            ids = tabs[name]
            census = {} if ids is None else {int(k): int(v) for k, v in zip(*np.unique(ids, return_counts=True))}
            rows[name] = dict(
                ms_per_frame=float(np.median(series[name])), series_ms=series[name],
                classes=0 if ids is None else rtx.material_classes(ids), census=census,
                last_chain=int(rt.info().lastChain), shading_list_entries=int(q[23]), queue3_entries=int(q[0]),
                queue4_entries=int(q[1]), internal_errors=int(q[10]), marked_frames=n,
                kernel_ms={k: round(v, 4) for k, v in ms.items()},
                empty_slots=sorted(k for k, v in ms.items() if k in rt.PT_KERNELS and v < EMPTY_SLOT_MS))
    finally:
        rt.cleanup()
        torch.cuda.set_stream(prev)

    def plan(r):  # what tells the plans apart: the chain, a kept shading list, the slots that ran
        return (r["last_chain"], r["shading_list_entries"] > 0, tuple(r["empty_slots"]))

    for name in names:
        rows[name]["same_kernels_as_none"] = plan(rows[name]) == plan(rows["none"])
        rows[name]["cost_over_none_ms"] = rows[name]["ms_per_frame"] - rows["none"]["ms_per_frame"]
    res = dict(device=torch.cuda.get_device_name(0),
               config="%dx%d, %d spp, terrain camera %r, pipelined FramePipeline, LBVH rebuild every frame" % (w, h, spp, TERRAIN_CAM),
               method="one context, the table changed between series; the tables timed in turn %d times, %d frames each "
                      "after %d warm-up frames; ms_per_frame is the median of the series; kernel_ms from %d frames bracketed by events"
                      % (a.repeats, a.frames, a.warmup, a.marked),
               tables=rows)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
