"""Synchronous draws and the work launched ahead: a state-change matrix over the whole API surface.

A synchronous draw launches the next frame's camera and shade kernels ahead (frame.cpp
launch_spec_camera); the next draw reuses them only if its launch parameters equal theirs
(spec_matches).  No draw's output may depend on that, which holds only if every input those two
kernels read is a field of PathTraceParams, or is changed only through a call that waits for the
streams, drops the launch, or bumps the geometry epoch or the material serial.  The
per-feature tests check their own setters; this module walks every call that changes state between
draws, in one script, against contexts that launch nothing ahead, and reads the launch counters
(RT_ARR_SPEC_STATS) so that "equal with and without" cannot pass because nothing was ever reused.

Each step has a class: DROP (the next draw must not reuse), KEEP (it must: the camera and shade
kernels do not read this input, so the change must not cost a retrace) or FREE (either).  Three draws
follow every step: the one that meets the change and two with nothing changed, so the drop path and
the reuse path alternate all along, and every script runs with 0 and 1 extra leading draws so that
every step meets both parities of the G-buffer set.
"""
import collections
import types

import numpy as np
import pytest

import material_scenes as M
from test_gpu_pathtrace import terrain_camera

pytestmark = pytest.mark.gpu

W, H, SPP = 100, 60, 2  # 6,000 pixels: no multiple of the 64-ray batches
DT = 16.667
SKY_DEPTH = 0x7C00
DROP, KEEP, FREE = "DROP", "KEEP", "FREE"
UNCHANGED = "unchanged"  # the transition between two draws without a step: a reuse, like KEEP
MAPS = ("SOIL_ALBEDO_AO", "SOIL_NORMAL_ROUGHNESS")
END_BUFFERS = ("RENDER_COLOR", "ACCUMULATION", "HISTORY_COLOR", "HISTORY_DEPTH")
GBUFFERS = ("NORMAL", "DEPTH", "ALBEDO", "MOTION", "RENDER_COLOR")

# name, callable(c), class, frames the step draws itself (each follows the draw before it unchanged)
Step = collections.namedtuple("Step", "name fn cls draws")


def step(name, cls, draws=0):
    return lambda fn: Step(name, fn, cls, draws)


# ---------------------------------------------------------------- the steps
SKY_CHANGES = dict(skyScalar=lambda v: v * 2, sunScalar=lambda v: v * 2, sunAngle=lambda v: 2.0,  # from 0.6
                   timeOfDay=lambda v: v + 0.02, sunAxisAngle=lambda v: v + 5, needRegenerate=lambda v: 1)


def sky_step(field, cls=DROP):
    def fn(c):
        p = c.rt.params
        setattr(p.sky, field, SKY_CHANGES[field](getattr(p.sky, field)))
        c.rt.params = p
    return Step("sky." + field, fn, cls, 0)


def camera_step(field, change):
    def fn(c):
        cam = c.rt.camera
        change(cam)
        c.rt.camera = cam
    return Step("camera." + field, fn, DROP, 0)


def params_step(name, change):
    def fn(c):
        p = c.rt.params
        change(p)
        c.rt.params = p
    return Step(name, fn, KEEP, 0)


def pos_x(cam):
    cam.pos[0] += 0.3


def yaw(cam):
    cam.yaw += 0.05


def pitch(cam):
    cam.pitch += 0.03


def focal(cam):
    cam.focal = 6.0


def aperture(cam):
    cam.aperture = 0.004


def fov_x(cam):
    cam.fovX *= 0.9


def sharpening_off(p):
    p.pass_.enableSharpening = 0


def exposure(p):
    p.post.exposure = 2.0  # auto exposure stays on


def sigma(p):
    p.denoise.local_denoise_sigma_depth = 0.2


@step("rt_load_camera", DROP)
def load_camera(c):
    c.rt.load_camera(c.camera_file)


@step("set_frame_index(4)", DROP)
def frame_index(c):
    c.rt.set_frame_index(4)


@step("set_delta_time(25.0)", KEEP)
def delta_time(c):
    c.rt.set_delta_time(25.0)


@step("update_vertices", DROP)
def update_vertices(c):
    c.rt.update_vertices(c.moved[c.sub], first=c.sub.start)


@step("update_vertices_device", DROP)
def update_vertices_device(c):
    c.rt.update_vertices_device(c.d_moved.data_ptr(), len(c.d_moved), first=c.sub.start)


@step("set_mesh(cube)", DROP)
def set_mesh(c):
    c.rt.set_mesh(c.cube_v, c.cube_i)


@step("set_mesh_device(terrain)", DROP)
def set_mesh_device(c):
    c.rt.set_mesh_device(c.d_verts.data_ptr(), len(c.verts), c.d_idx.data_ptr(), len(c.idx))


@step("set_geometry_motion(1)", DROP)
def geometry_motion(c):
    c.rt.geometry_motion = True


@step("set_triangle_materials", DROP)
def triangle_materials(c):
    c.rt.set_triangle_materials(c.ids)


@step("set_triangle_materials_device", DROP)
def triangle_materials_device(c):
    c.rt.set_triangle_materials_device(c.d_ids.data_ptr(), len(c.ids), 0, c.rtx.MAT_CLASS_ALL)


@step("reset_triangle_materials", DROP)
def reset_triangle_materials(c):
    c.rt.reset_triangle_materials()


@step("set_materials(0: emissive)", DROP)
def materials(c):
    m = c.rtx.default_material(0)
    m.emission[:] = (0.5, 1.0, 2.0)
    c.rt.set_materials(0, [m])


@step("reset_materials", DROP)
def reset_materials(c):
    c.rt.reset_materials()


@step("set_emitter_sampling(True, 0.5)", DROP)
def emitters_on(c):
    c.rt.set_emitter_sampling(True, 0.5)


@step("set_emitter_sampling(False)", DROP)
def emitters_off(c):
    c.rt.set_emitter_sampling(False, 0.5)


@step("upload_texture", DROP)
def upload_texture(c):
    c.rt.upload_texture(MAPS[0], c.images[0])


@step("upload_texture_set(1)", DROP)
def upload_texture_set(c):
    c.rt.upload_texture(MAPS[0], c.images[1], set=1)


@step("upload_texture_set_device(1)", DROP)
def upload_texture_set_device(c):
    c.rt.upload_texture_device(MAPS[1], c.d_image, 1, c.rtx.TEX_FORMAT_U16)


@step("set_material_textures(-> 1)", DROP)
def material_textures(c):
    c.rt.set_material_textures(0, [1] * 256)


@step("reset_material_textures", DROP)
def reset_material_textures(c):
    c.rt.reset_material_textures()


@step('get_buffer("DEPTH")', DROP)
def read_depth(c):
    c.rt.get_buffer("DEPTH")


@step("sync", DROP)
def sync(c):
    c.rt.sync()


@step("ray_count", DROP)
def ray_count(c):
    c.extras.append(np.uint64(c.rt.ray_count()))


@step("query.trace(257 rays)", KEEP)
def ray_query(c):
    from rtx import query

    c.hits = query.trace(c.rt, c.d_org, c.d_dir)  # read at the end: the read here would be a host wait


@step("draw(rgba)", DROP, draws=1)
def host_draw(c):
    """One frame into host memory: it follows the draw before it unchanged, and its copy to the host
    waits for the streams, which drops what it launched ahead."""
    rgba = np.zeros((H, W, 4), np.uint8)
    c.rt.draw(rgba)
    c.frames.append(rgba)


# skyScalar and sunScalar first: nothing before them may differ if the tables go stale.  The textures
# are bound to set 1 before the uploads into it, and the emissive table comes while ids of 0 are set,
# so that each of those steps changes what the kernels launched ahead would have read.
STEPS = [
    sky_step("skyScalar"), sky_step("sunScalar"), sky_step("sunAngle"), sky_step("timeOfDay"), sky_step("sunAxisAngle"),
    sky_step("needRegenerate", FREE),  # with nothing else changed
    camera_step("pos", pos_x), camera_step("yaw", yaw), camera_step("pitch", pitch), camera_step("focal", focal),
    camera_step("aperture", aperture), camera_step("fovX", fov_x), load_camera,
    frame_index, delta_time,
    params_step("pass.enableSharpening", sharpening_off), params_step("post.exposure", exposure),
    params_step("denoise.local_denoise_sigma_depth", sigma),
    update_vertices, geometry_motion, update_vertices_device, set_mesh, set_mesh_device,
    triangle_materials, triangle_materials_device, materials, emitters_on, emitters_off, reset_materials,
    reset_triangle_materials,
    upload_texture, material_textures, upload_texture_set, upload_texture_set_device, reset_material_textures,
    read_depth, sync, ray_count, ray_query, host_draw,
]
ORACLE_STEPS = [sky_step("skyScalar"), sky_step("sunScalar"), camera_step("yaw", yaw), sky_step("timeOfDay")]


def script(steps, lead):
    """One entry per draw: the step that runs before it, or None.  Two draws (and `lead` more) before the
    first step, three after every step."""
    entries = [None] * (2 + lead)
    for s in steps:
        entries += [s, None, None]
    return entries


def transitions(entries):
    """(draws, U, K, F): the draws of a script, and its draw-to-draw transitions without a step, behind a
    KEEP step and behind a FREE step."""
    steps = [e for e in entries if e is not None]
    own = sum(s.draws for s in steps)
    u = len(entries) - len(steps) - 1 + own
    return len(entries) + own, u, sum(s.cls == KEEP for s in steps), sum(s.cls == FREE for s in steps)


# ---------------------------------------------------------------- contexts
@pytest.fixture(scope="module")
def images():
    """Three level-0 texture images, never written."""
    out = [np.random.default_rng(seed).integers(0, 65536, size=(1024, 1024, 4), dtype=np.uint16) for seed in (51, 52, 53)]
    for a in out:
        a.setflags(write=False)
    return out


def to_dev(a):
    """A device copy of a numpy array (uint16 / uint32 as int16 / int32 bits), complete on return."""
    import torch

    a = np.array(a, order="C")
    bits = {np.dtype(np.uint16): np.int16, np.dtype(np.uint32): np.int32}.get(a.dtype)
    t = torch.from_numpy(a.view(bits) if bits else a).cuda()
    torch.cuda.synchronize()
    return t


def context(rtx, oracle, tmp_path, name, tuning, images=None):
    """The default scene at the terrain camera, with everything the steps need made before the first
    draw: no step allocates, copies to the device or waits on its own account."""
    cfg = rtx.write_config(str(tmp_path / (name + ".toml")), W, H, spp=SPP, tuning=tuning, texture_sets=2,
                           max_triangles=61440, max_vertices=32768)
    rt = rtx.RayTracer(W, H, cfg).init()
    rt.set_delta_time(DT)
    c = types.SimpleNamespace(rt=rt, rtx=rtx, frames=[], labels=[], classes=[], reused=[], extras=[], hits=None)
    c.ocam, rcam = terrain_camera(rtx, oracle, W, H)
    saved = terrain_camera(rtx, oracle, W, H, pos=(8.5, 15.0, -6.5), yaw=0.1, pitch=-0.65)[1]
    c.camera_file = str(tmp_path / (name + ".cam"))
    rt.camera = saved
    rt.save_camera(c.camera_file)
    rt.camera = rcam
    if images is None:
        return c
    info = rt.info()
    c.verts = rt.download("VERTICES", np.float32).reshape(-1, 3).copy()
    c.idx = rt.download("INDICES", np.uint32).reshape(-1, 3)[:info.triCount].copy()
    assert len(c.verts) == info.vertexCount <= 32768 and len(c.idx) == 60800
    c.sub = slice(len(c.verts) // 4, 3 * len(c.verts) // 4)
    c.moved = c.verts.copy()
    c.moved[:, 1] += np.float32(0.05) * np.sin(np.float32(3) * c.verts[:, 0] + np.float32(2) * c.verts[:, 2])
    again = c.verts.copy()
    again[:, 1] -= np.float32(0.04) * np.cos(np.float32(2) * c.verts[:, 0] - np.float32(3) * c.verts[:, 2])
    c.d_moved = to_dev(again[c.sub])
    c.d_verts, c.d_idx = to_dev(c.verts), to_dev(c.idx)
    cube = M.cube_triangles()
    c.cube_v = np.ascontiguousarray(cube.reshape(-1, 3))
    c.cube_i = np.arange(3 * len(cube), dtype=np.uint32).reshape(-1, 3)
    c.ids = M.hashed_ids(len(c.idx), (3, 3, 3, 5, 4, 1, 0, 7))
    c.d_ids = to_dev(c.ids[::-1])
    c.images = images
    c.d_image = to_dev(images[2])
    rng = np.random.default_rng(7)
    org = np.tile(np.asarray([(8.0, 15.0, -6.0)], np.float32), (257, 1))
    dirs = rng.uniform(-1.0, 1.0, size=(257, 3)).astype(np.float32)
    dirs[:, 1] = -np.abs(dirs[:, 1]) - np.float32(0.2)
    c.d_org, c.d_dir = to_dev(org), to_dev(dirs)
    return c


def note(c, label, cls):
    """A draw is done: its label, the class of the transition into it, and the reuses so far.  SPEC_STATS
    is host state: reading it waits for nothing and leaves what was launched ahead alone."""
    c.labels.append(label)
    c.classes.append(cls)
    c.reused.append(int(c.rt.download("SPEC_STATS", np.uint32)[1]))


def run(c, entries, draw):
    last = None
    for e in entries:
        label = "unchanged since " + last if last else "before any step"
        cls = UNCHANGED if c.labels else None
        if e is not None:
            own = len(c.frames)
            e.fn(c)
            for _ in range(len(c.frames) - own):  # a step that draws: its frame follows the last one unchanged
                note(c, e.name + " itself", UNCHANGED)
            last, label, cls = e.name, "after " + e.name, e.cls
        draw(c)
        note(c, label, cls)


def end_state(c):
    """What the sequence left behind; the context is gone afterwards."""
    rt = c.rt
    out = {k: rt.get_buffer(k).copy() for k in END_BUFFERS}
    out["EXPOSURE"] = rt.download("EXPOSURE").copy()
    out["RGBA8"] = rt.download("RGBA8").copy()
    out["rays"] = np.uint64(rt.ray_count())
    out["extras"] = np.asarray(c.extras, np.uint64)
    if c.hits is not None:
        out["hits"] = c.hits.cpu().numpy().view(np.uint32)
    depth = rt.get_buffer("DEPTH", dtype=np.uint16)
    errors = int(rt.download("PT_QUEUE", np.uint32)[10])
    rt.cleanup()
    assert errors == 0
    # the sky tables reach the image through the camera misses and through the light samples of the hits
    assert 0.2 < float((depth == SKY_DEPTH).mean()) < 0.8
    return out


def assert_same(got, want, what):
    assert len(got.labels) == len(want.labels) == len(got.frames) == len(want.frames)
    for k, (a, b) in enumerate(zip(got.frames, want.frames), start=1):
        assert a.dtype == b.dtype and np.array_equal(a, b), "frame %d (%s): %s" % (k, got.labels[k - 1], what)


def assert_end_states_equal(got, want):
    assert got.keys() == want.keys()
    for k in want:
        assert np.array_equal(got[k], want[k]), k


def draw_hdr(c):
    hdr = np.zeros((H, W, 4), np.float32)
    c.rt.draw(None, hdr)  # keeps what it launched ahead alive: no read of the context follows
    c.frames.append(hdr.view(np.uint32))


# ---------------------------------------------------------------- 2a
@pytest.mark.parametrize("lead", [0, 1])
def test_synchronous_draws_do_not_depend_on_the_launches_ahead(rtx, oracle, tmp_path, images, lead):
    """The whole matrix through rt.draw(None, hdr) with [tuning] syncSpec on and off: every frame's HDR
    bit for bit, and the state left behind.  Then the counters of the context that launches ahead: one
    launch per draw, a reuse at every transition without a step and behind every KEEP step, none behind a
    DROP step.  Without those bounds a renderer that dropped every launch would pass."""
    entries = script(STEPS, lead)
    draws, u, k, f = transitions(entries)
    on = context(rtx, oracle, tmp_path, "on", {"syncSpec": True}, images)
    run(on, entries, draw_hdr)
    stats = on.rt.download("SPEC_STATS", np.uint32).tolist()
    on_end = end_state(on)
    off = context(rtx, oracle, tmp_path, "off", {"syncSpec": False}, images)
    run(off, entries, draw_hdr)
    off_stats = off.rt.download("SPEC_STATS", np.uint32).tolist()
    off_end = end_state(off)
    assert len(on.frames) == draws
    assert_same(on, off, "syncSpec on against off")
    assert_end_states_equal(on_end, off_end)
    launched, reused, dropped, pending = stats
    assert launched == reused + dropped + pending and pending in (0, 1), stats
    assert launched == draws, stats
    so_far, wrong = 0, []
    for n, (cls, total, label) in enumerate(zip(on.classes, on.reused, on.labels), start=1):
        took, so_far = total - so_far, total
        if cls in (UNCHANGED, KEEP) and took != 1:
            wrong.append("frame %d (%s) traced again what was launched ahead" % (n, label))
        elif cls in (DROP, None) and took != 0:  # None: the first draw
            wrong.append("frame %d (%s) reused what was launched ahead" % (n, label))
    assert not wrong, wrong
    assert reused == on.reused[-1] and u + k <= reused <= u + k + f, (stats, u, k, f)
    assert off_stats == [0, 0, 0, 0] and not any(off.reused)


# ---------------------------------------------------------------- 2b
@pytest.mark.parametrize("lead", [0, 1])
def test_pipelined_draws_match_synchronous_ones_through_the_matrix(rtx, oracle, tmp_path, images, lead):
    """The same script (without the draw into host memory, which has no asynchronous form) through
    draw_device(asynchronous=True), each frame into its own slice of one device tensor read once after
    the final sync, against synchronous draw_device calls of a context that launches nothing ahead."""
    import torch

    entries = script([s for s in STEPS if not s.draws], lead)
    ends = []
    runs = []
    for name, asynchronous in (("pipe", True), ("serial", False)):
        c = context(rtx, oracle, tmp_path, name, {"syncSpec": False} if not asynchronous else {}, images)
        target = torch.zeros((len(entries), H, W, 4), dtype=torch.uint8, device="cuda:0")
        torch.cuda.synchronize()
        c.count = 0

        def draw(c):
            c.rt.draw_device(target[c.count].data_ptr(), asynchronous=asynchronous)
            c.count += 1

        run(c, entries, draw)
        c.rt.sync()
        torch.cuda.synchronize()
        c.frames = list(target.cpu().numpy())
        ends.append(end_state(c))
        runs.append(c)
    assert_same(runs[0], runs[1], "pipelined against synchronous")
    assert_end_states_equal(ends[0], ends[1])


# ---------------------------------------------------------------- 2c
def test_the_oracle_follows_sky_and_camera_changes_between_synchronous_draws(rtx, oracle, tmp_path, default_scene):
    """Eight draws that launch ahead, with skyScalar, sunScalar, the camera's yaw and timeOfDay changed in
    between, against the oracle in lockstep: both GPU modes of the matrix test could be wrong alike (tables
    that never regenerate), the oracle cannot."""
    entries = [None, ORACLE_STEPS[0], None, ORACLE_STEPS[1], None, ORACLE_STEPS[2], None, ORACLE_STEPS[3]]
    assert transitions(entries)[:2] == (8, 3)
    c = context(rtx, oracle, tmp_path, "orc", {"syncSpec": True})
    run(c, entries, draw_hdr)
    stats = c.rt.download("SPEC_STATS", np.uint32).tolist()
    c.rt.cleanup()
    sp = dict(oracle.SKY_DEFAULTS)
    tex = oracle.textures()
    dn = oracle.Denoiser(W, H)
    s = oracle.sky(sp)
    cam, prev = c.ocam, c.ocam
    wrong = []
    for f, e in enumerate(entries, start=1):
        if e is not None and e.name.startswith("sky."):  # from the float32 the renderer holds, as the step does
            field = e.name[len("sky."):]
            sp[field] = SKY_CHANGES[field](float(np.float32(sp[field])))
            s = oracle.sky(sp)
        elif e is not None:
            cam = terrain_camera(rtx, oracle, W, H, yaw=0.05)[0]  # the yaw step, from 0
        gb = oracle.pathtrace(default_scene["bvh"], W, H, frame_num=f, spp=SPP, cam=cam, hist_cam=prev, sky_out=s, tex=tex)
        o = dn.draw(gb, f, delta_time=DT)
        ref = o["color"][:, :3].view(np.float16).astype(np.float32).view(np.uint32)
        got = c.frames[f - 1].reshape(-1, 4)[:, :3]
        if not np.array_equal(got, ref):  # the oracle's history stays its own: a wrong frame shows in the later ones too
            wrong.append("frame %d (%s)" % (f, c.labels[f - 1]))
        prev = cam
    assert not wrong, "GPU against the oracle: %s" % wrong
    assert stats[0] == 8 and stats[1] == 3, stats  # the three transitions without a step were reused


# ---------------------------------------------------------------- 3
@pytest.mark.parametrize("names", [GBUFFERS, ("DEPTH",)], ids=["all", "depth"])
@pytest.mark.parametrize("k", [1, 2, 3])
def test_gbuffers_bound_between_synchronous_draws_are_written(rtx, oracle, tmp_path, k, names):
    """k synchronous draws alternate the G-buffer sets; then G-buffers are bound without a set flag (set 0),
    which ends the launches ahead.  Every later frame must land in the caller's memory: after each of four
    more draws the bound NORMAL, DEPTH, ALBEDO and MOTION tensors equal rt.get_buffer of the same name and
    that of a context that never binds, the context is in set 0, and the HDR frames of both are equal
    throughout.

    RENDER_COLOR is bound like the others, but after a whole draw rt.get_buffer("RENDER_COLOR") names the
    denoiser's output (the history buffer with TemporalFilter2 on) while the bound memory is the set's
    colour buffer, which the denoise passes use as scratch: the two differ by design.  Its tensor is
    therefore checked where the same three equalities are defined, after a staged path trace that follows
    the four draws, and after each draw for having been written everywhere (it starts as 0xFF bytes)."""
    import torch

    a = context(rtx, oracle, tmp_path, "bind", {})
    b = context(rtx, oracle, tmp_path, "free", {})
    a.hdr, b.hdr = (np.zeros((H, W, 4), np.float32) for _ in range(2))

    def draw_both(what):
        for c in (a, b):
            c.rt.draw(None, c.hdr)
        assert np.array_equal(a.hdr.view(np.uint32), b.hdr.view(np.uint32)), what

    for n in range(k):
        draw_both("draw %d of %d before the bind" % (n + 1, k))
    bound = {n: torch.full((a.rt.buffer_bytes(n),), 255, dtype=torch.uint8, device="cuda:0") for n in names}
    torch.cuda.synchronize()
    for n, t in bound.items():
        a.rt.bind_buffer(n, t.data_ptr(), t.numel())

    def caller_memory(n):
        torch.cuda.synchronize()
        return bound[n].cpu().numpy()

    for f in range(1, 5):
        what = "draw %d after a bind behind %d draws" % (f, k)
        draw_both(what)
        assert a.rt.info().gbufferSet == 0, what
        for n in names:
            got = caller_memory(n)
            if n == "RENDER_COLOR":
                assert not (got.reshape(-1, 8) == 255).all(axis=1).any(), what
                continue
            assert np.array_equal(got, a.rt.get_buffer(n)), (what, n)
            assert np.array_equal(got, b.rt.get_buffer(n)), (what, n)
    for c in (a, b):  # a staged path trace: RENDER_COLOR is the set's colour buffer until the denoise
        c.rt.build_bvh()
        c.rt.path_trace(k + 5)
        c.rt.sync()
    assert a.rt.info().gbufferSet == 0
    for n in names:
        got = caller_memory(n)
        assert np.array_equal(got, a.rt.get_buffer(n)), n
        assert np.array_equal(got, b.rt.get_buffer(n)), n
    for c in (a, b):
        assert c.rt.download("PT_QUEUE", np.uint32)[10] == 0
        c.rt.cleanup()
    torch.cuda.synchronize()
