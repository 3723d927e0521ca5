"""Geometry motion vectors (rt_set_geometry_motion, k_geom_displacement + k_pt_geom_motion): with the
feature on, the MOTION G-buffer of the first path trace on an LBVH build follows the vertices'
displacement since the previous build, and the temporal filters consume it.

References: the CPU oracle's path trace (whose motion is camera-only; a rigid translation of the
whole mesh by d is the history camera at pos + d), a float64 numpy model of the interpolated
displacement for the non-rigid cases, and one stateful oracle Denoiser fed the GPU's motion buffer.
Unless a test says otherwise: frame_num 2 follows frame 1, 1 spp, the stage calls update ->
build_bvh -> path_trace -> read G-buffers -> denoise_post, and a fixed delta time."""
import os
import socket

import numpy as np
import pytest

from scene_bin import read_bin, terrain_patch, write_bin

pytestmark = pytest.mark.gpu

DT = 16.667
GBUFFERS = (("color", "RENDER_COLOR", 4), ("normal", "NORMAL", 4), ("albedo", "ALBEDO", 4), ("depth", "DEPTH", 1),
            ("motion", "MOTION", 2))
PW, PH = 96, 64  # the patch's frame


# ---------------------------------------------------------------- helpers
def gbuffers(rt, w, h):
    return {k: rt.get_buffer(name, (w * h, c) if c > 1 else (w * h,), np.uint16).copy() for k, name, c in GBUFFERS}


def stage(rt, f, w, h, v=None, builds=1):
    """One staged frame; returns its G-buffers (read between the path trace and the denoise)."""
    if v is not None:
        rt.update_vertices(v)
    for _ in range(builds):
        rt.build_bvh()
    rt.path_trace(f)
    g = gbuffers(rt, w, h)
    rt.denoise_post(f)
    return g


def final(rt, w, h):
    return (rt.download("RGBA8", np.uint8).reshape(-1, 4).copy(),
            rt.get_buffer("RENDER_COLOR", (w * h, 4), np.uint16).copy())


def half_order(bits):
    """Half bit patterns as integers in value order: adjacent halves differ by one."""
    b = bits.astype(np.int32)
    return np.where(b & 0x8000, -(b & 0x7FFF), b & 0x7FFF)


def half_value(bits):
    return np.ascontiguousarray(bits, np.uint16).view(np.float16).astype(np.float64)


def half_ulp(x):
    """One ulp of the half format in the binade of x (subnormals: 2^-24)."""
    e = np.floor(np.log2(np.maximum(np.abs(x), 2.0 ** -14)))
    return 2.0 ** (e - 10)


def default_rt(rtx, tmp_path, w, h, spp=1, name="d.toml", motion=True):
    rt = rtx.RayTracer(w, h, rtx.write_config(str(tmp_path / name), w, h, spp=spp, geometry_motion=motion)).init()
    rt.set_delta_time(DT)
    return rt


def patch_rt(rtx, tmp_path, P, spp=1, name="b.toml", motion=True, tuning=None):
    """A context on the patch; motion True: switched on through the setter, None: never touched."""
    rt = rtx.RayTracer(PW, PH, rtx.write_config(str(tmp_path / name), PW, PH, spp=spp, mesh_file=P["path"],
                                                tuning=tuning)).init()
    rt.set_delta_time(DT)
    rt.camera = P["cam"]
    if motion is not None:
        rt.geometry_motion = motion
        assert rt.geometry_motion is motion
    return rt


def terrain_cameras(rtx, oracle, w, h):
    oc = oracle.default_camera(w, h)
    oc.pos[:] = (8.0, 15.0, -6.0)
    oc.pitch = -0.7
    rc = rtx.Camera()
    rc.pos[:] = (8.0, 15.0, -6.0)
    rc.yaw, rc.pitch, rc.focal, rc.aperture, rc.fovX = 0.0, -0.7, oc.focal, oc.aperture, oc.fovX
    return rc, oc


@pytest.fixture(scope="module")
def sky_tex(oracle):
    return oracle.sky(), oracle.textures()


@pytest.fixture(scope="module")
def patch(rtx, oracle, tmp_path_factory):
    """terrain_patch()[:1012] as a .bin scene (one batch, unshared corners): v the patch, v2 its
    halved heights, v3 only the triangles whose first vertex has x > 5.5 halved; oracle LBVHs."""
    d = tmp_path_factory.mktemp("patch")
    tris = terrain_patch()[:1012]
    tris2 = tris.copy()
    tris2[:, :, 1] *= np.float32(0.5)
    moved = tris[:, 0, 0] > np.float32(5.5)
    tris3 = tris.copy()
    tris3[moved, :, 1] *= np.float32(0.5)
    path = write_bin(str(d / "a.bin"), tris)
    v, i, n = read_bin(path)
    out = dict(path=path, v=v, i=i, n=n, moved=moved)
    for k, t in (("2", tris2), ("3", tris3)):
        out["v" + k] = np.ascontiguousarray(t.reshape(-1, 3))
    for k in ("", "2", "3"):
        vk = out["v" + k]
        out["b" + (k or "1")] = oracle.build_bvh(vk, i, n, oracle.smooth_normals(vk, i))
    cam = rtx.Camera()
    cam.pos[:] = (5.5, 4.0, -3.0)
    cam.yaw, cam.pitch, cam.focal, cam.aperture, cam.fovX = 0.0, -0.55, 5.0, 0.001, np.float32(90.0) * np.float32(0.01745329251)
    oc = oracle.default_camera(PW, PH)
    oc.pos[:] = (5.5, 4.0, -3.0)
    oc.pitch = -0.55
    out.update(cam=cam, oc=oc)
    return out


def motion_model(oracle, b_cur, b_prev, oc, w, h, sample_index):
    """float64 model of the motion buffer: sample 0's hit (oracle.intersect on the new LBVH) moved
    back by the corners' displacement b_cur - b_prev interpolated at (u, v), projected with the
    camera basis of oracle/camera.cpp, less the sample's screen position (blue-noise dimensions 0
    and 1 of sample_index).  Returns (expected [P, 2] with NaN on misses, hit mask, objectIdx)."""
    frame = sample_index // 4
    rays, _ = oracle.primary_rays(w, h, frame, cam=oc)
    oh = oracle.intersect(b_cur, rays)
    assert (oh["droppedPushes"] == 0).all()
    hit = oh["hit"] != 0
    k = oh["objectIdx"][hit]
    cur = b_cur["triangles"][k, :9].astype(np.float64).reshape(-1, 3, 3)
    prev = b_prev["triangles"][k, :9].astype(np.float64).reshape(-1, 3, 3)
    u, v = oh["u"][hit].astype(np.float64), oh["v"][hit].astype(np.float64)
    wts = np.stack([u, v, 1.0 - u - v], 1)[:, :, None]  # of v1, v2, v3
    pos = oh["pos"][hit].astype(np.float64)
    assert np.abs((wts * cur).sum(1) - pos).max() < 1e-4  # (u, v) are the accepted hit's
    pp = pos - (wts * (cur - prev)).sum(1)
    yaw, pitch = float(oc.yaw), float(oc.pitch)
    fwd = np.array([np.sin(yaw) * np.cos(pitch), np.sin(pitch), np.cos(yaw) * np.cos(pitch)])
    left = np.cross([0.0, 1.0, 0.0], fwd)
    left /= np.linalg.norm(left)
    up = np.cross(fwd, left)
    up /= np.linalg.norm(up)
    fov_x = float(oc.fovX)
    tan_x, tan_y = np.tan(fov_x / 2), np.tan(fov_x / w * h / 2)
    dvec = pp - np.array([float(oc.pos[0]), float(oc.pos[1]), float(oc.pos[2])])
    q = np.stack([dvec @ left, dvec @ up, dvec @ fwd], 1)
    last = np.stack([0.5 - (q[:, 0] / q[:, 2]) / tan_x * 0.5, 0.5 - (q[:, 1] / q[:, 2]) / tan_y * 0.5], 1)
    bn = oracle.bluenoise_tables()
    L = oracle.lib()
    px = np.nonzero(hit)[0]
    uv = np.array([[(p % w + L.orc_bluenoise(bn.ctypes.data, int(p % w), int(p // w), sample_index, 0)) / w,
                    (p // w + L.orc_bluenoise(bn.ctypes.data, int(p % w), int(p // w), sample_index, 1)) / h]
                   for p in px])
    want = np.full((w * h, 2), np.nan)
    want[hit] = last - uv + 0.5
    obj = np.full(w * h, -1, np.int64)
    obj[hit] = k
    return want, hit, obj


def assert_meets_model(motion, want, sel, what=""):
    """One ulp of the half at the value's binade, on the pixels sel."""
    got = half_value(motion[sel])
    err = np.abs(got - want[sel]) / half_ulp(want[sel])
    print("%s motion vs float64 model: %d pixels, max %.3f half-ulp" % (what, int(sel.sum()), float(err.max())))
    assert np.isfinite(want[sel]).all()
    assert err.max() <= 1.0, (what, float(err.max()))


def assert_gbuffers(g, o, keys=("color", "normal", "albedo", "depth")):
    for k in keys:
        assert np.array_equal(g[k], o[k].reshape(g[k].shape)), k


# ---------------------------------------------------------------- 1. rigid translation, many batches
def test_rigid_translation_is_a_shifted_history_camera(rtx, oracle, tmp_path, default_scene, sky_tex):
    """Default scene (60 batches), 192x108: the whole mesh moves by d = (0.25, 0.125, -0.5) between
    frames 1 and 2.  Frame 2's colour, normal, albedo and depth are the oracle's on the moved mesh,
    and its motion is the oracle's with the history camera at pos + d: each half component equal or
    the adjacent half (the displacement fl(fl(v + d) - v) is d to within rounding, far below a
    half-ulp of the result).  Without the feature the motion is the camera-only one."""
    s, tex = sky_tex
    w, h = 192, 108
    v, i, n = default_scene["vertices"], default_scene["indices"], default_scene["tri_count"]
    d = np.array([0.25, 0.125, -0.5], np.float32)
    v2 = (v + d).astype(np.float32)
    b2 = oracle.build_bvh(v2, i, n, oracle.smooth_normals(v2, i))
    rc, oc = terrain_cameras(rtx, oracle, w, h)
    shifted = oracle.default_camera(w, h)
    shifted.pos[:] = [float(np.float32(oc.pos[k]) + d[k]) for k in range(3)]
    shifted.pitch = oc.pitch
    same = oracle.pathtrace(b2, w, h, frame_num=2, cam=oc, hist_cam=oc, sky_out=s, tex=tex)
    want = oracle.pathtrace(b2, w, h, frame_num=2, cam=oc, hist_cam=shifted, sky_out=s, tex=tex)
    rays, _ = oracle.primary_rays(w, h, 2, cam=oc)
    hit = oracle.intersect(b2, rays)["hit"] != 0
    assert 0.4 < hit.mean() < 0.7
    assert (want["motion"][hit] != same["motion"][hit]).any(1).all()  # the shift shows at every hit pixel
    rt = default_rt(rtx, tmp_path, w, h)
    assert rt.geometry_motion is True  # [render] geometryMotion
    rt.camera = rc
    stage(rt, 1, w, h)
    g = stage(rt, 2, w, h, v2)
    rt.cleanup()
    assert_gbuffers(g, same)
    diff = np.abs(half_order(g["motion"]) - half_order(want["motion"]))
    print("rigid: %d of %d components one half off" % (int((diff == 1).sum()), diff.size))
    assert diff.max() <= 1
    assert np.array_equal(g["motion"][~hit], same["motion"][~hit])
    assert (g["motion"][hit] != same["motion"][hit]).any(1).mean() > 0.5


# ---------------------------------------------------------------- 2. non-rigid, one batch with padding
def test_non_rigid_motion_meets_the_model(rtx, oracle, tmp_path, patch, sky_tex):
    """The patch's heights halved between frames 1 and 2: every previous vertex is (x, 2y, z) of the
    current one.  Motion within one half-ulp (at the value's binade) of the float64 model at every
    hit pixel, those that reproject off screen included; the other G-buffers are the oracle's."""
    s, tex = sky_tex
    P = patch
    assert np.array_equal(P["b1"]["triangles"][:, 1:9:3], P["b2"]["triangles"][:, 1:9:3] * np.float32(2))
    want, hit, _ = motion_model(oracle, P["b2"], P["b1"], P["oc"], PW, PH, 4 * 2)
    assert 0.3 < hit.mean() < 0.6
    o = oracle.pathtrace(P["b2"], PW, PH, frame_num=2, cam=P["oc"], hist_cam=P["oc"], sky_out=s, tex=tex)
    rt = patch_rt(rtx, tmp_path, P)
    stage(rt, 1, PW, PH)
    g = stage(rt, 2, PW, PH, P["v2"])
    rt.cleanup()
    assert_gbuffers(g, o)
    assert_meets_model(g["motion"], want, hit, "non-rigid")
    assert np.array_equal(g["motion"][~hit], o["motion"][~hit])
    assert (g["motion"][hit] != o["motion"][hit]).any(1).mean() > 0.5


# ---------------------------------------------------------------- 3. zero displacement is exact
def test_unmoved_triangles_keep_the_camera_only_bits(rtx, oracle, tmp_path, patch, sky_tex):
    """Only the triangles whose first vertex has x > 5.5 are halved: a pixel whose sample-0 triangle
    did not move carries the camera-only oracle's motion bit for bit, the others meet the model."""
    s, tex = sky_tex
    P = patch
    want, hit, obj = motion_model(oracle, P["b3"], P["b1"], P["oc"], PW, PH, 4 * 2)
    on_moved = hit & P["moved"][np.maximum(obj, 0)]
    still = hit & ~on_moved
    assert on_moved.sum() > 200 and still.sum() > 200
    o = oracle.pathtrace(P["b3"], PW, PH, frame_num=2, cam=P["oc"], hist_cam=P["oc"], sky_out=s, tex=tex)
    rt = patch_rt(rtx, tmp_path, P)
    stage(rt, 1, PW, PH)
    g = stage(rt, 2, PW, PH, P["v3"])
    rt.cleanup()
    assert_gbuffers(g, o)
    assert np.array_equal(g["motion"][still], o["motion"][still])
    assert np.array_equal(g["motion"][~hit], o["motion"][~hit])
    assert_meets_model(g["motion"], want, on_moved, "partly moved")
    assert (g["motion"][on_moved] != o["motion"][on_moved]).any(1).mean() > 0.5


# ---------------------------------------------------------------- 4. static frames and the switch
def test_static_frames_are_the_frames_without_the_feature(rtx, oracle, tmp_path, patch):
    """No update: frames 1..3 with the feature on are byte-identical to a context that never heard
    of it: all five G-buffers, RGBA8 and RENDER_COLOR."""
    runs = []
    for motion in (None, True):
        rt = patch_rt(rtx, tmp_path, patch, motion=motion, name="s%d.toml" % bool(motion))
        frames = []
        for f in (1, 2, 3):
            g = stage(rt, f, PW, PH)
            frames.append(tuple(g[k] for k, _, _ in GBUFFERS) + final(rt, PW, PH))
        rt.cleanup()
        runs.append(frames)
    for f in range(3):
        for a, b in zip(runs[0][f], runs[1][f]):
            assert np.array_equal(a, b), f + 1


def test_which_builds_and_traces_carry_displacement(rtx, oracle, tmp_path, patch, sky_tex):
    """With the feature on: an update followed by two builds records nothing (the second build is at
    the first one's epoch); of two path traces on one build only the first is displaced; two updates
    before one build are one step from the previous build's positions to the last update's; and a
    context that switches the feature off again traces the camera-only motion."""
    s, tex = sky_tex
    P = patch
    cam_only = oracle.pathtrace(P["b2"], PW, PH, frame_num=2, cam=P["oc"], hist_cam=P["oc"], sky_out=s, tex=tex)["motion"]
    want, hit, _ = motion_model(oracle, P["b2"], P["b1"], P["oc"], PW, PH, 4 * 2)

    rt = patch_rt(rtx, tmp_path, P, name="two_builds.toml")
    stage(rt, 1, PW, PH)
    g = stage(rt, 2, PW, PH, P["v2"], builds=2)
    rt.cleanup()
    assert np.array_equal(g["motion"], cam_only)

    rt = patch_rt(rtx, tmp_path, P, name="two_traces.toml")
    stage(rt, 1, PW, PH)
    rt.update_vertices(P["v2"])
    rt.build_bvh()
    rt.path_trace(2)
    first = rt.get_buffer("MOTION", (PW * PH, 2), np.uint16).copy()
    rt.path_trace(2)
    second = rt.get_buffer("MOTION", (PW * PH, 2), np.uint16).copy()
    rt.cleanup()
    assert_meets_model(first, want, hit, "first trace")
    assert (first[hit] != cam_only[hit]).any(1).mean() > 0.5
    assert np.array_equal(second, cam_only)

    rt = patch_rt(rtx, tmp_path, P, name="two_updates.toml")
    stage(rt, 1, PW, PH)
    rt.update_vertices(P["v3"])
    assert rt.geometry_epoch == 1
    g = stage(rt, 2, PW, PH, P["v2"])
    assert rt.geometry_epoch == 2
    rt.cleanup()
    assert np.array_equal(g["motion"], first)  # the one-update run's bytes: from v, not from v3

    rt = patch_rt(rtx, tmp_path, P, name="off_again.toml")
    stage(rt, 1, PW, PH)
    rt.geometry_motion = False
    g = stage(rt, 2, PW, PH, P["v2"])
    rt.cleanup()
    assert np.array_equal(g["motion"], cam_only)


# ---------------------------------------------------------------- 5. the denoiser consumes it
def test_denoiser_reprojects_through_the_motion_buffer(rtx, oracle, tmp_path, patch, sky_tex):
    """Frames 1, 2, 3 on v, v2, v2: one stateful oracle Denoiser fed the oracle's colour, normal,
    albedo and depth and the GPU's motion buffer of each frame gives the GPU's RGBA8 and
    RENDER_COLOR bit for bit; frame 2 differs from the run without the feature; frame 3's motion
    is camera-only again."""
    s, tex = sky_tex
    P = patch
    got = {}
    for motion in (True, False):
        rt = patch_rt(rtx, tmp_path, P, motion=motion, name="dn%d.toml" % motion)
        frames = []
        for f, v in ((1, None), (2, P["v2"]), (3, None)):
            g = stage(rt, f, PW, PH, v)
            frames.append((g,) + final(rt, PW, PH))
        rt.cleanup()
        got[motion] = frames
    dn = oracle.Denoiser(PW, PH)
    for f, b in ((1, P["b1"]), (2, P["b2"]), (3, P["b2"])):
        o = oracle.pathtrace(b, PW, PH, frame_num=f, cam=P["oc"], hist_cam=P["oc"], sky_out=s, tex=tex)
        g, rgba, color = got[True][f - 1]
        assert_gbuffers(g, o)
        if f != 2:
            assert np.array_equal(g["motion"], o["motion"]), f
        else:
            assert not np.array_equal(g["motion"], o["motion"])
        fed = dict(o, motion=g["motion"])
        out = dn.draw(fed, f, delta_time=DT)
        assert np.array_equal(rgba, out["rgba"]), f
        assert np.array_equal(color, out["color"]), f
    assert np.array_equal(got[True][0][2], got[False][0][2])
    assert not np.array_equal(got[True][1][2], got[False][1][2])
    assert not np.array_equal(got[True][1][1], got[False][1][1])


# ---------------------------------------------------------------- 6. every frame path agrees with the staged one
def staged_frames(rtx, tmp_path, P, spp, name):
    rt = patch_rt(rtx, tmp_path, P, spp=spp, name=name)
    out = []
    for f, v in ((1, None), (2, P["v2"]), (3, None)):
        g = stage(rt, f, PW, PH, v)
        out.append((g["motion"],) + final(rt, PW, PH))
    rt.cleanup()
    return out


@pytest.mark.parametrize("read_each", [False, True], ids=["unread", "read_each"])
@pytest.mark.parametrize("spec", [True, False], ids=["lookahead", "no_lookahead"])
def test_synchronous_draws_match_the_staged_frames(rtx, tmp_path, patch, spec, read_each):
    """draw_device frames 1..3 at 2 spp with the update before frame 2.  Unread: nothing is read
    between the draws, so the LBVH prebuilt and the camera rays and shading traced ahead beside
    frame 1 are pending at the update and are redone, the motion kernel behind the repeated shade
    kernel.  MOTION, RGBA8 and RENDER_COLOR equal the staged frames' byte for byte."""
    import torch

    P = patch
    want = staged_frames(rtx, tmp_path, P, 2, "st.toml")
    rt = patch_rt(rtx, tmp_path, P, spp=2, name="dr.toml", tuning=None if spec else dict(syncSpec=False))
    targets = [torch.zeros((PH, PW, 4), dtype=torch.uint8, device="cuda") for _ in range(3)]
    reads = {}
    for f in (1, 2, 3):
        if f == 2:
            rt.update_vertices(P["v2"])
        rt.draw_device(targets[f - 1].data_ptr())
        if read_each or f == 3:
            reads[f] = (rt.get_buffer("MOTION", (PW * PH, 2), np.uint16).copy(),
                        rt.get_buffer("RENDER_COLOR", (PW * PH, 4), np.uint16).copy())
    rt.cleanup()
    for f in (1, 2, 3):
        assert np.array_equal(targets[f - 1].cpu().numpy().reshape(-1, 4), want[f - 1][1]), f
        if f in reads:
            assert np.array_equal(reads[f][0], want[f - 1][0]), f
            assert np.array_equal(reads[f][1], want[f - 1][2]), f
    assert not np.array_equal(want[1][0], want[2][0])  # frame 2's motion is displaced, frame 3's is not


def test_more_than_one_round_per_sample_wave(rtx, oracle, tmp_path, patch, sky_tex):
    """8 spp: two rounds per sample wave, sample 0's hit record in plane 0 of eight; its frame index
    is 8 (frame_num - 1) + 1."""
    s, tex = sky_tex
    P = patch
    want, hit, _ = motion_model(oracle, P["b2"], P["b1"], P["oc"], PW, PH, 4 * (8 * (2 - 1) + 1))
    o = oracle.pathtrace(P["b2"], PW, PH, frame_num=2, spp=8, cam=P["oc"], hist_cam=P["oc"], sky_out=s, tex=tex)
    rt = patch_rt(rtx, tmp_path, P, spp=8, name="s8.toml")
    stage(rt, 1, PW, PH)
    g = stage(rt, 2, PW, PH, P["v2"])
    rt.cleanup()
    assert_gbuffers(g, o)
    sel = hit & (half_value(o["depth"]) < 60000.0)  # sample 0 hit (the oracle's depth is sample 0's)
    assert sel.sum() > 0.3 * PW * PH
    assert_meets_model(g["motion"], want, sel, "8 spp")
    assert np.array_equal(g["motion"][~hit], o["motion"][~hit])


def _pipeline_run(rtx, tmp_path, seq, w, h, spp, pipelined, events, read_each):
    """FramePipeline frames 1..len(seq) with vertices=seq[f - 1] each, geometry motion on (as
    test_gpu_geometry._pipeline_run); reads MOTION, RGBA8 and RENDER_COLOR."""
    import torch

    from rtx.frames import FramePipeline

    dev = torch.device("cuda", 0)
    base = [torch.from_numpy(a).to(dev) for a in seq]
    torch.cuda.synchronize()
    rt = default_rt(rtx, tmp_path, w, h, spp=spp, name="p%d%d%d.toml" % (pipelined, events, read_each))
    prev = torch.cuda.current_stream(0)
    anim = torch.cuda.Stream(dev) if events else None
    fp = FramePipeline(rt, dev, pipelined=pipelined)
    keep, out = [], []

    def read():
        return (rt.get_buffer("MOTION", (w * h, 2), np.uint16).copy(),) + final(rt, w, h)

    try:
        for f, t in enumerate(base, 1):
            ev = None
            if events:
                with torch.cuda.stream(anim):
                    t = t.clone()
                    ev = torch.cuda.Event()
                    ev.record(anim)
                keep.append(t)
            fp.frame(f, vertices=t, vertices_ready=ev)
            if read_each:
                out.append(read())
        fp.finish()
        if not read_each:
            out.append(read())
    finally:
        rt.cleanup()
        torch.cuda.set_stream(prev)
    return out


def test_pipelined_frames_match_the_serial_run(rtx, oracle, tmp_path, default_scene):
    """FramePipeline on the default scene at 192x108, 4 spp, positions cycling v, v2, v, v2 with an
    update every frame: the pipelined frames, with a ready event per update and without one, equal
    the serial run byte for byte, read frame by frame and with the four frames enqueued unread; the
    serial run's motion is displaced in every frame after the first."""
    v = default_scene["vertices"]
    v2 = v.copy()
    v2[:, 1] += np.float32(0.05) * np.sin(np.float32(3) * v[:, 0] + np.float32(2) * v[:, 2])
    seq = [v, v2, v, v2]
    w, h, spp = 192, 108, 4
    serial = _pipeline_run(rtx, tmp_path, seq, w, h, spp, False, False, True)
    off = rtx.RayTracer(w, h, rtx.write_config(str(tmp_path / "off.toml"), w, h, spp=spp)).init()
    off.build_bvh()
    off.path_trace(1)
    static = off.get_buffer("MOTION", (w * h, 2), np.uint16).copy()  # camera-only, the camera never moves
    off.cleanup()
    assert np.array_equal(serial[0][0], static)
    for f in (1, 2, 3):
        assert (serial[f][0] != static).any(1).mean() > 0.05, f + 1
    for events in (True, False):
        each = _pipeline_run(rtx, tmp_path, seq, w, h, spp, True, events, True)
        for f in range(4):
            for a, b, what in zip(each[f], serial[f], ("MOTION", "RGBA8", "RENDER_COLOR")):
                assert np.array_equal(a, b), (events, f + 1, what)
        last = _pipeline_run(rtx, tmp_path, seq, w, h, spp, True, events, False)
        for a, b, what in zip(last[0], serial[3], ("MOTION", "RGBA8", "RENDER_COLOR")):
            assert np.array_equal(a, b), (events, "unread", what)


RW, RH = 256, 144


def free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def rank_render(rank, world, port, out_dir):
    """Three pipelined frames of the default scene with a whole-mesh update before frame 2, by `world`
    ranks on one GPU over gloo (as test_gpu_multirank.render); every rank updates with the same data."""
    import torch
    import torch.distributed as dist

    import rtx
    from oracle import oracle as O
    from rtx.dist import StripGather, strip_config

    torch.cuda.set_device(0)
    dev = torch.device("cuda", 0)
    if world > 1:
        os.environ["MASTER_ADDR"] = "127.0.0.1"
        os.environ["MASTER_PORT"] = str(port)
        dist.init_process_group("gloo", rank=rank, world_size=world)
    cfg = rtx.write_config(os.path.join(out_dir, "c%d_%d.toml" % (rank, world)), RW, RH, spp=2,
                           extra=strip_config(world, rank), geometry_motion=True)
    rt = rtx.RayTracer(RW, RH, cfg).init()
    rt.set_delta_time(DT)
    rt.set_stream(torch.cuda.current_stream(dev).cuda_stream)
    post = torch.cuda.Stream(dev)
    rt.set_post_stream(post.cuda_stream)
    sg = StripGather(RW, RH, world, rank, dev, rt, sets=rtx.GBUFFER_SETS) if world > 1 else None
    v, _, _ = O.scene(1)
    v2 = (v + np.array([0.25, 0.125, -0.5], np.float32)).astype(np.float32)
    motion = []
    for f in (1, 2, 3):
        if f == 2:
            rt.update_vertices(v2)
        rt.build_bvh()
        rt.path_trace(f)
        if sg is not None:
            rt.sync()
            sg.gather()
        rt.denoise_post(f)
        motion.append(rt.get_buffer("MOTION").copy())
    rgba = rt.download("RGBA8", np.uint8).copy()
    hdr = rt.get_buffer("HISTORY_COLOR").copy()
    rt.cleanup()
    np.savez(os.path.join(out_dir, "m%d_of%d.npz" % (rank, world)), rgba=rgba, hdr=hdr, m1=motion[0], m2=motion[1],
             m3=motion[2])
    if world > 1:
        dist.destroy_process_group()


def test_two_ranks_one_gpu_match_single_rank(tmp_path):
    """Each rank's motion kernel fixes the rows of its own strip before they are exchanged: after the
    gather both ranks hold the single rank's MOTION of every frame, and its final RGBA8 and HDR."""
    import torch.multiprocessing as mp

    mp.start_processes(rank_render, args=(1, 0, str(tmp_path)), nprocs=1, start_method="spawn")
    mp.start_processes(rank_render, args=(2, free_port(), str(tmp_path)), nprocs=2, start_method="spawn")
    ref = np.load(tmp_path / "m0_of1.npz")
    assert not np.array_equal(ref["m2"], ref["m3"])  # frame 2 is displaced
    for r in range(2):
        got = np.load(tmp_path / ("m%d_of2.npz" % r))
        for k in ("rgba", "hdr", "m1", "m2", "m3"):
            assert np.array_equal(got[k], ref[k]), "rank %d %s" % (r, k)
