"""Animated geometry (rt_update_vertices / rt_update_vertices_device, csrc/geometry.hip) vs the CPU
oracle, bit for bit: a context whose vertices were updated holds the vertices, the smooth normals
and, after the next build, the LBVH of a context that rt_init had given the new positions, and
every frame drawn after the update shows the new geometry — synchronous draws, whose next LBVH,
camera rays and shading are prepared ahead of the update, and pipelined frames with an update in
flight every frame alike.

The displaced default scene moves 99.6 % of the normals and 74 % of the reorder array (checked on
the oracle below), so no stale array passes."""
import numpy as np
import pytest

from scene_bin import read_bin, terrain_patch, write_bin

pytestmark = pytest.mark.gpu

DT = 16.667
RT_ERR_ARG = -1


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def displaced(v):
    v2 = v.copy()
    v2[:, 1] += np.float32(0.05) * np.sin(np.float32(3) * v[:, 0] + np.float32(2) * v[:, 2])
    assert v2.dtype == np.float32
    return v2


@pytest.fixture(scope="module")
def moved_scene(oracle, default_scene):
    """The default scene with displaced heights: positions, oracle normals and oracle LBVH."""
    v, i, n = default_scene["vertices"], default_scene["indices"], default_scene["tri_count"]
    v2 = displaced(v)
    nrm2 = oracle.smooth_normals(v2, i)
    bvh2 = oracle.build_bvh(v2, i, n, nrm2)
    # what the issue checked on the oracle: the update is visible in every array compared below
    assert np.isfinite(nrm2).all()
    assert (bits(nrm2) != bits(default_scene["normals"])).any(1).mean() > 0.99
    assert (bvh2["reorder"] != default_scene["bvh"]["reorder"]).mean() > 0.5
    assert bvh2["nodes"][:1023].tobytes() != default_scene["bvh"]["nodes"][:1023].tobytes()
    return dict(vertices=v2, normals=nrm2, bvh=bvh2)


def default_rt(rtx, tmp_path, w, h, spp=1, name="d.toml"):
    rt = rtx.RayTracer(w, h, rtx.write_config(str(tmp_path / name), w, h, spp=spp)).init()
    rt.set_delta_time(DT)
    return rt


def bin_rt(rtx, tmp_path, path, w=96, h=64, spp=1, name="b.toml", tuning=None):
    rt = rtx.RayTracer(w, h, rtx.write_config(str(tmp_path / name), w, h, spp=spp, mesh_file=path, tuning=tuning)).init()
    rt.set_delta_time(DT)
    return rt


def patch_cameras(rtx, oracle, w, h):
    """The camera of test_gpu_bin_scene.test_bin_terrain_frame, for the renderer and the oracle."""
    cam = rtx.Camera()
    cam.pos[:] = (5.5, 4.0, -3.0)
    cam.yaw, cam.pitch, cam.focal, cam.aperture, cam.fovX = 0.0, -0.55, 5.0, 0.001, np.float32(90.0) * np.float32(0.01745329251)
    oc = oracle.default_camera(w, h)
    oc.pos[:] = (5.5, 4.0, -3.0)
    oc.pitch = -0.55
    return cam, oc


def assert_bvh(rt, rtx, ob, n):
    """NODES (each batch's real nodes), TLAS_NODES, MORTON and REORDER of the last build vs the oracle's."""
    B = ob["batch_count"]
    nodes = rt.download("NODES").view(rtx.NODE_DTYPE)
    for k in range(B):
        cnt = 1024 if k < B - 1 else n - (B - 1) * 1024
        assert nodes[k * 1024:k * 1024 + cnt - 1].tobytes() == ob["nodes"][k * 1024:k * 1024 + cnt - 1].tobytes(), k
    assert rt.download("TLAS_NODES").view(rtx.NODE_DTYPE)[:len(ob["tlas_nodes"])].tobytes() == ob["tlas_nodes"].tobytes()
    assert np.array_equal(rt.download("MORTON", np.uint32)[:B * 1024], ob["morton"])
    assert np.array_equal(rt.download("REORDER", np.uint32)[:B * 1024], ob["reorder"])


def assert_primary_hits(rt, oracle, ob, w, h, oc):
    rt.trace_primary(1)
    hits = rt.download("HITS", np.float32).reshape(-1, 4)
    rays, _ = oracle.primary_rays(w, h, 1, cam=oc)
    oh = oracle.intersect(ob, rays)
    assert oh["hit"].mean() > 0.2
    assert np.array_equal(hits[:, 0].view(np.uint32), oh["t"].view(np.uint32))
    assert np.array_equal(hits[:, 1].view(np.int32), oh["objectIdx"])


def test_shared_vertex_mesh_update_and_rebuild(rtx, oracle, tmp_path, default_scene, moved_scene):
    """Default scene (30,801 vertices = 120 workgroups of 256 + 81, valence 1..11): vertices, normals,
    the rebuilt LBVH and primary hits after a whole-mesh update, then the way back to rt_init's normals."""
    v, i, n = default_scene["vertices"], default_scene["indices"], default_scene["tri_count"]
    v2 = moved_scene["vertices"]
    assert len(v) == 30801 and np.bincount(i[:n].ravel()).max() == 11
    w, h = 192, 108
    rt = default_rt(rtx, tmp_path, w, h)
    oc = oracle.default_camera(w, h)  # looking down on the terrain, as in test_gpu_pathtrace.py
    oc.pos[:] = (8.0, 15.0, -6.0)
    oc.pitch = -0.7
    rc = rtx.Camera()
    rc.pos[:] = (8.0, 15.0, -6.0)
    rc.yaw, rc.pitch, rc.focal, rc.aperture, rc.fovX = 0.0, -0.7, oc.focal, oc.aperture, oc.fovX
    rt.camera = rc
    assert rt.geometry_epoch == 0
    rt.update_vertices(v2)
    assert rt.geometry_epoch == 1
    assert np.array_equal(rt.download("VERTICES", np.float32).reshape(-1, 3), v2)
    assert np.array_equal(bits(rt.download("NORMALS", np.float32).reshape(-1, 3)), bits(moved_scene["normals"]))
    rt.build_bvh()
    assert_bvh(rt, rtx, moved_scene["bvh"], n)
    assert_primary_hits(rt, oracle, moved_scene["bvh"], w, h, oc)
    rt.update_vertices(v)
    assert rt.geometry_epoch == 2
    assert np.array_equal(rt.download("VERTICES", np.float32).reshape(-1, 3), v)
    assert np.array_equal(bits(rt.download("NORMALS", np.float32).reshape(-1, 3)), bits(default_scene["normals"]))
    rt.build_bvh()
    assert_bvh(rt, rtx, default_scene["bvh"], n)
    rt.cleanup()


def test_partial_ranges_and_range_errors(rtx, oracle, tmp_path, default_scene, moved_scene):
    """first = 1, count = nv - 2 and first = nv - 1, count = 1: the vertices outside keep their
    positions, all normals follow the combined array; ranges past the end are refused and change nothing."""
    import torch

    v, i = default_scene["vertices"], default_scene["indices"]
    v2 = moved_scene["vertices"]
    nv = len(v)
    rt = default_rt(rtx, tmp_path, 64, 64)
    comb = v.copy()

    def check():
        assert np.array_equal(rt.download("VERTICES", np.float32).reshape(-1, 3), comb)
        assert np.array_equal(bits(rt.download("NORMALS", np.float32).reshape(-1, 3)), bits(oracle.smooth_normals(comb, i)))

    rt.update_vertices(np.ascontiguousarray(v2[1:nv - 1]), first=1)
    comb[1:nv - 1] = v2[1:nv - 1]
    check()
    assert np.array_equal(comb[0], v[0]) and np.array_equal(comb[nv - 1], v[nv - 1])
    dev = torch.from_numpy(v2).cuda()
    torch.cuda.synchronize()
    rt.update_vertices_device(dev.data_ptr() + 12 * (nv - 1), 1, first=nv - 1)  # the device variant, last vertex
    comb[nv - 1] = v2[nv - 1]
    check()
    assert rt.geometry_epoch == 2
    junk = np.full((nv + 1, 3), 7.0, np.float32)
    djunk = torch.from_numpy(junk).cuda()
    torch.cuda.synchronize()
    L = rt.lib
    for first, count in ((1, nv), (0, nv + 1), (0xFFFFFFFF, 2), (nv, 1), (0, 0)):
        assert L.rt_update_vertices(rt.h, junk.ctypes.data, first, count) == RT_ERR_ARG, (first, count)
        assert L.rt_update_vertices_device(rt.h, djunk.data_ptr(), first, count, None) == RT_ERR_ARG, (first, count)
    assert L.rt_update_vertices_device(rt.h, djunk.data_ptr() + 2, 0, 1, None) == RT_ERR_ARG  # misaligned
    assert rt.geometry_epoch == 2
    check()
    rt.cleanup()


@pytest.mark.parametrize("ntri", [1012, 1010])
def test_unshared_corners_and_padding(rtx, oracle, tmp_path, ntri):
    """A .bin height field (one vertex per corner, valence 1; 1,010 triangles add two padding
    triangles on index 0, whose zero-length edges make vertex 0's normal non-finite in the oracle
    and nowhere else): heights halved by an update equal the oracle and a fresh context loaded from
    a .bin with the new positions — normals, LBVH and primary hits."""
    tris = terrain_patch()[:ntri]
    tris2 = tris.copy()
    tris2[:, :, 1] *= np.float32(0.5)
    path = write_bin(str(tmp_path / "a.bin"), tris)
    path2 = write_bin(str(tmp_path / "b.bin"), tris2)
    v, i, n = read_bin(path)
    v2, i2, _ = read_bin(path2)
    assert len(v) == 3 * ntri and np.array_equal(i, i2) and not np.array_equal(v, v2)
    on2 = oracle.smooth_normals(v2, i)
    odd = np.nonzero(~np.isfinite(on2).all(1))[0]
    assert list(odd) == ([0] if ntri == 1010 else [])
    w, h = 96, 64
    rt = bin_rt(rtx, tmp_path, path, w, h)
    cam, oc = patch_cameras(rtx, oracle, w, h)
    rt.camera = cam
    rt.build_bvh()  # the LBVH of the old heights, so the rebuild below has something to replace
    rt.update_vertices(v2)
    assert np.array_equal(rt.download("VERTICES", np.float32).reshape(-1, 3), v2)
    gn = rt.download("NORMALS", np.float32).reshape(-1, 3)
    nan = np.isnan(on2)
    assert np.array_equal(bits(gn)[~nan], bits(on2)[~nan])
    assert np.isnan(gn[nan]).all()
    rt.build_bvh()
    ob = oracle.build_bvh(v2, i, n, on2)
    assert_bvh(rt, rtx, ob, n)
    assert_primary_hits(rt, oracle, ob, w, h, oc)
    fresh = bin_rt(rtx, tmp_path, path2, w, h, name="fresh.toml")
    fresh.build_bvh()
    for name in ("VERTICES", "NODES", "TLAS_NODES", "MORTON", "REORDER", "AABBS", "TRI_POS"):
        assert np.array_equal(rt.download(name), fresh.download(name)), name
    fn = fresh.download("NORMALS", np.float32).reshape(-1, 3)
    assert np.array_equal(bits(gn)[~nan], bits(fn)[~nan]) and np.isnan(fn[nan]).all()
    fresh.cleanup()
    rt.cleanup()


def _sync_draws(rtx, tmp_path, path, v2, cam, w, h, mode, tuning=None, read_each=False):
    """draw frame 1, update, draw frames 2 and 3 (synchronous device draws, which keep what they
    prepared ahead for the next one).  Without read_each nothing is read between the draws, so the
    LBVH prebuilt and the camera rays traced ahead beside frame 1 are still pending at the update."""
    import torch

    rt = bin_rt(rtx, tmp_path, path, w, h, spp=2, tuning=tuning)
    rt.camera = cam
    targets = [torch.zeros((h, w, 4), dtype=torch.uint8, device="cuda") for _ in range(3)]
    dv2 = torch.from_numpy(v2).cuda()
    torch.cuda.synchronize()
    colors = []
    for f in (1, 2, 3):
        if f == 2:
            if mode == "host":
                rt.update_vertices(v2)
            else:
                rt.update_vertices_device(dv2.data_ptr(), len(v2), 0, None)
        rt.draw_device(targets[f - 1].data_ptr())
        if read_each or f == 3:
            colors.append(rt.get_buffer("RENDER_COLOR", (w * h, 4), np.uint16).copy())
    assert rt.geometry_epoch == 1
    rt.cleanup()
    return [t.cpu().numpy().reshape(-1, 4) for t in targets], colors


def test_synchronous_draws_across_an_update(rtx, oracle, tmp_path):
    """Frame 1 on the patch, frames 2 and 3 on its halved heights: RGBA8 and RENDER_COLOR of each
    frame equal the oracle's path trace + one stateful Denoiser fed BVH(v), BVH(v2), BVH(v2).  A
    renderer that kept the LBVH it prebuilt, or the camera rays it traced ahead, beside frame 1
    would draw frame 2 on the old heights.  With the lookahead off and with the device variant the
    frames are the same bytes."""
    tris = terrain_patch()[:1012]
    tris2 = tris.copy()
    tris2[:, :, 1] *= np.float32(0.5)
    path = write_bin(str(tmp_path / "a.bin"), tris)
    v, i, n = read_bin(path)
    v2 = np.ascontiguousarray(tris2.reshape(-1, 3))
    w, h = 96, 64
    cam, oc = patch_cameras(rtx, oracle, w, h)
    b1 = oracle.build_bvh(v, i, n, oracle.smooth_normals(v, i))
    b2 = oracle.build_bvh(v2, i, n, oracle.smooth_normals(v2, i))
    s, tex = oracle.sky(), oracle.textures()
    dn = oracle.Denoiser(w, h)
    want = []
    for f, b in ((1, b1), (2, b2), (3, b2)):
        gb = oracle.pathtrace(b, w, h, frame_num=f, spp=2, cam=oc, hist_cam=oc, sky_out=s, tex=tex)
        o = dn.draw(gb, f, delta_time=DT)
        want.append((o["rgba"].copy(), o["color"].copy()))
        if f == 2:  # the frame a stale LBVH would give is another one
            stale = oracle.pathtrace(b1, w, h, frame_num=f, spp=2, cam=oc, hist_cam=oc, sky_out=s, tex=tex)
            assert not np.array_equal(stale["color"], gb["color"])
    rgba, color = _sync_draws(rtx, tmp_path, path, v2, cam, w, h, "host", read_each=True)
    for f in range(3):
        assert np.array_equal(rgba[f], want[f][0]), f + 1
        assert np.array_equal(color[f], want[f][1]), f + 1
    runs = [_sync_draws(rtx, tmp_path, path, v2, cam, w, h, "host"),
            _sync_draws(rtx, tmp_path, path, v2, cam, w, h, "host", tuning=dict(syncSpec=False)),
            _sync_draws(rtx, tmp_path, path, v2, cam, w, h, "device")]
    for k, (rg, col) in enumerate(runs):
        for f in range(3):
            assert np.array_equal(rg[f], want[f][0]), (k, f + 1)
        assert np.array_equal(col[0], want[2][1]), k


def _pipeline_run(rtx, tmp_path, seq, w, h, spp, pipelined, events, read_each):
    """FramePipeline frames 1..len(seq) with vertices=seq[f - 1] each.  events: the tensors are
    produced on a second torch stream, each followed by an event there; otherwise they exist before
    the first frame.  read_each: RGBA8, HDR and RENDER_COLOR of every frame (each read drains the
    streams); otherwise only the last frame's, with every update enqueued beside the frames in flight."""
    import torch

    from rtx.frames import FramePipeline

    dev = torch.device("cuda", 0)
    base = [torch.from_numpy(a).to(dev) for a in seq]
    torch.cuda.synchronize()
    rt = default_rt(rtx, tmp_path, w, h, spp=spp)
    prev = torch.cuda.current_stream(0)
    anim = torch.cuda.Stream(dev) if events else None
    fp = FramePipeline(rt, dev, pipelined=pipelined)
    keep, out = [], []

    def read():
        return (rt.download("RGBA8", np.uint8).reshape(-1, 4).copy(), rt.download("HDR", np.uint32).copy(),
                rt.get_buffer("RENDER_COLOR", (w * h, 4), np.uint16).copy())

    try:
        for f, t in enumerate(base, 1):
            ev = None
            if events:
                with torch.cuda.stream(anim):
                    t = t.clone()  # this frame's positions, written on the animation stream
                    ev = torch.cuda.Event()
                    ev.record(anim)
                keep.append(t)
            fp.frame(f, hdr=True, vertices=t, vertices_ready=ev)
            if read_each:
                out.append(read())
        fp.finish()
        if not read_each:
            out.append(read())
        epoch = rt.geometry_epoch
    finally:
        rt.cleanup()
        torch.cuda.set_stream(prev)
    return out, epoch


def test_pipelined_frames_with_an_update_every_frame(rtx, oracle, tmp_path, default_scene, moved_scene):
    """Frames 1..4 at 192x108, 4 spp, positions cycling v, v2, v, v2: the pipelined frames, with a
    ready event per update and without one, equal the serial run byte for byte (every frame when
    read frame by frame, the last one when the four frames and their updates are enqueued without a
    read between them), frame 2 equals the oracle, and four updates were counted."""
    v, v2 = default_scene["vertices"], moved_scene["vertices"]
    seq = [v, v2, v, v2]
    w, h, spp = 192, 108, 4
    serial, epoch = _pipeline_run(rtx, tmp_path, seq, w, h, spp, False, False, True)
    assert epoch == 4
    s, tex = oracle.sky(), oracle.textures()
    cam = oracle.default_camera(w, h)
    dn = oracle.Denoiser(w, h)
    for f, b in ((1, default_scene["bvh"]), (2, moved_scene["bvh"])):
        g = oracle.pathtrace(b, w, h, frame_num=f, spp=spp, cam=cam, hist_cam=cam, sky_out=s, tex=tex)
        o = dn.draw(g, f, delta_time=DT)
        assert np.array_equal(serial[f - 1][0], o["rgba"]), f
        assert np.array_equal(serial[f - 1][2], o["color"]), f
    for events in (True, False):
        each, epoch = _pipeline_run(rtx, tmp_path, seq, w, h, spp, True, events, True)
        assert epoch == 4
        for f in range(4):
            for a, b, what in zip(each[f], serial[f], ("RGBA8", "HDR", "RENDER_COLOR")):
                assert np.array_equal(a, b), (events, f + 1, what)
        last, epoch = _pipeline_run(rtx, tmp_path, seq, w, h, spp, True, events, False)
        assert epoch == 4
        for a, b, what in zip(last[0], serial[3], ("RGBA8", "HDR", "RENDER_COLOR")):
            assert np.array_equal(a, b), (events, "unread", what)


def test_update_with_the_same_positions_changes_nothing(rtx, oracle, tmp_path):
    """update_vertices with the positions the context already has, before frame 1 and again between
    frames 1 and 2: frames 1..3 are byte-identical to a context that never calls it."""
    tris = terrain_patch()[:1012]
    path = write_bin(str(tmp_path / "a.bin"), tris)
    v, _, _ = read_bin(path)
    w, h = 96, 64
    cam, _ = patch_cameras(rtx, oracle, w, h)
    got = []
    for update in (False, True):
        rt = bin_rt(rtx, tmp_path, path, w, h, spp=2)
        rt.camera = cam
        frames = []
        for f in (1, 2, 3):
            if update and f < 3:
                rt.update_vertices(v)
            rgba, hdr = np.zeros((h, w, 4), np.uint8), np.zeros((h, w, 4), np.float32)
            rt.draw(rgba, hdr)
            frames.append((rgba, hdr.view(np.uint32), rt.get_buffer("RENDER_COLOR", (w * h, 4), np.uint16).copy()))
        assert rt.geometry_epoch == (2 if update else 0)
        rt.cleanup()
        got.append(frames)
    for f in range(3):
        for a, b in zip(got[0][f], got[1][f]):
            assert np.array_equal(a, b), f + 1
