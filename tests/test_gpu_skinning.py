"""Skinned meshes on the device (rt_set_skin / rt_pose_skin / rt_pose_skin_device, csrc/skin.hip): a posed
context holds, bit for bit, what a context given the host rule's positions through update_vertices* holds
— vertices, normals, epoch, LBVH, frames, motion vectors — in synchronous draws, which prepare work ahead
of the pose, and in pipelined frames with a pose in flight every frame.

The positions come from rtx.skin_vertices (the rule compiled for the host), which test_skinning_api.py
pins to a numpy restatement; the two small meshes are compared with that restatement here as well."""
import ctypes as C

import numpy as np
import pytest

from mesh_scenes import grid, soup2
from scene_bin import terrain_patch, write_bin
from skin_scenes import F, identity, random_pose, random_skin, rotation, rule32, scale, translation

pytestmark = pytest.mark.gpu

W, H = 96, 64
DT = 16.667
RT_OK, RT_ERR_ARG, RT_ERR_STATE = 0, -1, -4


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def patch_camera(rtx):
    """Looking down on a height field of 0.5-unit quads at the origin (terrain_patch, mesh_scenes.grid)."""
    cam = rtx.Camera()
    cam.pos[:] = (5.5, 4.0, -3.0)
    cam.yaw, cam.pitch, cam.focal, cam.aperture, cam.fovX = 0.0, -0.55, 5.0, 0.001, np.float32(90.0) * np.float32(0.01745329251)
    return cam


def mesh_rt(rtx, tmp_path, mesh=None, name="m.toml", **kw):
    """A 96 x 64 context: the default scene (mesh None), or the terrain patch's .bin with room for a
    set_mesh of `mesh` = (vertices, indices)."""
    if mesh is None:
        cfg = rtx.write_config(str(tmp_path / name), W, H, **kw)
    else:
        path = write_bin(str(tmp_path / "patch.bin"), terrain_patch()[:1012])
        cfg = rtx.write_config(str(tmp_path / name), W, H, mesh_file=path, max_triangles=2048, max_vertices=4096, **kw)
    rt = rtx.RayTracer(W, H, cfg).init()
    rt.set_delta_time(DT)
    if mesh is not None:
        rt.camera = patch_camera(rtx)
        rt.set_mesh(*mesh)
    return rt


def arrays(rt):
    return (rt.download("VERTICES", np.uint32).copy(), rt.download("NORMALS", np.uint32).copy(), rt.geometry_epoch)


def grid_poses(n, nj=3):
    """n gentle poses of nj joints about the grid: the frames differ, the mesh stays in view."""
    out = []
    for k in range(n):
        m = np.stack([rotation((0, 0, 1), 0.04 * (k + 1), (5.5, 0.0, 3.5)),
                      translation((0.0, 0.125 * (k + 1), 0.0)),
                      scale(1.0, 1.0 + 0.1 * (k + 1), 1.0)][:nj]).astype(F)
        out.append(np.ascontiguousarray(m))
    return out


@pytest.fixture(scope="module")
def grid_skin():
    v, idx = grid(600)
    assert len(v) == 360  # one full workgroup and a tail of 104
    rest, joints, weights = random_skin(len(v), 3, seed=21, rest=v)
    return dict(mesh=(v, idx), rest=rest, joints=joints, weights=weights)


# ---------------------------------------------------------------- 1
@pytest.mark.parametrize("which", ["soup2", "grid600", "default"])
def test_posed_positions_normals_epoch_and_lbvh(rtx, tmp_path, default_scene, which):
    """set_skin + pose_skin against update_vertices of the host rule's positions on a second context, for
    1, 3 and 4096 joints (the last joint named): VERTICES, NORMALS, epoch + 1, and the next build."""
    mesh = dict(soup2=soup2, grid600=lambda: grid(600), default=lambda: None)[which]()
    rt = mesh_rt(rtx, tmp_path, mesh, "a.toml")
    ref = mesh_rt(rtx, tmp_path, mesh, "b.toml")
    v = mesh[0] if mesh is not None else default_scene["vertices"]
    nv = len(v)
    assert nv == dict(soup2=6, grid600=360, default=30801)[which] == rt.info().vertexCount
    for nj in (1, 3, 4096):
        rest, joints, weights = random_skin(nv, nj, seed=nj + nv, rest=v)
        assert nj == 1 or (joints[weights != 0] == nj - 1).any()
        pose = random_pose(nj, seed=7 * nj, amount=0.3)
        want = rtx.skin_vertices(rest, joints, weights, pose)
        assert not np.array_equal(want, v)
        if which != "default":
            assert np.array_equal(bits(want), bits(rule32(rest, joints, weights, pose)))
        rt.set_skin(rest, joints, weights, nj)
        assert rt.skin == (nv, nj)
        e0 = rt.geometry_epoch
        assert np.array_equal(rt.download("VERTICES", np.float32).reshape(-1, 3), ref.download("VERTICES", np.float32).reshape(-1, 3))
        rt.pose_skin(pose)
        assert rt.geometry_epoch == e0 + 1
        assert np.array_equal(bits(rt.download("VERTICES", np.float32).reshape(-1, 3)), bits(want)), nj
        ref.update_vertices(want)
        assert np.array_equal(rt.download("NORMALS", np.uint32), ref.download("NORMALS", np.uint32)), nj
        rt.build_bvh()
        ref.build_bvh()
        for name in ("NODES", "TLAS_NODES", "MORTON", "REORDER"):
            assert np.array_equal(rt.download(name), ref.download(name)), (nj, name)
    rt.cleanup()
    ref.cleanup()


# ---------------------------------------------------------------- 2
def test_device_pose_equals_host_pose(rtx, tmp_path, grid_skin):
    import torch

    g = grid_skin
    rt = mesh_rt(rtx, tmp_path, g["mesh"])
    rt.set_skin(g["rest"], g["joints"], g["weights"], 3)
    e0 = rt.geometry_epoch
    p1, p2 = grid_poses(2)
    rt.pose_skin(p1)
    a1 = arrays(rt)
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        d2 = torch.from_numpy(p2).cuda()
        ev = torch.cuda.Event()
        ev.record(side)
    rt.pose_skin_device(d2, 3, ev.cuda_event)
    got2 = arrays(rt)
    rt.pose_skin(p2)
    a2 = arrays(rt)
    assert not np.array_equal(a1[0], a2[0])
    assert np.array_equal(got2[0], a2[0]) and np.array_equal(got2[1], a2[1])
    assert np.array_equal(bits(rtx.skin_vertices(g["rest"], g["joints"], g["weights"], p2)).ravel(), a2[0])
    d1 = torch.from_numpy(np.concatenate([p1.reshape(3, 12), np.zeros((1, 12), F)])).cuda()
    torch.cuda.synchronize()
    rt.pose_skin_device(d1.data_ptr(), 3)  # no event: behind the context stream
    got1 = arrays(rt)
    assert np.array_equal(got1[0], a1[0]) and np.array_equal(got1[1], a1[1])
    assert (a1[2], got2[2], a2[2], got1[2]) == (e0 + 1, e0 + 2, e0 + 3, e0 + 4)
    for off in (4, 8, 12):  # not 16-byte aligned: refused, nothing changes
        bad = rtx.Pose(d1.data_ptr() + off, 3, None)
        assert rt.lib.rt_pose_skin_device(rt.h, C.byref(bad)) == RT_ERR_ARG, off
    bad = rtx.Pose(d1.data_ptr(), 2, None)  # not the skin's joint count
    assert rt.lib.rt_pose_skin_device(rt.h, C.byref(bad)) == RT_ERR_ARG
    after = arrays(rt)
    assert after[2] == e0 + 4 and np.array_equal(after[0], a1[0]) and np.array_equal(after[1], a1[1])
    rt.cleanup()


# ---------------------------------------------------------------- 3
def _pipeline_run(rtx, tmp_path, g, name, seq, posed, read_each):
    """FramePipeline(pipelined=True) frames 1..len(seq), frame f fed pose= (posed) or vertices= seq[f - 1],
    each produced on a second torch stream and followed by an event there.  read_each: RGBA8 and HDR of every
    frame (each read drains the streams); otherwise the last frame's, every pose enqueued beside frames in flight."""
    import torch

    from rtx.frames import FramePipeline

    dev = torch.device("cuda", 0)
    base = [torch.from_numpy(np.ascontiguousarray(a)).to(dev) for a in seq]
    torch.cuda.synchronize()
    rt = mesh_rt(rtx, tmp_path, g["mesh"], name, spp=2)
    if posed:
        rt.set_skin(g["rest"], g["joints"], g["weights"], 3)
    prev = torch.cuda.current_stream(0)
    anim = torch.cuda.Stream(dev)
    fp = FramePipeline(rt, dev, pipelined=True)
    keep, out = [], []

    def read():
        return rt.download("RGBA8", np.uint8).reshape(-1, 4).copy(), rt.download("HDR", np.uint32).copy()

    try:
        for f, t in enumerate(base, 1):
            with torch.cuda.stream(anim):
                t = t.clone()  # this frame's matrices or positions, written on the animation stream
                ev = torch.cuda.Event()
                ev.record(anim)
            keep.append(t)
            if posed:
                fp.frame(f, hdr=True, pose=t, pose_ready=ev)
            else:
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


def test_pipelined_frames_with_a_pose_every_frame(rtx, tmp_path, grid_skin):
    """Six pipelined frames on grid(600), a different pose each: every frame equals the frame of a pipeline
    fed vertices= with the host rule's positions, read frame by frame and with nothing read in between."""
    import torch

    g = grid_skin
    poses = grid_poses(6)
    positions = [rtx.skin_vertices(g["rest"], g["joints"], g["weights"], p) for p in poses]
    want, epoch = _pipeline_run(rtx, tmp_path, g, "v.toml", positions, False, True)
    assert epoch == 7  # the mesh set and six updates
    assert all(not np.array_equal(a[0], b[0]) for a, b in zip(want, want[1:]))  # the poses show
    got, epoch = _pipeline_run(rtx, tmp_path, g, "p.toml", poses, True, True)
    assert epoch == 7
    for f in range(6):
        for a, b, what in zip(got[f], want[f], ("RGBA8", "HDR")):
            assert np.array_equal(a, b), (f + 1, what)
    last, epoch = _pipeline_run(rtx, tmp_path, g, "u.toml", poses, True, False)
    assert epoch == 7
    for a, b, what in zip(last[0], want[5], ("RGBA8", "HDR")):
        assert np.array_equal(a, b), ("unread", what)
    # pose and vertices together are refused before anything is enqueued
    from rtx.frames import FramePipeline

    class _NoRenderer:
        def __getattr__(self, name):
            raise AssertionError("frame() called %s" % name)

    fp = FramePipeline.__new__(FramePipeline)
    fp.rt = _NoRenderer()
    t = torch.zeros((3, 12), dtype=torch.float32, device="cuda")
    with pytest.raises(ValueError):
        fp.frame(1, pose=t, vertices=torch.zeros((4, 3), dtype=torch.float32, device="cuda"))
    with pytest.raises(ValueError):
        fp.frame(1, pose=torch.zeros((3, 16), dtype=torch.float32, device="cuda"))


# ---------------------------------------------------------------- 4
def _hdr_draw(rt):
    hdr = np.zeros((H, W, 4), np.float32)
    rt.draw(None, hdr)  # keeps what it launched ahead alive: no read of the context follows
    return hdr.view(np.uint32)


def _no_temporal(rt):
    p = rt.params
    p.pass_.enableTemporalDenoising = 0
    p.pass_.enableTemporalDenoising2 = 0
    p.pass_.enableAutoExposure = 0
    rt.params = p


def test_synchronous_draws_across_a_pose(rtx, tmp_path, grid_skin):
    """draw, pose, draw.  The first draw traced the next frame's camera rays ahead on the rest pose: the
    second drops them (SPEC_STATS) and shows the pose.  Its HDR equals that of a context that launches
    nothing ahead through the same calls, and, with the passes that carry state from frame to frame
    (temporal filters, auto exposure) off, that of a fresh context posed before its first draw and set to
    the same frame index."""
    g = grid_skin
    pose = grid_poses(3)[2]

    def run(name, tuning, temporal, fresh=False):
        rt = mesh_rt(rtx, tmp_path, g["mesh"], name, spp=2, tuning=tuning)
        if not temporal:
            _no_temporal(rt)
        rt.set_skin(g["rest"], g["joints"], g["weights"], 3)
        frames = []
        if fresh:
            rt.pose_skin(pose)
            rt.set_frame_index(2)
            frames.append(_hdr_draw(rt))
        else:
            frames.append(_hdr_draw(rt))
            rt.pose_skin(pose)
            frames.append(_hdr_draw(rt))
        stats = rt.download("SPEC_STATS", np.uint32).tolist()
        rt.cleanup()
        return frames, stats

    on, stats = run("on.toml", {"syncSpec": True}, True)
    assert stats[:3] == [2, 0, 1], stats  # launched by both draws; the first one's dropped, not reused
    assert not np.array_equal(on[0], on[1])
    off, off_stats = run("off.toml", {"syncSpec": False}, True)
    assert off_stats[:3] == [0, 0, 0]
    assert np.array_equal(on[0], off[0]) and np.array_equal(on[1], off[1])
    plain, stats = run("plain.toml", {"syncSpec": True}, False)
    assert stats[:3] == [2, 0, 1], stats
    fresh, _ = run("fresh.toml", {"syncSpec": True}, False, fresh=True)
    assert np.array_equal(plain[1], fresh[0])


# ---------------------------------------------------------------- 5
def test_geometry_motion_follows_a_pose(rtx, tmp_path, grid_skin):
    """geometry_motion on; draw, pose, draw: MOTION and the HDR equal those of a context that received the
    same positions by update_vertices_device."""
    import torch

    g = grid_skin
    pose = grid_poses(2)[1]
    want = rtx.skin_vertices(g["rest"], g["joints"], g["weights"], pose)
    dwant = torch.from_numpy(want).cuda()
    torch.cuda.synchronize()
    res = []
    for posed in (True, False):
        rt = mesh_rt(rtx, tmp_path, g["mesh"], "m%d.toml" % posed, spp=2)
        rt.geometry_motion = True
        rt.set_skin(g["rest"], g["joints"], g["weights"], 3)
        first = _hdr_draw(rt)
        if posed:
            rt.pose_skin(pose)
        else:
            rt.update_vertices_device(dwant.data_ptr(), len(want))
        second = _hdr_draw(rt)
        res.append((first, second, rt.get_buffer("MOTION", (W * H, 2), np.uint16).copy()))
        rt.cleanup()
    static = res[1][2]
    for a, b, what in zip(res[0], res[1], ("frame 1", "frame 2", "MOTION")):
        assert np.array_equal(a, b), what
    # the motion buffer does follow the vertices: without the feature it is the still camera's
    rt = mesh_rt(rtx, tmp_path, g["mesh"], "still.toml", spp=2)
    _hdr_draw(rt)
    rt.update_vertices(want)
    _hdr_draw(rt)
    assert not np.array_equal(rt.get_buffer("MOTION", (W * H, 2), np.uint16), static)
    rt.cleanup()


# ---------------------------------------------------------------- 6
def test_nan_matrix_of_an_unweighted_joint_reaches_no_vertex(rtx, tmp_path, grid_skin):
    g = grid_skin
    joints = g["joints"].copy()
    joints[g["weights"] == 0] = 3  # joint 3: named by zero-weight slots only
    assert (joints == 3).sum() > 100
    pose = np.concatenate([grid_poses(1)[0], np.full((1, 3, 4), np.nan, F)])
    rt = mesh_rt(rtx, tmp_path, g["mesh"])
    rt.set_skin(g["rest"], joints, g["weights"], 4)
    rt.pose_skin(pose)
    got = rt.download("VERTICES", np.float32).reshape(-1, 3)
    assert np.isfinite(got).all()
    assert np.array_equal(bits(got), bits(rtx.skin_vertices(g["rest"], joints, g["weights"], pose)))
    assert np.array_equal(bits(got), bits(rule32(g["rest"], joints, g["weights"], pose)))
    rt.cleanup()


# ---------------------------------------------------------------- 7
def test_skin_lifecycle(rtx, tmp_path, grid_skin):
    g = grid_skin
    v, idx = g["mesh"]
    nv = len(v)
    rt = mesh_rt(rtx, tmp_path, g["mesh"])
    assert rt.skin == (0, 0)
    with pytest.raises(rtx.RtError, match="rt_pose_skin: RT_ERR_STATE"):
        rt.pose_skin(identity(3))
    rt.set_skin(g["rest"], g["joints"], g["weights"], 3)
    e0 = rt.geometry_epoch
    before = arrays(rt)
    # a skin of another vertex count, or naming a joint it does not have: refused, the skin stays
    for n in (nv - 1, nv + 1):
        r2, j2, w2 = random_skin(n, 3, seed=1)
        with pytest.raises(rtx.RtError, match="rt_set_skin: RT_ERR_ARG"):
            rt.set_skin(r2, j2, w2, 3)
    j2 = g["joints"].copy()
    j2[nv - 1, 0] = 3
    with pytest.raises(rtx.RtError, match="rt_set_skin: RT_ERR_ARG"):
        rt.set_skin(g["rest"], j2, g["weights"], 3)
    assert rt.skin == (nv, 3) and rt.geometry_epoch == e0
    after = arrays(rt)
    assert np.array_equal(after[0], before[0]) and np.array_equal(after[1], before[1])
    p1, p2 = grid_poses(2)
    rt.pose_skin(p1)
    assert np.array_equal(bits(rt.download("VERTICES", np.float32).reshape(-1, 3)),
                          bits(rtx.skin_vertices(g["rest"], g["joints"], g["weights"], p1)))
    # update_vertices between two poses overrides until the next pose, which starts from the rest pose
    junk = np.full((nv, 3), 2.5, F)
    rt.update_vertices(junk)
    assert np.array_equal(rt.download("VERTICES", np.float32).reshape(-1, 3), junk)
    rt.pose_skin(p2)
    assert np.array_equal(bits(rt.download("VERTICES", np.float32).reshape(-1, 3)),
                          bits(rtx.skin_vertices(g["rest"], g["joints"], g["weights"], p2)))
    # a mesh set drops the skin; a new one for the new, smaller mesh poses it
    sv, sidx = soup2()
    rt.set_mesh(sv, sidx)
    assert rt.skin == (0, 0)
    with pytest.raises(rtx.RtError, match="rt_pose_skin: RT_ERR_STATE"):
        rt.pose_skin(p2)
    with pytest.raises(rtx.RtError, match="rt_set_skin: RT_ERR_ARG"):
        rt.set_skin(g["rest"], g["joints"], g["weights"], 3)  # the old mesh's count
    r3, j3, w3 = random_skin(len(sv), 2, seed=4, rest=sv)
    rt.set_skin(r3, j3, w3, 2)
    assert rt.skin == (6, 2)
    p3 = random_pose(2, seed=8, amount=0.5)
    rt.pose_skin(p3)
    got = rt.download("VERTICES", np.float32).reshape(-1, 3)
    assert got.shape == (6, 3)
    assert np.array_equal(bits(got), bits(rtx.skin_vertices(r3, j3, w3, p3)))
    ref = mesh_rt(rtx, tmp_path, (sv, sidx), "ref.toml")
    ref.update_vertices(rtx.skin_vertices(r3, j3, w3, p3))
    assert np.array_equal(rt.download("NORMALS", np.uint32), ref.download("NORMALS", np.uint32))
    ref.cleanup()
    rt.reset_skin()
    assert rt.skin == (0, 0)
    with pytest.raises(rtx.RtError, match="rt_pose_skin: RT_ERR_STATE"):
        rt.pose_skin(p3)
    rt.cleanup()


# ---------------------------------------------------------------- 8
def test_stage_8_times_a_pose_and_changes_nothing(rtx, tmp_path, grid_skin):
    g = grid_skin
    rt = mesh_rt(rtx, tmp_path, g["mesh"])
    with pytest.raises(rtx.RtError, match="rt_time_stage: RT_ERR_STATE"):
        rt.time_stage(8, 1)
    rt.set_skin(g["rest"], g["joints"], g["weights"], 3)
    before = arrays(rt)
    assert rt.time_stage(8, 3) > 0.0  # identity: no pose yet
    now = arrays(rt)
    assert now[2] == before[2] and np.array_equal(now[0], before[0]) and np.array_equal(now[1], before[1])
    rt.pose_skin(grid_poses(1)[0])
    rt.update_vertices(np.full((360, 3), 1.5, F) + g["rest"])  # the arrays are no longer the staged pose's
    before = arrays(rt)
    assert rt.time_stage(8, 3) > 0.0
    now = arrays(rt)
    assert now[2] == before[2] and np.array_equal(now[0], before[0]) and np.array_equal(now[1], before[1])
    rt.cleanup()
