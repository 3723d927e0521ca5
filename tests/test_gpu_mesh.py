"""Run-time mesh replacement (rt_set_mesh / rt_set_mesh_device, csrc/mesh.hip) vs numpy and the CPU
oracle, bit for bit: after a set the context holds the vertices, the padded indices, the vertex ->
corner adjacency, the smooth normals and, after the next build, the LBVH and the frames of a context
that rt_init had given the new mesh; frames, prebuilds and ray queries already enqueued keep the
mesh they were issued on.

No expectation comes from the code under test: the adjacency is numpy's stable argsort (and
rt_mesh_adjacency, which test_mesh_api.py pins to it), the rest the oracle's."""
import numpy as np
import pytest

from material_scenes import cube_camera, hashed_ids
from mesh_scenes import ORDER, SHAPES, TOP_NV, grid, numpy_adjacency, pad_indices, welded_cube
from scene_bin import read_bin, terrain_patch, write_bin

pytestmark = pytest.mark.gpu

W, H = 96, 54
DT = 16.667
RT_OK, RT_ERR_ARG = 0, -1


def terrain_camera(rtx, oracle, w, h, pos=(8.0, 15.0, -6.0), yaw=0.0, pitch=-0.7):
    """A camera looking down on the default terrain (as in test_gpu_pathtrace.py)."""
    c = oracle.default_camera(w, h)
    c.pos[:] = pos
    c.yaw = yaw
    c.pitch = pitch
    r = rtx.Camera()
    r.pos[:] = pos
    r.yaw, r.pitch, r.focal, r.aperture, r.fovX = yaw, pitch, c.focal, c.aperture, c.fovX
    return c, r


def gpu_gbuffers(rt, w, h):
    P = w * h
    return dict(color=rt.get_buffer("RENDER_COLOR", (P, 4), np.uint16), normal=rt.get_buffer("NORMAL", (P, 4), np.uint16),
                albedo=rt.get_buffer("ALBEDO", (P, 4), np.uint16), depth=rt.get_buffer("DEPTH", (P,), np.uint16),
                motion=rt.get_buffer("MOTION", (P, 2), np.uint16), rays=rt.download("RAYS", np.uint32)[:P])


def assert_gbuffers_equal(g, o):
    for k in ("color", "normal", "albedo", "depth", "motion", "rays"):
        bad = np.nonzero(np.any((g[k] != o[k]).reshape(g[k].shape[0], -1), axis=1))[0]
        assert bad.size == 0, "%s differs at %d pixels, first %s" % (k, bad.size, bad[:5])


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def assert_normals(rt, want):
    """NORMALS vs the oracle's, bit for bit; where the oracle's are NaN (vertex 0 of a mesh with
    padding triangles, whose edges have no length) the renderer's are NaN too."""
    got = rt.download("NORMALS", np.float32).reshape(-1, 3)
    assert got.shape == want.shape
    nan = np.isnan(want)
    assert np.array_equal(bits(got)[~nan], bits(want)[~nan])
    assert np.isnan(got[nan]).all()


def assert_mesh_arrays(rt, rtx, v, idx):
    """info, VERTICES, INDICES and the adjacency arrays of the current mesh."""
    ip = pad_indices(idx)
    info = rt.info()
    assert (info.triCount, info.triCountPadded, info.batchCount, info.vertexCount) == (
        len(idx), len(ip), (len(idx) + 1023) // 1024, len(v))
    assert np.array_equal(rt.download("VERTICES", np.float32).reshape(-1, 3), v)
    assert np.array_equal(rt.download("INDICES", np.uint32).reshape(-1, 3), ip)
    off, _, slots = rtx.mesh_adjacency(ip, len(v))
    noff, _, nslots = numpy_adjacency(ip, len(v))
    assert np.array_equal(off, noff) and np.array_equal(slots, nslots)
    assert np.array_equal(rt.download("ADJ_OFFSETS", np.uint32), off)
    assert np.array_equal(rt.download("CORNER_SLOTS", np.uint32), slots)
    return ip


def assert_bvh(rt, rtx, ob, n):
    """The BVH arrays of the last build vs the oracle's (NODES: each batch's real nodes)."""
    B = ob["batch_count"]
    nodes = rt.download("NODES").view(rtx.NODE_DTYPE)
    assert len(nodes) == B * 1024
    for k in range(B):
        cnt = 1024 if k < B - 1 else n - (B - 1) * 1024
        assert nodes[k * 1024:k * 1024 + cnt - 1].tobytes() == ob["nodes"][k * 1024:k * 1024 + cnt - 1].tobytes(), k
    assert rt.download("TLAS_NODES").view(rtx.NODE_DTYPE).tobytes() == ob["tlas_nodes"].tobytes()
    assert np.array_equal(rt.download("MORTON", np.uint32), ob["morton"])
    assert np.array_equal(rt.download("REORDER", np.uint32), ob["reorder"])
    assert np.array_equal(bits(rt.download("AABBS", np.float32).reshape(-1, 6)), bits(ob["aabbs"]))
    tp = rt.download("TRI_POS", np.float32).reshape(-1, 3, 4)[:, :, :3].reshape(-1, 9)
    assert np.array_equal(tp, ob["triangles"][:, :9])


def patch_file(tmp_path):
    return write_bin(str(tmp_path / "patch.bin"), terrain_patch()[:1012])


def patch_camera(rtx, oracle):
    """Looking down on a height field of 0.5-unit quads at the origin (terrain_patch, mesh_scenes.grid)."""
    cam = rtx.Camera()
    cam.pos[:] = (5.5, 4.0, -3.0)
    cam.yaw, cam.pitch, cam.focal, cam.aperture, cam.fovX = 0.0, -0.55, 5.0, 0.001, np.float32(90.0) * np.float32(0.01745329251)
    oc = oracle.default_camera(W, H)
    oc.pos[:] = (5.5, 4.0, -3.0)
    oc.pitch = -0.55
    return cam, oc


def patch_rt(rtx, tmp_path, name="p.toml", **kw):
    cfg = rtx.write_config(str(tmp_path / name), W, H, mesh_file=patch_file(tmp_path), **kw)
    rt = rtx.RayTracer(W, H, cfg).init()
    rt.set_delta_time(DT)
    return rt


def oracle_mesh(oracle, v, idx):
    ip = pad_indices(idx)
    nrm = oracle.smooth_normals(v, ip)
    return dict(v=v, idx=idx, ip=ip, normals=nrm, bvh=oracle.build_bvh(v, ip, len(idx), nrm))


def test_adjacency_kernels_on_every_shape(rtx, oracle, tmp_path):
    """set_mesh_device of each shape on one context (maxTriangles 8192, maxVertices 2^21 + 8), in an
    order that shrinks after growing: indices, adjacency and normals each time."""
    import torch

    rt = patch_rt(rtx, tmp_path, max_triangles=8192, max_vertices=TOP_NV)
    wants = {}
    for name in ORDER:
        v, idx = SHAPES[name]()
        if name not in wants:
            wants[name] = oracle.smooth_normals(v, pad_indices(idx))
        dv, di = torch.from_numpy(v).cuda(), torch.from_numpy(idx.astype(np.int32)).cuda()
        torch.cuda.synchronize()
        rt.set_mesh_device(dv.data_ptr(), len(v), di.data_ptr(), len(idx))
        rt.sync()
        assert_mesh_arrays(rt, rtx, v, idx)
        assert_normals(rt, wants[name])
    assert rt.geometry_epoch == len(ORDER)
    rt.cleanup()


def test_setting_the_same_mesh_changes_nothing(rtx, oracle, tmp_path, default_scene):
    """set_mesh of the context's own terrain: every mesh and BVH array and the frame-1 G-buffers equal
    the untouched context's and the oracle's; the epoch is +1."""
    v, ip, n = default_scene["vertices"], default_scene["indices"], default_scene["tri_count"]
    oc, rc = terrain_camera(rtx, oracle, W, H)
    got = []
    for touch in (False, True):
        rt = rtx.RayTracer(W, H, rtx.write_config(str(tmp_path / "d.toml"), W, H)).init()
        rt.camera = rc
        if touch:
            rt.set_mesh(v, np.ascontiguousarray(ip[:n]))
        assert rt.geometry_epoch == (1 if touch else 0)
        rt.build_bvh()
        rt.path_trace(1, detail=True)
        rt.sync()
        arrays = {k: rt.download(k).copy() for k in (
            "VERTICES", "INDICES", "NORMALS", "ADJ_OFFSETS", "CORNER_SLOTS", "TRI_MATERIALS", "TRI_POS", "TRI_NRM",
            "AABBS", "MORTON", "REORDER", "NODES", "TLAS_AABBS", "TLAS_MORTON", "TLAS_REORDER", "TLAS_NODES",
            "TLAS_SCENE_AABB", "BATCH_SCENE_AABBS", "BVH_ARENA")}
        if touch:
            assert_mesh_arrays(rt, rtx, v, ip[:n])
            assert_normals(rt, default_scene["normals"])
            assert_bvh(rt, rtx, default_scene["bvh"], n)
        got.append((arrays, gpu_gbuffers(rt, W, H)))
        rt.cleanup()
    for k in got[0][0]:
        assert np.array_equal(got[0][0][k], got[1][0][k]), k
    o = oracle.pathtrace(default_scene["bvh"], W, H, frame_num=1, cam=oc)
    assert (o["depth"] != o["depth"][0]).any()
    for _, g in got:
        assert_gbuffers_equal(g, o)


def test_terrain_to_cube_and_back(rtx, oracle, tmp_path, default_scene):
    """A default-capacity terrain context (60,800 triangles, 60 batches) takes the welded cube (768
    triangles, one batch) and the terrain again: after each set and build, info, the mesh and BVH
    arrays and the path trace equal the oracle's for that mesh; a mixed material table set before
    is back to 3 everywhere."""
    tv, tip, tn = default_scene["vertices"], default_scene["indices"], default_scene["tri_count"]
    cv, cidx = welded_cube()
    assert cv.shape == (6 * 81, 3) and cidx.shape == (768, 3)
    cube = oracle_mesh(oracle, cv, cidx)
    terrain = dict(v=tv, idx=np.ascontiguousarray(tip[:tn]), ip=tip, normals=default_scene["normals"], bvh=default_scene["bvh"])
    s, tex = oracle.sky(), oracle.textures()
    cams = {"cube": cube_camera(rtx, oracle), "terrain": terrain_camera(rtx, oracle, W, H)}
    rt = rtx.RayTracer(W, H, rtx.write_config(str(tmp_path / "d.toml"), W, H)).init()
    rt.build_bvh()
    rt.set_triangle_materials(hashed_ids(tn, (3, 5, 4, 1)))
    assert (rt.download("TRI_MATERIALS") != 3).any()
    for f, (name, m) in enumerate((("cube", cube), ("terrain", terrain)), 1):
        oc, rc = cams[name]
        rt.set_mesh(m["v"], m["idx"])
        assert_mesh_arrays(rt, rtx, m["v"], m["idx"])
        mats = rt.download("TRI_MATERIALS")
        assert mats.shape == (len(m["idx"]),) and (mats == 3).all()
        assert_normals(rt, m["normals"])
        rt.build_bvh()
        assert_bvh(rt, rtx, m["bvh"], len(m["idx"]))
        rt.camera = rc
        rt.path_trace(f, detail=True)
        rt.sync()
        o = oracle.pathtrace(m["bvh"], W, H, frame_num=f, cam=oc, hist_cam=oc, sky_out=s, tex=tex)
        assert (o["depth"] != o["depth"][0]).any(), name  # the mesh is in view
        g = gpu_gbuffers(rt, W, H)
        for k in ("color", "normal", "albedo", "depth", "rays"):  # the history camera is the previous frame's
            assert np.array_equal(g[k], o[k]), (name, k)
        assert int(rt.download("PT_QUEUE", np.uint32)[10]) == 0
    assert rt.geometry_epoch == 2
    rt.cleanup()


@pytest.fixture(scope="module")
def two_meshes(oracle):
    """Two height fields over the same ground with different batch counts: 2 batches against 1."""
    va, ia = grid(1500, nx=22, seed=11)
    vb, ib = grid(1000, nx=22, seed=12)
    a, b = oracle_mesh(oracle, va, ia), oracle_mesh(oracle, vb, ib)
    assert (a["bvh"]["batch_count"], b["bvh"]["batch_count"]) == (2, 1)
    return a, b


@pytest.mark.parametrize("asynchronous", [True, False], ids=["pipelined", "synchronous"])
def test_frames_in_flight_keep_their_mesh(rtx, oracle, tmp_path, two_meshes, asynchronous):
    """Six frames with the mesh alternating every frame, the device copies produced on a second torch
    stream with an event each and nothing read in between: every frame's target equals the serial
    oracle sequence.  Pipelined draws keep up to four frames in flight across each set; synchronous
    draws have a prebuild and the camera rays traced ahead pending across each set."""
    import torch

    a, b = two_meshes
    cam, oc = patch_camera(rtx, oracle)
    s, tex = oracle.sky(), oracle.textures()
    dn = oracle.Denoiser(W, H)
    want = []
    for f in range(1, 7):
        m = a if f % 2 else b
        gb = oracle.pathtrace(m["bvh"], W, H, frame_num=f, cam=oc, hist_cam=oc, sky_out=s, tex=tex)
        want.append(dn.draw(gb, f, delta_time=DT)["rgba"].copy())
    assert not np.array_equal(want[4], want[5])
    rt = patch_rt(rtx, tmp_path, max_triangles=2048, max_vertices=4096)
    rt.camera = cam
    base = {id(m): (torch.from_numpy(m["v"]).cuda(), torch.from_numpy(m["idx"].astype(np.int32)).cuda()) for m in (a, b)}
    targets = [torch.zeros((H, W, 4), dtype=torch.uint8, device="cuda") for _ in range(6)]
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    keep = []
    for f in range(1, 7):
        m = a if f % 2 else b
        with torch.cuda.stream(side):
            dv, di = (t.clone() for t in base[id(m)])
            ev = torch.cuda.Event()
            ev.record(side)
        keep.append((dv, di, ev))
        rt.set_mesh_device(dv.data_ptr(), len(m["v"]), di.data_ptr(), len(m["idx"]), ev.cuda_event)
        rt.draw_device(targets[f - 1].data_ptr(), asynchronous=asynchronous)
    rt.sync()
    assert rt.geometry_epoch == 6
    got = [t.cpu().numpy().reshape(-1, 4) for t in targets]
    rt.cleanup()
    for f in range(6):
        assert np.array_equal(got[f], want[f]), f + 1


@pytest.mark.parametrize("pipelined", [False, True], ids=["one_stream", "pipelined"])
def test_a_query_holds_its_set(rtx, oracle, tmp_path, two_meshes, pipelined):
    """trace_rays_device on mesh A with no sync, then set_mesh_device(B) and build_bvh, then sync:
    the hits and iteration counts equal rt_trace_rays taken on A beforehand."""
    import torch

    a, b = two_meshes
    cam, oc = patch_camera(rtx, oracle)
    rays, _ = oracle.primary_rays(W, H, 1, cam=oc)
    org, dirs = np.ascontiguousarray(rays[:, :3]), np.ascontiguousarray(rays[:, 3:6])
    rt = patch_rt(rtx, tmp_path, max_triangles=2048, max_vertices=4096)
    rt.set_mesh(a["v"], a["idx"])
    rt.build_bvh()
    t, tri, u, v, iters, _ = rt.trace_rays(org, dirs, want_iters=True)
    oh = oracle.intersect(a["bvh"], rays)
    assert np.array_equal(tri, oh["objectIdx"]) and (tri >= 0).mean() > 0.2
    ob = oracle.intersect(b["bvh"], rays)
    assert not np.array_equal(ob["objectIdx"], oh["objectIdx"])
    post = torch.cuda.Stream() if pipelined else None
    if pipelined:
        rt.set_post_stream(post.cuda_stream)
        rt.build_bvh()  # a pipelined context's build of A, on the side stream
    do, dd = torch.from_numpy(org).cuda(), torch.from_numpy(dirs).cuda()
    hits = torch.zeros((len(org), 4), dtype=torch.float32, device="cuda")
    it = torch.zeros(len(org), dtype=torch.int32, device="cuda")
    dv, di = torch.from_numpy(b["v"]).cuda(), torch.from_numpy(b["idx"].astype(np.int32)).cuda()
    torch.cuda.synchronize()
    rt.trace_rays_device(do.data_ptr(), dd.data_ptr(), len(org), hits.data_ptr(), iters_ptr=it.data_ptr())
    rt.set_mesh_device(dv.data_ptr(), len(b["v"]), di.data_ptr(), len(b["idx"]))
    rt.build_bvh()
    rt.sync()
    h = hits.cpu().numpy()
    assert np.array_equal(bits(h[:, 0]), bits(t)) and np.array_equal(h[:, 1].view(np.int32), tri)
    assert np.array_equal(bits(h[:, 2]), bits(u)) and np.array_equal(bits(h[:, 3]), bits(v))
    assert np.array_equal(it.cpu().numpy().view(np.uint32), iters)
    assert_bvh(rt, rtx, b["bvh"], len(b["idx"]))  # and the build after the set is B's
    if pipelined:
        rt.set_post_stream(None)
    rt.cleanup()


def test_first_frame_after_a_set_has_camera_only_motion(rtx, oracle, tmp_path, two_meshes):
    """Geometry motion vectors on: a vertex update between two builds makes the displacement machinery
    live, then a mesh set: the first build after it records no displacement, and the frame's MOTION
    buffer is the oracle's camera-only one."""
    a, b = two_meshes
    cam, oc = patch_camera(rtx, oracle)
    rt = patch_rt(rtx, tmp_path, max_triangles=2048, max_vertices=4096, geometry_motion=True)
    rt.camera = cam
    rt.set_mesh(a["v"], a["idx"])
    rt.build_bvh()
    rt.path_trace(1)
    moved = a["v"].copy()
    moved[:, 1] += np.float32(0.25)
    rt.update_vertices(moved)
    rt.build_bvh()
    rt.path_trace(2)
    rt.set_mesh(b["v"], b["idx"])
    rt.build_bvh()
    rt.path_trace(3, detail=True)
    rt.sync()
    o = oracle.pathtrace(b["bvh"], W, H, frame_num=3, cam=oc, hist_cam=oc)
    assert_gbuffers_equal(gpu_gbuffers(rt, W, H), o)
    assert (o["motion"] != o["motion"][0]).any()
    rt.cleanup()


def test_errors_leave_the_mesh_unchanged(rtx, oracle, tmp_path):
    """Counts over the capacity, a single triangle and (host variant) an index equal to vertex_count are
    argument errors that change nothing.  The device variant cannot see its indices: three such
    indices are read as 0, the call returns RT_OK, the next sync reports RT_ERR_DEVICE once, naming 3."""
    import torch

    v0, i0, n0 = read_bin(patch_file(tmp_path))
    rt = patch_rt(rtx, tmp_path, max_triangles=2048, max_vertices=4096)
    v, idx = grid(600)
    dv, di = torch.from_numpy(v).cuda(), torch.from_numpy(idx.astype(np.int32)).cuda()
    big = torch.zeros(3 * 4097, dtype=torch.float32, device="cuda")
    bigi = torch.zeros(3 * 2049, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    L = rt.lib

    def unchanged():
        assert rt.geometry_epoch == 0
        assert_mesh_arrays(rt, rtx, v0, i0[:n0])

    bad = idx.copy()
    bad[17, 1] = len(v)
    hv, hi = np.zeros((4097, 3), np.float32), np.zeros((2049, 3), np.uint32)
    for fn, args in (
            ("rt_set_mesh_device", (dv.data_ptr(), len(v), bigi.data_ptr(), 2049)),
            ("rt_set_mesh_device", (big.data_ptr(), 4097, di.data_ptr(), len(idx))),
            ("rt_set_mesh_device", (dv.data_ptr(), len(v), di.data_ptr(), 1)),
            ("rt_set_mesh", (v.ctypes.data, len(v), hi.ctypes.data, 2049)),
            ("rt_set_mesh", (hv.ctypes.data, 4097, idx.ctypes.data, len(idx))),
            ("rt_set_mesh", (v.ctypes.data, len(v), idx.ctypes.data, 1)),
            ("rt_set_mesh", (v.ctypes.data, len(v), bad.ctypes.data, len(bad)))):
        m = rtx.Mesh(args[0], args[1], args[2], args[3], None)
        assert getattr(L, fn)(rt.h, m) == RT_ERR_ARG, (fn, args[1], args[3])
        assert fn.encode() in L.rt_last_error(rt.h)
    rt.sync()
    unchanged()
    for c in ((17, 1), (200, 0), (599, 2)):
        bad[c] = len(v)
    fixed = bad.copy()
    fixed[bad == len(v)] = 0
    dbad = torch.from_numpy(bad.astype(np.int32)).cuda()
    torch.cuda.synchronize()
    rt.set_mesh_device(dv.data_ptr(), len(v), dbad.data_ptr(), len(bad))  # RT_OK
    with pytest.raises(rtx.RtError, match=r"rt_sync: RT_ERR_DEVICE .* 3 index"):
        rt.sync()
    rt.sync()  # reported once
    assert_mesh_arrays(rt, rtx, v, fixed)
    assert_normals(rt, oracle.smooth_normals(v, pad_indices(fixed)))
    rt.sync()
    rt.cleanup()
