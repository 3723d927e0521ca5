"""Stream-ordered triangle materials (rt_set_triangle_materials_device, csrc/materials.hip; DESIGN.md
§4.1.3), bit for bit.

No expectation comes from the new call: tables and censuses are numpy's, frames are the oracle's
(composed as material_scenes.py composes them) or, where paths cross types and no oracle exists, those
of a second context driven through the synchronous host setter.  Every path-trace launch that is read
must leave the internal error counter PT_QUEUE[10] at 0.
"""
import numpy as np
import pytest

import material_scenes as M
from mesh_scenes import grid, welded_cube
from test_gpu_materials import DT, MIX8, cube, cube_rt, sky_tex, terrain_rt, trace, with_mask  # noqa: F401 (fixtures)
from test_gpu_mesh import patch_camera, patch_rt
from test_gpu_pathtrace import assert_gbuffers_equal

pytestmark = pytest.mark.gpu

W, H = 96, 54
FACES_A = {"x+": 5, "y+": 3, "z-": 4}
FACES_B = {"x+": 4, "y+": 5, "z-": 3}


def to_dev(*arrays):
    import torch

    out = [torch.from_numpy(np.ascontiguousarray(a)).cuda() for a in arrays]
    torch.cuda.synchronize()
    return out if len(out) > 1 else out[0]


def dev_set(rtx, rt, ids, first=0, classes=None, keep=None):
    """One device set of a numpy id array (uploaded and complete before the call)."""
    d = to_dev(ids)
    if keep is not None:
        keep.append(d)
    rt.set_triangle_materials_device(d.data_ptr(), len(ids), first,
                                     rtx.material_classes(ids) if classes is None else classes)
    return d


def census_of(table):
    return np.bincount(table, minlength=256).astype(np.uint32)


def assert_table(rt, want):
    assert np.array_equal(rt.download("TRI_MATERIALS"), want)
    assert np.array_equal(rt.download("TRI_MATERIAL_CENSUS", np.uint32), census_of(want))


def scene_rt(rtx, oracle, tmp_path, cube, name):
    if name == "cube":
        return cube_rt(rtx, oracle, tmp_path, cube)
    if name == "patch":
        return patch_rt(rtx, tmp_path)
    return rtx.RayTracer(W, H, rtx.write_config(str(tmp_path / "t.toml"), W, H)).init()


@pytest.mark.parametrize("scene,n", [("cube", 768), ("patch", 1012), ("terrain", 60800)])
def test_merge_kernel_on_every_shape(rtx, oracle, tmp_path, cube, scene, n):
    """Tables and censuses against numpy after every set: a partial first set lands among 3s, later
    ones accumulate; head and tail lanes, ranges inside one 16-byte group and across groups and
    workgroups, sources offset by 1, 2 and 3 bytes into a larger tensor; then a burst of sets with
    nothing read in between (the pool's buffers in turn)."""
    import torch

    rt = scene_rt(rtx, oracle, tmp_path, cube, scene)
    assert rt.info().triCount == n
    assert_table(rt, np.full(n, 3, np.uint8))
    rng = np.random.default_rng(n)
    want = np.full(n, 3, np.uint8)
    keep = []
    for first, count in ((13, 40), (0, n), (0, 1), (n - 1, 1), (1, 5), (15, 2), (13, 40), (127, 130)):
        ids = rng.integers(0, 256, count, dtype=np.uint8)
        dev_set(rtx, rt, ids, first, rtx.MAT_CLASS_ALL, keep)
        want[first:first + count] = ids
        assert_table(rt, want)
    big = rng.integers(0, 256, n + 64, dtype=np.uint8)
    dbig = to_dev(big)
    for off, (first, count) in ((1, (0, n)), (2, (13, 40)), (3, (127, 130)), (3, (n - 7, 7)), (1, (16, 16))):
        rt.set_triangle_materials_device(dbig.data_ptr() + off, count, first, rtx.MAT_CLASS_ALL)
        want[first:first + count] = big[off:off + count]
        assert_table(rt, want)
    for k in range(7):
        first, count = (5 * k + 1) % n, min(n - (5 * k + 1) % n, 100 + 37 * k)
        rt.set_triangle_materials_device(dbig.data_ptr() + 2 * k, count, first, rtx.MAT_CLASS_ALL)
        want[first:first + count] = big[2 * k:2 * k + count]
    assert_table(rt, want)
    torch.cuda.synchronize()
    rt.cleanup()


def test_equals_the_host_setter(rtx, oracle, tmp_path, cube, sky_tex):
    """Two contexts render the same table, one through each call, with rt_material_classes of the table
    declared: G-buffers, RAYS and lastChain are equal; the cube's face table also equals the oracle's
    composite."""
    s, tex = sky_tex
    w, h = M.CUBE_W, M.CUBE_H
    ocam, rcam = M.cube_camera(rtx, oracle)
    face = M.face_table(FACES_A)
    for table in (np.full(768, 5, np.uint8), face):
        got = []
        for device in (False, True):
            rt = cube_rt(rtx, oracle, tmp_path, cube)
            rt.camera = rcam
            rt.build_bvh()
            if device:
                dev_set(rtx, rt, table)
            else:
                rt.set_triangle_materials(table)
            got.append((trace(rt, 1, w, h), rt.info().lastChain))
            assert_table(rt, table)
            rt.cleanup()
        assert_gbuffers_equal(got[1][0], got[0][0])
        assert got[1][1] == got[0][1] == 0
    frames = {m: oracle.pathtrace(cube["bvh"], w, h, frame_num=1, cam=ocam, sky_out=s, tex=tex, material_override=m)
              for m in set(FACES_A.values())}
    tri = cube["tri"]
    pick = np.where(tri >= 0, face[np.maximum(tri, 0)], 5).astype(np.int64)
    assert_gbuffers_equal(got[1][0], M.compose_by_pixel(frames, pick))
    got = []
    for device in (False, True):  # paths that cross between the types: the hashed eight-way mix, spp 2
        rt, _ = terrain_rt(rtx, oracle, tmp_path, "m%d" % device, spp=2)
        ids = M.hashed_ids(rt.info().triCount, MIX8)
        if device:
            dev_set(rtx, rt, ids)
        else:
            rt.set_triangle_materials(ids)
        got.append((trace(rt, 2), rt.info().lastChain))
        rt.cleanup()
    assert_gbuffers_equal(got[1][0], got[0][0])
    assert got[1][1] == got[0][1] == 0
    assert got[0][0]["rays"].max() >= 4


def test_over_declared_classes_change_only_the_plan(rtx, oracle, tmp_path, default_scene, sky_tex):
    """The Lambertian 3 / 7 / 9 table declared RT_MAT_CLASS_ALL runs the glossy microfacet kernels and
    equals the oracle's override-3 frame with the table's mask, in every buffer and in RAYS."""
    s, tex = sky_tex
    rt, ocam = terrain_rt(rtx, oracle, tmp_path, "o")
    n = rt.info().triCount
    ids = M.hashed_ids(n, (3, 7, 9))
    assert rtx.material_classes(ids) == 0
    dev_set(rtx, rt, ids, classes=rtx.MAT_CLASS_ALL)
    g = trace(rt, 1)
    assert rt.info().lastChain == 0  # the declared plan, not the census'
    dev_set(rtx, rt, ids, classes=0)
    g0 = trace(rt, 1)
    assert rt.info().lastChain == 1
    rt.cleanup()
    o = oracle.pathtrace(default_scene["bvh"], W, H, frame_num=1, cam=ocam, sky_out=s, tex=tex, material_override=3)
    tri = M.primary_triangles(oracle, default_scene["bvh"], W, H, ocam)
    mask = np.where(tri >= 0, ids.astype(np.int64)[np.maximum(tri, 0)], M.SKY_MASK).astype(np.uint16)
    assert len(set(mask[tri >= 0].tolist())) == 3
    assert_gbuffers_equal(g, with_mask(o, mask))
    assert_gbuffers_equal(g0, with_mask(o, mask))


def serial_cube_frames(rtx, oracle, tmp_path, cube, tables, cams):
    """RGBA8 of frames 1.. of a context that gets tables[k] through the host setter before draw k."""
    rt = cube_rt(rtx, oracle, tmp_path, cube)
    out = []
    rgba = np.zeros((M.CUBE_H, M.CUBE_W, 4), np.uint8)
    for table, k in zip(tables, cams):
        rt.camera = M.cube_camera(rtx, oracle, k)[1]
        rt.set_triangle_materials(table)
        rt.draw(rgba)
        out.append(rgba.reshape(-1, 4).copy())
    assert rt.download("PT_QUEUE", np.uint32)[10] == 0
    rt.cleanup()
    return out


@pytest.mark.parametrize("asynchronous", [True, False], ids=["pipelined", "synchronous"])
def test_frames_in_flight_keep_their_table(rtx, oracle, tmp_path, cube, asynchronous):
    """Six cube frames with a moving camera, two face tables alternating every frame, the ids cloned on
    a second torch stream with an event each and nothing read in between: every frame's RGBA8 equals
    the serial sequence of the host setter."""
    import torch

    tabs = [M.face_table(FACES_A), M.face_table(FACES_B)]
    classes = rtx.material_classes(tabs[0])
    assert classes == rtx.material_classes(tabs[1]) == rtx.MAT_CLASS_ALL
    want = serial_cube_frames(rtx, oracle, tmp_path, cube, [tabs[f % 2] for f in range(6)], range(6))
    assert not np.array_equal(want[4], want[5])
    rt = cube_rt(rtx, oracle, tmp_path, cube)
    base = to_dev(*tabs)
    targets = [torch.zeros((M.CUBE_H, M.CUBE_W, 4), dtype=torch.uint8, device="cuda") for _ in range(6)]
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    keep = []
    for f in range(6):
        with torch.cuda.stream(side):
            d = base[f % 2].clone()
            ev = torch.cuda.Event()
            ev.record(side)
        keep.append((d, ev))
        rt.camera = M.cube_camera(rtx, oracle, f)[1]
        rt.set_triangle_materials_device(d.data_ptr(), 768, 0, classes, ev.cuda_event)
        rt.draw_device(targets[f].data_ptr(), asynchronous=asynchronous)
    rt.sync()
    assert rt.download("PT_QUEUE", np.uint32)[10] == 0
    got = [t.cpu().numpy().reshape(-1, 4) for t in targets]
    assert_table(rt, tabs[1])
    rt.cleanup()
    for f in range(6):
        assert np.array_equal(got[f], want[f]), f + 1


def test_sets_between_synchronous_draws_recycle_addresses(rtx, oracle, tmp_path, cube):
    """Synchronous draws with a still camera and two tables of the same classes, so that only the
    table's contents tell the frames apart and the launch parameters never change.  Draw 1 under A; B
    then A again and draw 2 (A's frame); B and draw 3; then 2, 3, 4, 5 and 6 alternating sets between
    two draws, each run ending on the table the previous draw did not have: with a pool of 2 to 6
    buffers one of them brings the previous draw's address back with other contents.  Every frame is
    its table's, not what the draw before traced ahead."""
    import torch

    a, b = M.face_table(FACES_A), M.face_table(FACES_B)
    classes = rtx.MAT_CLASS_ALL
    finals = [a, a, b, a, b, a, b, a]
    nsets = [1, 2, 1, 2, 3, 4, 5, 6]
    want = serial_cube_frames(rtx, oracle, tmp_path, cube, finals, [0] * len(finals))
    assert not np.array_equal(want[2], want[3])
    rt = cube_rt(rtx, oracle, tmp_path, cube)
    rt.camera = M.cube_camera(rtx, oracle, 0)[1]
    da, db = to_dev(a, b)
    targets = [torch.zeros((M.CUBE_H, M.CUBE_W, 4), dtype=torch.uint8, device="cuda") for _ in finals]
    torch.cuda.synchronize()
    for k, final in enumerate(finals):
        last, other = (da, db) if final is a else (db, da)
        for t in ([other, last] * 3)[-nsets[k]:]:
            rt.set_triangle_materials_device(t.data_ptr(), 768, 0, classes)
        rt.draw_device(targets[k].data_ptr())
    rt.sync()
    assert rt.download("PT_QUEUE", np.uint32)[10] == 0
    got = [t.cpu().numpy().reshape(-1, 4) for t in targets]
    rt.cleanup()
    for k in range(len(finals)):
        assert np.array_equal(got[k], want[k]), k + 1


def test_streaming_sequence_without_a_wait(rtx, oracle, tmp_path):
    """set_mesh_device(patch -> cube), set_triangle_materials_device, build_bvh, draw, one sync at the
    end: the frame of a fresh context that was given the cube and the table through the host calls.  A
    later set_mesh_device leaves the table all 3."""
    import torch

    cv, cidx = welded_cube()
    table = M.face_table(FACES_A)
    _, rcam = M.cube_camera(rtx, oracle)
    ref = patch_rt(rtx, tmp_path, name="r.toml", max_triangles=2048, max_vertices=4096)
    ref.camera = rcam
    ref.set_mesh(cv, cidx)
    ref.set_triangle_materials(table)
    ref.build_bvh()
    want = np.zeros((H, W, 4), np.uint8)
    ref.draw(want)
    assert ref.download("PT_QUEUE", np.uint32)[10] == 0
    ref.cleanup()
    rt = patch_rt(rtx, tmp_path, max_triangles=2048, max_vertices=4096)
    rt.camera = rcam
    dv, di, dt = to_dev(cv, cidx.astype(np.int32), table)
    gv, gi = grid(600)
    dgv, dgi = to_dev(gv, gi.astype(np.int32))
    target = torch.zeros((H, W, 4), dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    rt.set_mesh_device(dv.data_ptr(), len(cv), di.data_ptr(), len(cidx))
    rt.set_triangle_materials_device(dt.data_ptr(), 768, 0, rtx.material_classes(table))
    rt.build_bvh()
    rt.draw_device(target.data_ptr())
    rt.sync()
    assert rt.download("PT_QUEUE", np.uint32)[10] == 0
    assert np.array_equal(target.cpu().numpy(), want)
    assert len(np.unique(want.reshape(-1, 4), axis=0)) > 10  # the cube is in view
    assert_table(rt, table)
    rt.set_mesh_device(dgv.data_ptr(), len(gv), dgi.data_ptr(), len(gi))
    assert_table(rt, np.full(600, 3, np.uint8))
    # ... and a device set on the new, smaller mesh starts from 3 over its triangles
    rt.set_triangle_materials_device(dt.data_ptr(), 10, 590, rtx.MAT_CLASS_ALL)
    want_t = np.full(600, 3, np.uint8)
    want_t[590:] = table[:10]
    assert_table(rt, want_t)
    with pytest.raises(rtx.RtError, match="RT_ERR_ARG"):
        rt.set_triangle_materials_device(dt.data_ptr(), 11, 590, rtx.MAT_CLASS_ALL)  # past the current mesh
    assert_table(rt, want_t)
    rt.cleanup()


def test_no_host_synchronisation(rtx, oracle, tmp_path, cube):
    """A pipelined context on torch streams.  After a warm-up set (the allocation), a set without a
    ready event returns while earlier work on the context stream is still pending; the source tensor
    is overwritten on that stream right after the call; the table is the one the source held at the
    call, and a frame drawn behind it equals the host-set context's."""
    import torch

    a, b = M.face_table(FACES_A), M.face_table(FACES_B)
    want = serial_cube_frames(rtx, oracle, tmp_path, cube, [b], [0])[0]
    rt = cube_rt(rtx, oracle, tmp_path, cube)
    rt.camera = M.cube_camera(rtx, oracle, 0)[1]
    prev = torch.cuda.current_stream(0)
    main, post = torch.cuda.Stream(device=0), torch.cuda.Stream(device=0)
    da, db = to_dev(a, b)
    src = da.clone()
    x = torch.ones((8192, 8192), dtype=torch.float32, device="cuda")
    y = torch.empty_like(x)
    target = torch.zeros((M.CUBE_H, M.CUBE_W, 4), dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    try:
        torch.cuda.set_stream(main)
        rt.set_stream(main.cuda_stream)
        rt.set_post_stream(post.cuda_stream)
        rt.set_triangle_materials_device(src.data_ptr(), 768, 0, rtx.MAT_CLASS_ALL)  # warm-up: table A
        torch.cuda.synchronize()
        for _ in range(12):  # about a tenth of a second of work on the context stream
            torch.mm(x, x, out=y)
        src.copy_(db)  # behind it, the ids the timed call is to read
        busy = torch.cuda.Event()
        busy.record(main)
        rt.set_triangle_materials_device(src.data_ptr(), 768, 0, rtx.MAT_CLASS_ALL)
        pending = not busy.query()
        src.fill_(9)  # on the context stream, behind the read of the source
        rt.draw_device(target.data_ptr(), asynchronous=True)
        torch.cuda.synchronize()
        rt.sync()
        assert pending, "the set returned only after the context stream's earlier work"
        assert_table(rt, b)
        assert rt.download("PT_QUEUE", np.uint32)[10] == 0
        assert np.array_equal(target.cpu().numpy().reshape(-1, 4), want)
        assert (src.cpu().numpy() == 9).all()
    finally:
        rt.cleanup()
        torch.cuda.set_stream(prev)


def test_undeclared_class_is_stored_as_3_and_reported_once(rtx, oracle, tmp_path, cube):
    """One id 5 among 3s with classes = 0: RT_OK, then the next rt_sync is RT_ERR_DEVICE once with the
    count 1, the table has 3 in that place and the frame is the all-3 frame.  The same for a
    carried-over id 4 when a later partial set declares GLOSSY only."""
    w, h = M.CUBE_W, M.CUBE_H
    rt = cube_rt(rtx, oracle, tmp_path, cube)
    rt.camera = M.cube_camera(rtx, oracle)[1]
    rt.build_bvh()
    fresh = trace(rt, 1, w, h)
    ids = np.full(768, 3, np.uint8)
    ids[4 * M.CUBE_FACE_TRIS + 17] = 5  # on z-, in view
    dev_set(rtx, rt, ids, classes=0)  # RT_OK
    with pytest.raises(rtx.RtError, match=r"rt_sync: RT_ERR_DEVICE .* 1 id"):
        rt.sync()
    rt.sync()  # reported once
    assert_table(rt, np.full(768, 3, np.uint8))
    g = trace(rt, 1, w, h)
    assert rt.info().lastChain == 1
    assert_gbuffers_equal(g, fresh)
    ids[:] = 3
    ids[700] = 4
    dev_set(rtx, rt, ids)  # declared MICROFACET by rt_material_classes: nothing to report
    rt.sync()
    assert_table(rt, ids)
    part = np.full(9, 5, np.uint8)
    dev_set(rtx, rt, part, first=100, classes=rtx.MAT_CLASS_GLOSSY)
    with pytest.raises(rtx.RtError, match=r"rt_sync: RT_ERR_DEVICE .* 1 id"):
        rt.sync()
    rt.sync()
    want = np.full(768, 3, np.uint8)
    want[100:109] = 5
    assert_table(rt, want)
    # several at once, new and carried over, across waves and workgroups
    ids = np.full(768, 4, np.uint8)
    ids[::5] = 12
    dev_set(rtx, rt, ids, classes=rtx.MAT_CLASS_ALL)
    dev_set(rtx, rt, np.full(100, 1, np.uint8), first=300, classes=rtx.MAT_CLASS_MICROFACET)
    merged = ids.copy()
    merged[300:400] = 1
    bad = int((merged != 4).sum())
    with pytest.raises(rtx.RtError, match=r"rt_sync: RT_ERR_DEVICE .* %d id" % bad):
        rt.sync()
    assert_table(rt, np.where(merged == 4, 4, 3).astype(np.uint8))
    rt.cleanup()


def test_interplay_with_the_host_setters(rtx, oracle, tmp_path, default_scene, sky_tex):
    """Device set then partial host sets: the merge, an exact census, and the plan follows it once the
    host sets have overwritten every mirror; host set then a partial device set starts from the host
    table; reset then a device set starts from 3; materialOverride wins."""
    s, tex = sky_tex
    rt, ocam = terrain_rt(rtx, oracle, tmp_path, "i")
    n = rt.info().triCount
    half = n // 2 + 3
    mix = M.hashed_ids(n, MIX8)
    dev_set(rtx, rt, mix, classes=rtx.MAT_CLASS_ALL)
    want = mix.copy()
    want[:half] = 7
    rt.set_triangle_materials(want[:half])
    assert_table(rt, want)
    trace(rt, 1)
    assert rt.info().lastChain == 0  # the upper half still holds mirrors
    want[half:] = M.hashed_ids(n - half, (3, 9))
    rt.set_triangle_materials(want[half:], first=half)
    assert_table(rt, want)
    g = trace(rt, 1)
    assert rt.info().lastChain == 1  # the census is exact again: no glossy id left
    o = oracle.pathtrace(default_scene["bvh"], W, H, frame_num=1, cam=ocam, sky_out=s, tex=tex, material_override=3)
    tri = M.primary_triangles(oracle, default_scene["bvh"], W, H, ocam)
    mask = np.where(tri >= 0, want.astype(np.int64)[np.maximum(tri, 0)], M.SKY_MASK).astype(np.uint16)
    assert_gbuffers_equal(g, with_mask(o, mask))
    # host set, then a partial device set starts from the host table
    part = np.full(1000, 5, np.uint8)
    dev_set(rtx, rt, part, first=77, classes=rtx.MAT_CLASS_GLOSSY)
    want[77:1077] = 5
    assert_table(rt, want)
    trace(rt, 1)
    assert rt.info().lastChain == 0
    # reset, then a device set starts from 3
    rt.reset_triangle_materials()
    assert_table(rt, np.full(n, 3, np.uint8))
    dev_set(rtx, rt, part, first=n - 1000, classes=rtx.MAT_CLASS_GLOSSY)
    want = np.full(n, 3, np.uint8)
    want[n - 1000:] = 5
    assert_table(rt, want)
    rt.cleanup()
    # the override wins over a device-set table
    rt, ocam = terrain_rt(rtx, oracle, tmp_path, "ov", extra="materialOverride = 3\n")
    dev_set(rtx, rt, mix, classes=rtx.MAT_CLASS_ALL)
    g = trace(rt, 1)
    assert rt.info().lastChain == 1
    assert_table(rt, mix)
    rt.cleanup()
    assert_gbuffers_equal(g, o)
