"""Mesh replacement at the C-ABI boundary, without a GPU: rt_mesh_adjacency (the host definition of
the adjacency the device kernels of rt_set_mesh reproduce) against numpy, the argument and state
checks of rt_set_mesh / rt_set_mesh_device on a context that was created but not inited, and the
[scene] maxTriangles / maxVertices checks of rt_create and rt_init.

Check order of the setters: NULL ctx / mesh, then the argument checks that need no context state,
then the init state; the capacity and (host variant) the index range need an inited context."""
import ctypes as C

import numpy as np
import pytest

from mesh_scenes import SHAPES, numpy_adjacency, pad_indices

RT_OK, RT_ERR_ARG, RT_ERR_IO, RT_ERR_STATE, RT_ERR_NO_DEVICE = 0, -1, -3, -4, -5


@pytest.mark.parametrize("shape", sorted(SHAPES))
def test_mesh_adjacency_is_the_stable_sort(rtx, shape):
    v, idx = SHAPES[shape]()
    nv = len(v)
    ip = pad_indices(idx)
    off, corners, slots = rtx.mesh_adjacency(ip, nv)
    woff, wcorners, wslots = numpy_adjacency(ip, nv)
    assert np.array_equal(off, woff)
    assert np.array_equal(corners, wcorners)
    assert np.array_equal(slots, wslots)
    assert off[0] == 0 and off[nv] == ip.size
    if shape == "soup2":  # the padding corners 6..11 end vertex 0's run, behind corner 0
        assert corners[:7].tolist() == [0, 6, 7, 8, 9, 10, 11] and slots[6:].tolist() == [1, 2, 3, 4, 5, 6]
    if shape == "fan5000":
        assert off[1] == 5000
    if shape == "gaps":  # empty runs first, in the middle and last
        assert off[5] == 0 and off[nv - 7] == ip.size and (np.diff(off.astype(np.int64)) == 0).sum() >= 312


def test_mesh_adjacency_optional_outputs_and_errors(rtx):
    L = rtx.load_library()
    idx = np.asarray([0, 1, 2, 2, 1, 3], np.uint32)
    off = np.zeros(5, np.uint32)
    slots = np.zeros(6, np.uint32)
    assert L.rt_mesh_adjacency(idx.ctypes.data, 2, 4, off.ctypes.data, None, slots.ctypes.data) == RT_OK
    assert off.tolist() == [0, 1, 3, 5, 6] and slots.tolist() == [0, 1, 3, 4, 2, 5]
    assert L.rt_mesh_adjacency(idx.ctypes.data, 2, 4, off.ctypes.data, None, None) == RT_OK
    assert L.rt_mesh_adjacency(None, 2, 4, off.ctypes.data, None, None) == RT_ERR_ARG
    assert L.rt_mesh_adjacency(idx.ctypes.data, 2, 4, None, None, None) == RT_ERR_ARG
    assert L.rt_mesh_adjacency(idx.ctypes.data, 2, 0, off.ctypes.data, None, None) == RT_ERR_ARG
    assert L.rt_mesh_adjacency(idx.ctypes.data, 2, 3, off.ctypes.data, None, None) == RT_ERR_ARG  # index 3 >= 3
    with pytest.raises(rtx.RtError, match="RT_ERR_ARG"):
        rtx.mesh_adjacency(idx.reshape(2, 3), 3)


@pytest.fixture()
def rt(rtx):
    r = rtx.RayTracer(64, 64, None)  # created, not inited: no device needed
    yield r
    r.cleanup()


@pytest.fixture()
def arrays():
    """Host memory standing in for both variants' pointers: the checks before the init state never read it."""
    return dict(xyz=np.zeros((8, 3), np.float32), indices=np.zeros((4, 3), np.uint32))


def mesh(rtx, a, **kw):
    f = dict(xyz=a["xyz"].ctypes.data, vertex_count=8, indices=a["indices"].ctypes.data, triangle_count=4,
             ready_event=None)
    f.update(kw)
    return rtx.Mesh(**f)


@pytest.mark.parametrize("fn", ["rt_set_mesh", "rt_set_mesh_device"])
def test_null_context_and_null_mesh_come_first(rt, rtx, arrays, fn):
    call = getattr(rt.lib, fn)
    assert call(None, C.byref(mesh(rtx, arrays))) == RT_ERR_ARG
    assert call(rt.h, None) == RT_ERR_ARG
    assert call(None, None) == RT_ERR_ARG


@pytest.mark.parametrize("fn", ["rt_set_mesh", "rt_set_mesh_device"])
def test_argument_errors_come_before_the_state_error(rt, rtx, arrays, fn):
    call = getattr(rt.lib, fn)
    assert call(rt.h, C.byref(mesh(rtx, arrays))) == RT_ERR_STATE
    assert b"before rt_init" in rt.lib.rt_last_error(rt.h)
    for bad in (dict(xyz=None), dict(indices=None), dict(xyz=arrays["xyz"].ctypes.data + 2),
                dict(indices=arrays["indices"].ctypes.data + 1), dict(triangle_count=1), dict(triangle_count=0),
                dict(vertex_count=0)):
        assert call(rt.h, C.byref(mesh(rtx, arrays, **bad))) == RT_ERR_ARG, bad
        assert fn.encode() in rt.lib.rt_last_error(rt.h)
    # the capacity is the init mesh's: on this context it is not known yet, and the state error comes first
    assert call(rt.h, C.byref(mesh(rtx, arrays, triangle_count=0xFFFFFFFF, vertex_count=0xFFFFFFFF))) == RT_ERR_STATE


def test_wrappers_pack_the_mesh(rt, rtx, arrays):
    with pytest.raises(rtx.RtError, match="rt_set_mesh: RT_ERR_STATE"):
        rt.set_mesh(arrays["xyz"], arrays["indices"])
    with pytest.raises(rtx.RtError, match="rt_set_mesh_device: RT_ERR_STATE"):
        rt.set_mesh_device(arrays["xyz"].ctypes.data, 8, arrays["indices"].ctypes.data, 4)
    with pytest.raises(rtx.RtError, match="RT_ERR_ARG"):
        rt.set_mesh_device(arrays["xyz"].ctypes.data, 8, arrays["indices"].ctypes.data, 1)
    with pytest.raises(ValueError):
        rt.set_mesh(arrays["xyz"].astype(np.float64), arrays["indices"])
    with pytest.raises(ValueError):
        rt.set_mesh(arrays["xyz"], arrays["indices"].reshape(-1))
    with pytest.raises(ValueError):
        rt.set_mesh(arrays["xyz"][::2], arrays["indices"])
    with pytest.raises(ValueError):
        rt.set_mesh_device(arrays["xyz"].ctypes.data, 1 << 32, arrays["indices"].ctypes.data, 4)
    for name in ("ADJ_OFFSETS", "CORNER_SLOTS"):
        assert name in rtx.ARR
    assert (rtx.ARR["ADJ_OFFSETS"], rtx.ARR["CORNER_SLOTS"]) == (43, 44)


@pytest.mark.parametrize("value", ["-1", '"x"', "x", "1.5", "4294967296"])
@pytest.mark.parametrize("key", ["maxTriangles", "maxVertices"])
def test_unparsable_capacity_is_an_io_error(rtx, tmp_path, key, value):
    cfg = rtx.write_config(str(tmp_path / "c.toml"), 64, 64, **{"max_triangles" if key == "maxTriangles" else "max_vertices": value})
    assert "%s = %s\n" % (key, value) in open(cfg).read()
    with pytest.raises(rtx.RtError, match="rt_create: RT_ERR_IO .*%s" % key):
        rtx.RayTracer(64, 64, cfg)


@pytest.mark.parametrize("kw", [dict(max_triangles=1048577), dict(max_triangles=1023 * 1024 + 1),
                                dict(max_triangles=60799), dict(max_vertices=30800)],
                         ids=["over_the_limit", "too_many_batches", "triangles_below_init", "vertices_below_init"])
def test_bad_capacity_is_an_argument_error_of_init(rtx, tmp_path, kw):
    """Raised before any device call: RT_ERR_ARG, not RT_ERR_NO_DEVICE, on a machine without a GPU too.
    The default scene has 60,800 triangles and 30,801 vertices."""
    r = rtx.RayTracer(64, 64, rtx.write_config(str(tmp_path / "c.toml"), 64, 64, **kw))
    try:
        assert r.lib.rt_init(r.h) == RT_ERR_ARG
        assert b"maxTriangles" in r.lib.rt_last_error(r.h)
    finally:
        r.cleanup()


def test_capacity_within_the_limits_passes_the_scene_checks(rtx, tmp_path):
    """0 and the init mesh's own counts are the default capacity; the largest one is allowed."""
    for kw in (dict(max_triangles=0, max_vertices=0), dict(max_triangles=60800, max_vertices=30801),
               dict(max_triangles=1023 * 1024)):
        r = rtx.RayTracer(64, 64, rtx.write_config(str(tmp_path / "c.toml"), 64, 64, **kw))
        try:
            assert r.lib.rt_init(r.h) in (RT_OK, RT_ERR_NO_DEVICE), kw
        finally:
            r.cleanup()
