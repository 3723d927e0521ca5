"""Surface queries at the C-ABI boundary, without a GPU: the header's structs and constants against the
Python mirror, the argument and state checks of rt_trace_surfaces_device (include/rtx_amd.h) in their
documented order on a context that was created but not inited, the input checks of
rtx.query.trace(surface=True) and rtx.query.surfaces, the views, and the premise of the surface pass on
the CPU oracle.

Check order of rt_trace_surfaces_device: NULL ctx / q; every argument check of rt_trace_rays_device on
q->rays; unknown bits in flags; with n > 0 a NULL or misaligned surface; the two RT_SURFACE_FROM_HITS
rules; then the init state."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from surface_scenes import ray_set

RT_OK, RT_ERR_ARG, RT_ERR_STATE = 0, -1, -4
HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "rtx_amd.h")


@pytest.fixture()
def rt(rtx):
    r = rtx.RayTracer(64, 64, None)  # created, not inited: no device needed
    yield r
    r.cleanup()


@pytest.fixture()
def bufs():
    """Host memory standing in for device pointers: the checks never dereference them."""
    def aligned(floats):
        raw = np.zeros(floats + 8, np.float32)
        off = (-raw.ctypes.data % 16) // 4
        a = raw[off:off + floats]
        assert a.ctypes.data % 16 == 0
        return a, raw

    hits, k0 = aligned(64 * 4)
    surface, k1 = aligned(64 * 16)
    return dict(org=np.zeros((64, 3), np.float32), dir=np.ones((64, 3), np.float32), hits=hits, surface=surface,
                iters=np.zeros(64, np.uint32), keep=(k0, k1))


def query(rtx, b, flags=0, surface=0, ray_flags=0, **kw):
    """flags: the surface query's; surface: the valid pointer moved by that many bytes, or None."""
    f = dict(org=b["org"].ctypes.data, org_stride=3, dir=b["dir"].ctypes.data, dir_stride=3, n=64,
             hits=b["hits"].ctypes.data, iters=None, flags=ray_flags, ready_event=None, done_event=None)
    f.update(kw)
    s = b["surface"].ctypes.data + surface if surface is not None else None
    return rtx.SurfaceQuery(rtx.RayQuery(**f), s, flags)


def call(rt, q):
    return rt.lib.rt_trace_surfaces_device(rt.h, C.byref(q))


def test_header_matches_the_mirror(rtx):
    text = open(HEADER).read()
    for name, value in (("RT_SURFACE_FROM_HITS", rtx.SURFACE_FROM_HITS), ("RT_SURFACE_MOTION", rtx.SURFACE_MOTION)):
        m = re.search(r"#define %s\s+(\d+)u" % name, text)
        assert m and int(m.group(1)) == value, name
    assert "#define RT_SURFACE_FLOATS(flags) (((flags) & RT_SURFACE_MOTION) ? 16u : 12u)" in text
    assert [rtx.surface_floats(f) for f in (0, 1, 2, 3)] == [12, 12, 16, 16]
    m = re.search(r"typedef struct rt_surface_query \{(.*?)\} rt_surface_query;", text, re.S)
    fields = re.findall(r"^\s*([A-Za-z_0-9]+\*?)\s+(\w+);", m.group(1), re.M)
    assert fields == [("rt_ray_query", "rays"), ("float*", "surface"), ("uint32_t", "flags")]
    assert [n for n, _ in rtx.SurfaceQuery._fields_] == ["rays", "surface", "flags"]
    assert rtx.SurfaceQuery._fields_[0][1] is rtx.RayQuery
    # the C layout on LP64: the 72-byte ray query, the pointer, the flags and the tail padding
    assert C.sizeof(rtx.RayQuery) == 72 and C.sizeof(rtx.SurfaceQuery) == 88
    assert rtx.SurfaceQuery.surface.offset == 72 and rtx.SurfaceQuery.flags.offset == 80
    assert "int rt_trace_surfaces_device(rt_context* ctx, const rt_surface_query* q);" in text
    assert "rt_trace_surfaces_device" in rtx.SIGNATURES


def test_refusals_in_the_documented_order(rt, rtx, bufs):
    L, b = rt.lib, bufs
    # 1. NULL ctx / q
    assert L.rt_trace_surfaces_device(None, C.byref(query(rtx, b))) == RT_ERR_ARG
    assert L.rt_trace_surfaces_device(rt.h, None) == RT_ERR_ARG
    # 2. the ray query's own checks, with its messages, ahead of the surface query's
    for kw, msg in ((dict(org_stride=2), b"strides"), (dict(n=(1 << 30) + 1), b"RT_QUERY_MAX_RAYS"),
                    (dict(ray_flags=2), b"unknown flags"), (dict(org=None), b"must not be NULL"),
                    (dict(hits=b["hits"].ctypes.data + 4), b"hits must be 16-byte aligned"),
                    (dict(dir=b["dir"].ctypes.data + 2), b"4-byte aligned")):
        assert call(rt, query(rtx, b, flags=8, surface=None, **kw)) == RT_ERR_ARG, kw
        err = L.rt_last_error(rt.h)
        assert msg in err and b"rt_trace_surfaces_device" in err, (kw, err)
    # 3. unknown bits in flags, ahead of the surface pointer
    for flags in (4, 8, 0x80000000, 7):
        assert call(rt, query(rtx, b, flags=flags, surface=None)) == RT_ERR_ARG
        assert b"unknown surface flags" in L.rt_last_error(rt.h)
    # 4. with n > 0 a NULL or misaligned surface, ahead of the FROM_HITS rules
    for surface, msg in ((None, b"surface must not be NULL"), (4, b"surface must be 16-byte aligned"), (8, b"16-byte")):
        q = query(rtx, b, flags=rtx.SURFACE_FROM_HITS, surface=surface, iters=b["iters"].ctypes.data)
        assert call(rt, q) == RT_ERR_ARG
        assert msg in L.rt_last_error(rt.h)
    # 5. RT_SURFACE_FROM_HITS traces nothing: no iters, no any-hit
    for flags in (rtx.SURFACE_FROM_HITS, rtx.SURFACE_FROM_HITS | rtx.SURFACE_MOTION):
        assert call(rt, query(rtx, b, flags=flags, iters=b["iters"].ctypes.data)) == RT_ERR_ARG
        assert b"iters must be NULL" in L.rt_last_error(rt.h)
    q = query(rtx, b, flags=rtx.SURFACE_FROM_HITS)
    q.rays.flags = rtx.QUERY_ANY_HIT
    assert call(rt, q) == RT_ERR_ARG
    assert b"RT_QUERY_ANY_HIT must be clear" in L.rt_last_error(rt.h)
    # 6. every well-formed query is a state error on this context
    for flags in (0, rtx.SURFACE_MOTION, rtx.SURFACE_FROM_HITS, rtx.SURFACE_FROM_HITS | rtx.SURFACE_MOTION):
        assert call(rt, query(rtx, b, flags=flags)) == RT_ERR_STATE
        assert b"rt_trace_surfaces_device before rt_init" in L.rt_last_error(rt.h)
    q = query(rtx, b, iters=b["iters"].ctypes.data)
    q.rays.flags = rtx.QUERY_ANY_HIT
    assert call(rt, q) == RT_ERR_STATE
    # n == 0 needs no buffers, but the state check still comes
    assert call(rt, query(rtx, b, n=0, org=None, dir=None, hits=None, surface=None)) == RT_ERR_STATE


def test_wrapper_packs_the_query(rt, rtx, bufs):
    b = bufs
    args = (b["org"].ctypes.data, b["dir"].ctypes.data, 64, b["hits"].ctypes.data, b["surface"].ctypes.data)
    with pytest.raises(rtx.RtError, match="before rt_init"):
        rt.trace_surfaces_device(*args)
    with pytest.raises(rtx.RtError, match="before rt_init"):
        rt.trace_surfaces_device(*args, from_hits=True, motion=True)
    with pytest.raises(rtx.RtError, match="RT_QUERY_ANY_HIT must be clear"):
        rt.trace_surfaces_device(*args, from_hits=True, any_hit=True)
    with pytest.raises(rtx.RtError, match="iters must be NULL"):
        rt.trace_surfaces_device(*args, from_hits=True, iters_ptr=b["iters"].ctypes.data)
    with pytest.raises(rtx.RtError, match="surface must be 16-byte aligned"):
        rt.trace_surfaces_device(*args[:4], b["surface"].ctypes.data + 4)
    with pytest.raises(ValueError):
        rt.trace_surfaces_device(args[0], args[1], 1 << 32, args[3], args[4])


class _NoLibrary:
    """Stands in for librtx: any call through it fails the test."""

    def __getattr__(self, name):
        raise AssertionError("the wrapper called %s for tensors it must refuse" % name)


def _torch():
    try:
        import torch

        torch.zeros((2, 3), dtype=torch.float32)
        return torch
    except Exception as e:  # no torch, or one that cannot make CPU tensors
        pytest.skip("torch CPU tensors unavailable: %s" % e)


BAD_TENSORS = {
    # name: (origins, directions, what the refusal names); the device check comes last
    "float64": lambda t: (t.zeros((4, 3), dtype=t.float64), t.zeros((4, 3)), "float32"),
    "int32_dirs": lambda t: (t.zeros((4, 3)), t.zeros((4, 3), dtype=t.int32), "float32"),
    "cpu_device": lambda t: (t.zeros((4, 3)), t.zeros((4, 3)), "device"),
    "cpu_device_8": lambda t: (t.zeros((4, 8))[:, 0:3], t.zeros((4, 8))[:, 4:7], "device"),
    "rank_1": lambda t: (t.zeros(12), t.zeros((4, 3)), "shape"),
    "two_columns": lambda t: (t.zeros((4, 2)), t.zeros((4, 3)), "shape"),
    "nine_columns": lambda t: (t.zeros((4, 3)), t.zeros((4, 9)), "shape"),
    "inner_stride": lambda t: (t.zeros((4, 6))[:, ::2], t.zeros((4, 3)), "inner stride"),
    "broadcast_rows": lambda t: (t.zeros((1, 3)).expand(4, 3), t.zeros((4, 3)), "row stride"),
    "count_mismatch": lambda t: (t.zeros((4, 3)), t.zeros((5, 3)), "same number"),
    "numpy": lambda t: (np.zeros((4, 3), np.float32), t.zeros((4, 3)), "torch tensor"),
}


@pytest.mark.parametrize("case", sorted(BAD_TENSORS))
def test_surface_forms_refuse_bad_tensors_before_the_library(rt, case):
    torch = _torch()
    from rtx import query

    o, d, what = BAD_TENSORS[case](torch)
    lib = rt.lib
    rt.lib = _NoLibrary()
    try:
        for motion in (False, True):
            with pytest.raises(ValueError, match=what):
                query.trace(rt, o, d, surface=True, motion=motion)
            with pytest.raises(ValueError, match=what):
                query.surfaces(rt, o, d, torch.zeros((4, 4)), motion=motion)
        if what == "device":  # wrong result and record tensors are refused as well, ahead of the device check
            with pytest.raises(ValueError, match="^out must be"):
                query.trace(rt, o, d, surface=True, out=torch.zeros((4, 3)))
            for motion, cols in ((False, 16), (True, 12), (False, 4)):
                with pytest.raises(ValueError, match="surface_out must be a contiguous \\(n, %d\\)" % (16 if motion else 12)):
                    query.trace(rt, o, d, surface=True, motion=motion, surface_out=torch.zeros((4, cols)))
                with pytest.raises(ValueError, match="^out must be a contiguous \\(n, %d\\)" % (16 if motion else 12)):
                    query.surfaces(rt, o, d, torch.zeros((4, 4)), motion=motion, out=torch.zeros((4, cols)))
            with pytest.raises(ValueError, match="surface_out must be"):
                query.trace(rt, o, d, surface=True, surface_out=torch.zeros((4, 12), dtype=torch.float64))
            with pytest.raises(ValueError, match="surface_out must be"):
                query.trace(rt, o, d, surface=True, surface_out=torch.zeros((12, 4)).T)
            for hits in (torch.zeros((4, 3)), torch.zeros((5, 4)), torch.zeros((4, 4), dtype=torch.int32),
                         torch.zeros((4, 8))[:, :4], np.zeros((4, 4), np.float32), None):
                with pytest.raises(ValueError, match="hits must be"):
                    query.surfaces(rt, o, d, hits)
            with pytest.raises(ValueError, match="belong to surface=True"):
                query.trace(rt, o, d, motion=True)
            with pytest.raises(ValueError, match="belong to surface=True"):
                query.trace(rt, o, d, surface_out=torch.zeros((4, 12)))
    finally:
        rt.lib = lib


def test_views_and_spawn_origins():
    torch = _torch()
    from rtx import query

    s = torch.arange(32, dtype=torch.float32).reshape(2, 16)
    s.view(torch.int32)[:, 11] = torch.tensor([7 | 1 << 16 | 1 << 17, 0x12345 & 0xFFFF | 1 << 17], dtype=torch.int32)
    assert query.position(s).tolist() == [[0, 1, 2], [16, 17, 18]] and query.offset(s).tolist() == [3, 19]
    assert query.normal(s).tolist() == [[4, 5, 6], [20, 21, 22]] and query.normal_dot_dir(s).tolist() == [7, 23]
    assert query.shading_normal(s).tolist() == [[8, 9, 10], [24, 25, 26]]
    assert query.displacement(s).tolist() == [[12, 13, 14], [28, 29, 30]]
    assert query.material(s).dtype == torch.int32 and query.material(s).tolist() == [7, 0x2345]
    assert query.front_face(s).dtype == torch.bool and query.front_face(s).tolist() == [True, False]
    assert query.is_hit(s).tolist() == [True, True]
    assert query.position(s).data_ptr() == s.data_ptr() and query.normal(s).data_ptr() == s.data_ptr() + 16  # views
    s12 = s[:, :12].contiguous()
    assert query.material(s12).tolist() == [7, 0x2345]
    with pytest.raises(ValueError):
        query.displacement(s12)
    z = torch.zeros((2, 12))
    z[:, 0:3] = torch.tensor([[1.0, 2.0, 3.0], [1.0, 2.0, 3.0]])
    z[:, 3] = 0.5
    z[:, 4:7] = torch.tensor([[0.0, 1.0, 0.0], [0.0, 1.0, 0.0]])
    d = torch.tensor([[0.0, 1.0, 0.0, 9.0], [1.0, -1.0, 0.0, 9.0]])  # away from the surface, and through it
    assert query.spawn_origins(z, d).tolist() == [[1.0, 2.5, 3.0], [1.0, 1.5, 3.0]]


def test_offset_is_a_function_of_t_and_the_position(oracle, default_scene):
    """The premise of the dense pass, on the CPU oracle alone (it needs no surface query): the one input of
    the hit finalisation that a hit record lacks, errorT, is gamma(16) |t|, so the oracle's offset equals
    fl(fl(gamma(16) |t|) + fl(max|pos| gamma(6))) for every hit of the ray set, bit for bit."""
    r = ray_set(oracle, default_scene)
    o, hit = r["o"], r["hit"]
    eps = np.float32(2.0 ** -23)  # kMachineEps

    def gamma(n):
        ne = np.float32(n) * eps
        return ne / (np.float32(1.0) - ne)

    assert gamma(16).dtype == np.float32
    err_t = gamma(16) * np.abs(o["t"][hit])
    err_p = np.abs(o["pos"][hit]).max(1) * gamma(6)
    want = err_t + err_p
    assert want.dtype == np.float32 and hit.sum() > 2000
    assert np.array_equal(want.view(np.uint32), o["offset"][hit].view(np.uint32))
