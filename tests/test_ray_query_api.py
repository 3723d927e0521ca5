"""Device ray queries at the C-ABI boundary, without a GPU: the argument and state checks of
rt_trace_rays_device (include/rtx_amd.h) on a context that was created but not inited, and the
input checks of rtx.query.trace, which refuses bad tensors before touching the library.

Check order of rt_trace_rays_device: NULL ctx / q, then every other argument check, then the init
state; so each bad argument below is an argument error although the context is not inited, and a
well-formed query on it is a state error."""
import ctypes as C

import numpy as np
import pytest

RT_OK, RT_ERR_ARG, RT_ERR_STATE = 0, -1, -4


@pytest.fixture()
def rt(rtx):
    r = rtx.RayTracer(64, 64, None)  # created, not inited: no device needed
    yield r
    r.cleanup()


@pytest.fixture()
def bufs():
    """Host memory standing in for device pointers: the checks never dereference them."""
    raw = np.zeros(64 * 4 + 8, np.float32)
    off = (-raw.ctypes.data % 16) // 4
    hits = raw[off:off + 64 * 4]
    assert hits.ctypes.data % 16 == 0
    return dict(org=np.zeros((64, 3), np.float32), dir=np.ones((64, 3), np.float32), hits=hits,
                iters=np.zeros(64, np.uint32), keep=raw)


def query(rtx, b, **kw):
    f = dict(org=b["org"].ctypes.data, org_stride=3, dir=b["dir"].ctypes.data, dir_stride=3, n=64,
             hits=b["hits"].ctypes.data, iters=b["iters"].ctypes.data, flags=0, ready_event=None, done_event=None)
    f.update(kw)
    return rtx.RayQuery(**f)


def call(rt, q):
    return rt.lib.rt_trace_rays_device(rt.h, C.byref(q))


def test_query_before_init_is_a_state_error(rt, rtx, bufs):
    assert call(rt, query(rtx, bufs)) == RT_ERR_STATE
    assert b"before rt_init" in rt.lib.rt_last_error(rt.h)
    assert call(rt, query(rtx, bufs, flags=rtx.QUERY_ANY_HIT, iters=None)) == RT_ERR_STATE
    # n == 0 enqueues nothing, but the state check still comes first
    assert call(rt, query(rtx, bufs, n=0, org=None, dir=None, hits=None, iters=None)) == RT_ERR_STATE
    assert call(rt, query(rtx, bufs, n=rtx.QUERY_MAX_RAYS)) == RT_ERR_STATE  # the largest n is an allowed one


def test_null_context_and_null_query_come_first(rt, rtx, bufs):
    L = rt.lib
    assert L.rt_trace_rays_device(None, C.byref(query(rtx, bufs))) == RT_ERR_ARG
    assert L.rt_trace_rays_device(rt.h, None) == RT_ERR_ARG
    assert L.rt_trace_rays_device(None, None) == RT_ERR_ARG


@pytest.mark.parametrize("bad", [
    dict(org=None), dict(dir=None), dict(hits=None),
    dict(org_stride=2), dict(dir_stride=2), dict(org_stride=0), dict(dir_stride=0),
    dict(n=(1 << 30) + 1), dict(n=0xFFFFFFFF),
    dict(flags=2), dict(flags=3), dict(flags=0x80000000),
    dict(hits=+4), dict(hits=+8),
    dict(org=+2), dict(dir=+1), dict(iters=+2),
], ids=["null_org", "null_dir", "null_hits", "org_stride_2", "dir_stride_2", "org_stride_0", "dir_stride_0",
        "n_over_max", "n_u32_max", "flag_2", "flag_3", "flag_top", "hits_plus_4", "hits_plus_8",
        "org_plus_2", "dir_plus_1", "iters_plus_2"])
def test_bad_arguments_are_argument_errors(rt, rtx, bufs, bad):
    kw = {}
    for k, v in bad.items():  # +k: the valid pointer moved by k bytes (misaligned)
        kw[k] = bufs[k].ctypes.data + v if k in ("org", "dir", "hits", "iters") and v is not None else v
    assert call(rt, query(rtx, bufs, **kw)) == RT_ERR_ARG
    if "n" not in bad or bad["n"] <= (1 << 30):
        assert b"rt_trace_rays_device" in rt.lib.rt_last_error(rt.h)


def test_wrapper_packs_the_query(rt, rtx, bufs):
    """RayTracer.trace_rays_device reaches the library with the arguments it was given: a state error
    on this context, raised as RtError; values that do not fit the 32-bit fields are refused."""
    b = bufs
    with pytest.raises(rtx.RtError, match="before rt_init"):
        rt.trace_rays_device(b["org"].ctypes.data, b["dir"].ctypes.data, 64, b["hits"].ctypes.data)
    with pytest.raises(rtx.RtError, match="RT_ERR_ARG"):
        rt.trace_rays_device(b["org"].ctypes.data, b["dir"].ctypes.data, 64, b["hits"].ctypes.data, org_stride=2)
    with pytest.raises(rtx.RtError, match="RT_ERR_ARG"):
        rt.trace_rays_device(b["org"].ctypes.data, b["dir"].ctypes.data, 64, b["hits"].ctypes.data + 4)
    with pytest.raises(ValueError):
        rt.trace_rays_device(b["org"].ctypes.data, b["dir"].ctypes.data, 1 << 32, b["hits"].ctypes.data)
    with pytest.raises(ValueError):
        rt.trace_rays_device(b["org"].ctypes.data, b["dir"].ctypes.data, 64, b["hits"].ctypes.data, dir_stride=-1)


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
    # name: (origins, directions, what the refusal names).  The device check comes last, so on these CPU
    # tensors every other fault is named for what it is, and a well-formed CPU pair is the device mismatch.
    "float64": lambda t: (t.zeros((4, 3), dtype=t.float64), t.zeros((4, 3)), "float32"),
    "int32_dirs": lambda t: (t.zeros((4, 3)), t.zeros((4, 3), dtype=t.int32), "float32"),
    "cpu_device": lambda t: (t.zeros((4, 3)), t.zeros((4, 3)), "device"),
    "cpu_device_8": lambda t: (t.zeros((4, 8))[:, 0:3], t.zeros((4, 8))[:, 4:7], "device"),
    "rank_1": lambda t: (t.zeros(12), t.zeros((4, 3)), "shape"),
    "rank_3": lambda t: (t.zeros((4, 3, 1)), t.zeros((4, 3)), "shape"),
    "two_columns": lambda t: (t.zeros((4, 2)), t.zeros((4, 3)), "shape"),
    "nine_columns": lambda t: (t.zeros((4, 3)), t.zeros((4, 9)), "shape"),
    "inner_stride": lambda t: (t.zeros((4, 6))[:, ::2], t.zeros((4, 3)), "inner stride"),
    "transposed": lambda t: (t.zeros((3, 4)).T, t.zeros((4, 3)), "inner stride"),
    "broadcast_rows": lambda t: (t.zeros((1, 3)).expand(4, 3), t.zeros((4, 3)), "row stride"),
    "count_mismatch": lambda t: (t.zeros((4, 3)), t.zeros((5, 3)), "same number"),
    "numpy": lambda t: (np.zeros((4, 3), np.float32), t.zeros((4, 3)), "torch tensor"),
}


@pytest.mark.parametrize("case", sorted(BAD_TENSORS))
def test_query_trace_refuses_bad_tensors_before_the_library(rt, case):
    torch = _torch()
    from rtx import query

    o, d, what = BAD_TENSORS[case](torch)
    lib = rt.lib
    rt.lib = _NoLibrary()
    try:
        with pytest.raises(ValueError, match=what):
            query.trace(rt, o, d)
        if what == "device":  # a bad `out` is refused as well, ahead of the device check
            with pytest.raises(ValueError, match="out must be"):
                query.trace(rt, o, d, out=torch.zeros((4, 3)))
    finally:
        rt.lib = lib


def test_split_helpers():
    torch = _torch()
    from rtx import query

    hits = torch.tensor([[1.5, 0.0, 0.25, 0.5], [1e11, 0.0, 0.0, 0.0]], dtype=torch.float32)
    hits.view(torch.int32)[:, 1] = torch.tensor([7, -1], dtype=torch.int32)
    t, tri, u, v = query.split(hits)
    assert tri.dtype == torch.int32 and tri.tolist() == [7, -1]
    assert t.tolist() == [1.5, float(np.float32(1e11))]
    assert u.tolist() == [0.25, 0.0] and v.tolist() == [0.5, 0.0]
    assert query.tri_of(hits).data_ptr() == hits.data_ptr() + 4  # views, not copies
