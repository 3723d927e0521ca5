"""Animated geometry at the C-ABI boundary, without a GPU: argument and state checks of
rt_update_vertices / rt_update_vertices_device / rt_get_geometry_epoch (include/rtx_amd.h) and the
input checks of their Python wrappers, which refuse bad arrays before touching the library."""
import ctypes as C

import numpy as np
import pytest

RT_ERR_ARG, RT_ERR_STATE = -1, -4


@pytest.fixture()
def rt(rtx):
    r = rtx.RayTracer(64, 64, None)  # created, not inited: no device needed
    yield r
    r.cleanup()


def test_update_before_init_is_a_state_error(rt):
    xyz = np.zeros((4, 3), np.float32)
    assert rt.lib.rt_update_vertices(rt.h, xyz.ctypes.data, 0, 4) == RT_ERR_STATE
    assert rt.lib.rt_update_vertices_device(rt.h, xyz.ctypes.data, 0, 4, None) == RT_ERR_STATE
    assert b"before rt_init" in rt.lib.rt_last_error(rt.h)


def test_null_arguments_are_argument_errors(rt):
    xyz = np.zeros((4, 3), np.float32)
    L = rt.lib
    assert L.rt_update_vertices(None, xyz.ctypes.data, 0, 4) == RT_ERR_ARG
    assert L.rt_update_vertices(rt.h, None, 0, 4) == RT_ERR_ARG
    assert L.rt_update_vertices_device(None, xyz.ctypes.data, 0, 4, None) == RT_ERR_ARG
    assert L.rt_update_vertices_device(rt.h, None, 0, 4, None) == RT_ERR_ARG
    e = C.c_uint64(7)
    assert L.rt_get_geometry_epoch(None, C.byref(e)) == RT_ERR_ARG
    assert L.rt_get_geometry_epoch(rt.h, None) == RT_ERR_ARG
    assert e.value == 7


def test_fresh_context_is_at_epoch_zero(rt):
    e = C.c_uint64(7)
    assert rt.lib.rt_get_geometry_epoch(rt.h, C.byref(e)) == 0 and e.value == 0
    assert rt.geometry_epoch == 0


class _NoLibrary:
    """Stands in for librtx: any call through it fails the test."""

    def __getattr__(self, name):
        raise AssertionError("the wrapper called %s for an array it must refuse" % name)


@pytest.mark.parametrize("bad", [
    np.zeros((4, 3), np.float64),
    np.zeros((4, 2), np.float32),
    np.zeros((4, 3, 1), np.float32),
    np.zeros(12, np.float32),
    np.zeros((4, 6), np.float32)[:, ::2],          # (4, 3) view, not contiguous
    np.zeros((3, 4), np.float32).T,                # (4, 3) Fortran order
    [[0.0, 0.0, 0.0]],
], ids=["float64", "n_by_2", "3d", "flat", "strided", "fortran", "list"])
def test_wrapper_refuses_bad_arrays_before_the_library(rt, bad):
    lib = rt.lib
    rt.lib = _NoLibrary()
    try:
        with pytest.raises(ValueError):
            rt.update_vertices(bad)
    finally:
        rt.lib = lib
    assert rt.geometry_epoch == 0
