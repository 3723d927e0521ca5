"""Geometry motion vectors at the C-ABI boundary, without a GPU: rt_set_geometry_motion /
rt_get_geometry_motion (include/rtx_amd.h) are bound, check their arguments and the context's
state, and the [render] geometryMotion config key sets the initial state (a value that is no
boolean is refused by rt_create with RT_ERR_IO)."""
import ctypes as C
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RT_OK, RT_ERR_ARG, RT_ERR_IO, RT_ERR_STATE = 0, -1, -3, -4


@pytest.fixture()
def rt(rtx):
    r = rtx.RayTracer(64, 64, None)  # created, not inited: no device needed
    yield r
    r.cleanup()


def test_header_entries_are_bound(rtx):
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "rtx_amd.h")).read(), flags=re.S)
    for name in ("rt_set_geometry_motion", "rt_get_geometry_motion"):
        assert re.search(r"\bint\s+%s\s*\(" % name, text), name
        assert name in rtx.SIGNATURES and hasattr(rtx.load_library(), name), name
    assert isinstance(rtx.RayTracer.geometry_motion, property) and rtx.RayTracer.geometry_motion.fset is not None


def test_info_keeps_its_layout(rtx):
    assert C.sizeof(rtx.Info) == 19 * 4


def test_null_arguments_are_argument_errors(rt):
    L = rt.lib
    on = C.c_int(7)
    assert L.rt_set_geometry_motion(None, 1) == RT_ERR_ARG
    assert L.rt_get_geometry_motion(None, C.byref(on)) == RT_ERR_ARG
    assert L.rt_get_geometry_motion(rt.h, None) == RT_ERR_ARG
    assert on.value == 7


def test_set_before_init_is_a_state_error(rtx, rt):
    assert rt.lib.rt_set_geometry_motion(rt.h, 1) == RT_ERR_STATE
    assert b"before rt_init" in rt.lib.rt_last_error(rt.h)
    assert rt.lib.rt_set_geometry_motion(rt.h, 0) == RT_ERR_STATE
    with pytest.raises(rtx.RtError, match="RT_ERR_STATE"):
        rt.geometry_motion = True
    assert rt.geometry_motion is False  # the getter needs no device: the configured state


def test_off_by_default(rtx, rt, tmp_path):
    on = C.c_int(7)
    assert rt.lib.rt_get_geometry_motion(rt.h, C.byref(on)) == RT_OK and on.value == 0
    r = rtx.RayTracer(64, 64, rtx.write_config(str(tmp_path / "plain.toml"), 64, 64))
    assert r.geometry_motion is False
    r.cleanup()
    assert "geometryMotion" not in open(str(tmp_path / "plain.toml")).read()


@pytest.mark.parametrize("value", [True, False])
def test_config_key_sets_the_initial_state(rtx, tmp_path, value):
    cfg = rtx.write_config(str(tmp_path / "m.toml"), 64, 64, geometry_motion=value)
    assert ("geometryMotion = %s\n" % ("true" if value else "false")) in open(cfg).read()
    r = rtx.RayTracer(64, 64, cfg)
    assert r.geometry_motion is value
    r.cleanup()


def test_config_key_is_read_from_the_render_table_only(rtx, tmp_path):
    cfg = rtx.write_config(str(tmp_path / "t.toml"), 64, 64, tuning={"geometryMotion": True})
    r = rtx.RayTracer(64, 64, cfg)
    assert r.geometry_motion is False
    r.cleanup()


@pytest.mark.parametrize("bad", ["1", "0", '"true"', "yes", "True", '["true"]', "2.5"],
                         ids=["one", "zero", "string", "yes", "capital", "array", "float"])
def test_config_key_refuses_a_non_bool(rtx, tmp_path, bad):
    cfg = rtx.write_config(str(tmp_path / "bad.toml"), 64, 64, extra="geometryMotion = %s\n" % bad)
    h = C.c_void_p()
    assert rtx.load_library().rt_create(64, 64, cfg.encode(), C.byref(h)) == RT_ERR_IO
    assert not h.value
    assert b"geometryMotion" in rtx.load_library().rt_last_error(None)
    with pytest.raises(rtx.RtError, match="RT_ERR_IO"):
        rtx.RayTracer(64, 64, cfg)
