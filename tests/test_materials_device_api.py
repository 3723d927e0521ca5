"""rt_set_triangle_materials_device at the C-ABI boundary, without a GPU: the argument checks come
before the init state (include/rtx_amd.h), the Python table covers the new entries, and the class
rule the device kernel compiles (csrc/mat_kernels.h mat_class_of, exposed as rt_material_class_rule)
is rt_material_classes' over every id."""
import ctypes as C
import os
import re

import numpy as np
import pytest

RT_OK, RT_ERR_ARG, RT_ERR_STATE = 0, -1, -4
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture()
def rt(rtx):
    r = rtx.RayTracer(64, 64, None)  # created, not inited: no device needed
    yield r
    r.cleanup()


def update(rtx, ids=0x1000, first=0, count=4, classes=0, ready=None):
    return rtx.MaterialUpdate(ids, first, count, classes, ready)


def test_argument_checks_come_before_the_init_state(rtx, rt):
    """NULL ctx / u, NULL ids, count 0 and unknown class bits are RT_ERR_ARG on a context that is not
    inited; a well-formed update is RT_ERR_STATE there.  No pointer is followed (0x1000 is not memory)."""
    L = rt.lib
    good = update(rtx, classes=rtx.MAT_CLASS_ALL)
    assert L.rt_set_triangle_materials_device(None, C.byref(good)) == RT_ERR_ARG
    assert L.rt_set_triangle_materials_device(rt.h, None) == RT_ERR_ARG
    for bad, text in ((update(rtx, ids=None), b"ids"), (update(rtx, count=0), b"count"),
                      (update(rtx, classes=4), b"classes"), (update(rtx, classes=0x80000001), b"classes"),
                      (update(rtx, ids=None, count=0, classes=8), b"ids")):  # the first failing check names itself
        assert L.rt_set_triangle_materials_device(rt.h, C.byref(bad)) == RT_ERR_ARG
        err = L.rt_last_error(rt.h)
        assert b"rt_set_triangle_materials_device" in err and text in err, err
    for classes in (0, rtx.MAT_CLASS_GLOSSY, rtx.MAT_CLASS_MICROFACET, rtx.MAT_CLASS_ALL):
        assert L.rt_set_triangle_materials_device(rt.h, C.byref(update(rtx, classes=classes))) == RT_ERR_STATE
        assert b"before rt_init" in L.rt_last_error(rt.h)
    # a range that no mesh could hold is still a state error before rt_init: the range check is the later one
    far = update(rtx, first=0xFFFFFFFF, count=0xFFFFFFFF)
    assert L.rt_set_triangle_materials_device(rt.h, C.byref(far)) == RT_ERR_STATE


def test_structure_layout_and_names(rtx):
    u = rtx.MaterialUpdate
    assert [f[0] for f in u._fields_] == ["ids", "first", "count", "classes", "ready_event"]
    assert (u.ids.offset, u.first.offset, u.count.offset, u.classes.offset, u.ready_event.offset) == (0, 8, 12, 16, 24)
    assert C.sizeof(u) == 32
    assert rtx.MAT_CLASS_ALL == rtx.MAT_CLASS_GLOSSY | rtx.MAT_CLASS_MICROFACET == 3
    assert rtx.ARR["TRI_MATERIAL_CENSUS"] == 45
    assert len(set(rtx.ARR.values())) == len(rtx.ARR)


def test_signatures_cover_the_new_entries(rtx):
    """Every rt_* function the header declares has a SIGNATURES entry the library resolves."""
    with open(os.path.join(ROOT, "include", "rtx_amd.h")) as f:
        text = re.sub(r"/\*.*?\*/", "", f.read(), flags=re.S)
    declared = set(re.findall(r"\b(rt_[a-z0-9_]+)\s*\(", text))
    assert {"rt_set_triangle_materials_device", "rt_material_class_rule"} <= declared
    assert declared <= set(rtx.SIGNATURES), sorted(declared - set(rtx.SIGNATURES))
    lib = rtx.load_library()
    for name in ("rt_set_triangle_materials_device", "rt_material_class_rule"):
        res, args = rtx.SIGNATURES[name]
        fn = getattr(lib, name)
        assert fn.restype is res and list(fn.argtypes) == args


def test_wrapper_refuses_values_past_32_bits(rtx, rt):
    for kw in (dict(count=1 << 32), dict(count=4, first=-1), dict(count=4, classes=1 << 32), dict(count=-1)):
        with pytest.raises(ValueError):
            rt.set_triangle_materials_device(0x1000, **{"count": 4, **kw})


def test_device_class_rule_is_the_host_rule_for_every_id(rtx):
    """mat_class_of, the statement k_mat_set compiles, against rt_material_classes, id by id."""
    L = rtx.load_library()
    for i in range(256):
        assert L.rt_material_class_rule(i) == rtx.material_classes(np.array([i], np.uint8)), i
        assert L.rt_material_class_rule(i + 256) == L.rt_material_class_rule(i)  # the low 8 bits only
    assert L.rt_material_class_rule(5) == rtx.MAT_CLASS_GLOSSY and L.rt_material_class_rule(4) == rtx.MAT_CLASS_MICROFACET
