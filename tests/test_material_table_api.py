"""The material table at the C-ABI boundary, without a GPU (rt_set_materials, include/rtx_amd.h):
the defaults against the class rule, every argument check on a context that is created but not
inited, the order RT_ERR_ARG before RT_ERR_STATE, and the layout of the Python mirror."""
import ctypes as C
import math
import os
import re

import numpy as np
import pytest

RT_OK, RT_ERR_ARG, RT_ERR_STATE = 0, -1, -4
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "rtx_amd.h")
F32 = lambda x: float(np.float32(x))  # noqa: E731


@pytest.fixture()
def rt(rtx):
    r = rtx.RayTracer(64, 64, None)  # created, not inited: no device needed
    yield r
    r.cleanup()


def header_text():
    with open(HEADER) as f:
        return re.sub(r"/\*.*?\*/", "", f.read(), flags=re.S)


def test_constants_match_the_header(rtx):
    consts = {k: int(v.rstrip("u"), 0) for k, v in re.findall(r"#define\s+(RT_MAT_[A-Z]+(?:_[A-Z]+)?)\s+(\w+)\s", header_text())}
    assert consts["RT_MAT_LAMBERTIAN"] == rtx.MAT_LAMBERTIAN == 0
    assert consts["RT_MAT_MIRROR"] == rtx.MAT_MIRROR == 1
    assert consts["RT_MAT_GLASS"] == rtx.MAT_GLASS == 2
    assert consts["RT_MAT_MICROFACET"] == rtx.MAT_MICROFACET == 3
    assert consts["RT_MAT_EMISSIVE"] == rtx.MAT_EMISSIVE == 4
    assert consts["RT_MAT_FLAG_FLAT"] == rtx.MAT_FLAG_FLAT == 1


def test_entries_are_declared_and_bound(rtx):
    text = header_text()
    lib = rtx.load_library()
    for name in ("rt_default_material", "rt_set_materials", "rt_get_materials", "rt_reset_materials"):
        assert re.search(r"\bint\s+%s\s*\(" % name, text), name
        res, args = rtx.SIGNATURES[name]
        fn = getattr(lib, name)
        assert fn.restype is res and list(fn.argtypes) == args
    for name in ("set_materials", "get_materials", "reset_materials"):
        assert callable(getattr(rtx.RayTracer, name))


def test_structure_layout_matches_the_header(rtx):
    """The fields of rt_material in the header's order, each a 4-byte scalar or an array of them, so the
    C layout is the running sum; rt_default_material then writes through the C struct and every field
    is read back through the mirror at its own, distinguishable value."""
    body = re.search(r"typedef\s+struct\s+rt_material\s*\{(.*?)\}\s*rt_material\s*;", header_text(), flags=re.S).group(1)
    fields = re.findall(r"\b(int32_t|uint32_t|float)\s+(\w+)(?:\[(\d+)\])?\s*;", body)
    assert [f[1] for f in fields] == ["type", "flags", "color", "emission", "ior", "alpha", "f0"]
    M = rtx.Material
    assert [f[0] for f in M._fields_] == [f[1] for f in fields]
    off = 0
    ctype = {"int32_t": C.c_int32, "uint32_t": C.c_uint32, "float": C.c_float}
    for (ty, name, n), (_, mirror) in zip(fields, M._fields_):
        want = ctype[ty] * int(n) if n else ctype[ty]
        assert mirror is want or (n and mirror._type_ is ctype[ty] and mirror._length_ == int(n)), name
        assert getattr(M, name).offset == off, name
        off += 4 * (int(n) if n else 1)
    assert C.sizeof(M) == off == 52
    m = rtx.default_material(4)
    assert (m.type, m.flags) == (rtx.MAT_MICROFACET, 0)
    assert list(m.color) == [1.0] * 3 and list(m.emission) == [0.0] * 3
    assert (m.ior, m.alpha) == (F32(1.33), F32(0.05))
    assert list(m.f0) == [F32(0.56), F32(0.57), F32(0.58)]


def test_defaults_agree_with_the_class_rule(rtx):
    """All 256 ids: mirror or glass exactly when rt_material_classes says GLOSSY, microfacet exactly when
    it says MICROFACET; the types of the reference's ten entries; the constants of every entry."""
    ref = {0: rtx.MAT_EMISSIVE, 1: rtx.MAT_GLASS, 2: rtx.MAT_EMISSIVE, 3: rtx.MAT_LAMBERTIAN, 4: rtx.MAT_MICROFACET,
           5: rtx.MAT_MIRROR, 6: rtx.MAT_LAMBERTIAN, 7: rtx.MAT_LAMBERTIAN, 8: rtx.MAT_LAMBERTIAN, 9: rtx.MAT_LAMBERTIAN}
    for i in range(256):
        m = rtx.default_material(i)
        cls = rtx.material_classes([i])
        assert (m.type in (rtx.MAT_MIRROR, rtx.MAT_GLASS)) == (cls == rtx.MAT_CLASS_GLOSSY), i
        assert (m.type == rtx.MAT_MICROFACET) == (cls == rtx.MAT_CLASS_MICROFACET), i
        assert m.type == ref.get(i, rtx.MAT_MIRROR), i
        assert m.flags == 0 and list(m.color) == [1.0] * 3 and list(m.emission) == [0.0] * 3, i
        assert (m.ior, m.alpha, list(m.f0)) == (F32(1.33), F32(0.05), [F32(0.56), F32(0.57), F32(0.58)]), i
    L = rtx.load_library()
    assert L.rt_default_material(256, C.byref(rtx.Material())) == RT_ERR_ARG
    assert L.rt_default_material(3, None) == RT_ERR_ARG


def good(rtx, **kw):
    m = rtx.default_material(3)
    for k, v in kw.items():
        if isinstance(v, tuple):
            getattr(m, k)[:] = v
        else:
            setattr(m, k, v)
    return m


def test_get_returns_the_defaults_without_a_table(rtx, rt):
    got = rt.get_materials()
    assert len(got) == 256 and all(got[i] == rtx.default_material(i) for i in range(256))
    assert rt.get_materials(250, 6) == [rtx.default_material(i) for i in range(250, 256)]
    out = (rtx.Material * 4)()
    L = rt.lib
    assert L.rt_get_materials(None, 0, 4, out) == RT_ERR_ARG
    assert L.rt_get_materials(rt.h, 0, 4, None) == RT_ERR_ARG
    assert L.rt_get_materials(rt.h, 0, 0, out) == RT_ERR_ARG
    assert L.rt_get_materials(rt.h, 253, 4, out) == RT_ERR_ARG
    assert L.rt_get_materials(rt.h, 0xFFFFFFFF, 2, out) == RT_ERR_ARG


def test_argument_checks_come_before_the_init_state(rtx, rt):
    """Every RT_ERR_ARG case of the header on a context that is not inited (so RT_ERR_ARG wins over
    RT_ERR_STATE); valid arguments are RT_ERR_STATE there; nothing changes on any of them."""
    L = rt.lib
    one = (rtx.Material * 1)(good(rtx))
    assert L.rt_set_materials(None, 0, 1, one) == RT_ERR_ARG
    assert L.rt_set_materials(rt.h, 0, 1, None) == RT_ERR_ARG
    assert L.rt_set_materials(rt.h, 0, 0, one) == RT_ERR_ARG
    assert L.rt_set_materials(rt.h, 256, 1, one) == RT_ERR_ARG
    assert L.rt_set_materials(rt.h, 0xFFFFFFFF, 1, one) == RT_ERR_ARG
    big = (rtx.Material * 256)(*[good(rtx)] * 256)
    assert L.rt_set_materials(rt.h, 1, 256, big) == RT_ERR_ARG
    nan, inf = math.nan, math.inf
    bad = [dict(type=-1), dict(type=5), dict(flags=2), dict(flags=0x80000001),
           dict(color=(1.0, -0.5, 1.0)), dict(color=(nan, 1.0, 1.0)), dict(color=(1.0, 1.0, inf)),
           dict(emission=(-1.0, 0.0, 0.0)), dict(emission=(0.0, nan, 0.0)), dict(emission=(0.0, 0.0, inf)),
           dict(ior=0.0), dict(ior=-1.5), dict(ior=nan), dict(ior=inf),
           dict(alpha=0.0), dict(alpha=-0.1), dict(alpha=1.5), dict(alpha=nan),
           dict(f0=(-0.1, 0.5, 0.5)), dict(f0=(0.5, 1.5, 0.5)), dict(f0=(0.5, 0.5, nan))]
    for kw in bad:
        arr = (rtx.Material * 2)(good(rtx), good(rtx, **kw))  # the faulty entry is not the first
        assert L.rt_set_materials(rt.h, 7, 2, arr) == RT_ERR_ARG, kw
        err = L.rt_last_error(rt.h)
        assert b"rt_set_materials" in err and b"entry 8" in err, (kw, err)
        with pytest.raises(rtx.RtError):
            rt.set_materials(7, [good(rtx), good(rtx, **kw)])
    # the limits themselves are valid: alpha 1, f0 0 and 1, colour and emission 0, every type, the flag
    edge = [good(rtx, type=t, flags=f, alpha=1.0, f0=(0.0, 1.0, 0.5), color=(0.0, 2.0, 1.0), emission=(0.0, 50.0, 1.0), ior=0.5)
            for t in range(5) for f in (0, 1)]
    arr = (rtx.Material * len(edge))(*edge)
    assert L.rt_set_materials(rt.h, 246, len(edge), arr) == RT_ERR_STATE
    assert b"before rt_init" in L.rt_last_error(rt.h)
    assert L.rt_set_materials(rt.h, 0, 256, big) == RT_ERR_STATE
    assert L.rt_reset_materials(rt.h) == RT_ERR_STATE
    assert L.rt_reset_materials(None) == RT_ERR_ARG
    assert rt.get_materials() == [rtx.default_material(i) for i in range(256)]  # nothing changed


def test_wrappers_refuse_what_is_not_a_material(rtx, rt):
    with pytest.raises(ValueError):
        rt.set_materials(0, [object()])
    with pytest.raises(ValueError):
        rt.set_materials(-1, [good(rtx)])
    with pytest.raises(ValueError):
        rt.get_materials(0, -1)
    with pytest.raises(rtx.RtError):
        rt.set_materials(0, [])
    with pytest.raises(ValueError):
        rtx.default_material(-1)
    with pytest.raises(rtx.RtError):
        rtx.default_material(256)
    a, b = good(rtx), good(rtx)
    assert a == b and not (a != b)
    b.alpha = 0.5
    assert a != b
