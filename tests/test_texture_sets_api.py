"""Texture sets at the C-ABI boundary, without a GPU (rt_upload_texture_set*, rt_set_material_textures;
include/rtx_amd.h): the header against the Python mirror, [scene] textureSets in
rt_create and rt_init, every argument check that precedes the init state, in the stated order, on a
context that is created but not inited, and the wrappers' own validation."""
import ctypes as C
import os
import re

import numpy as np
import pytest

RT_OK, RT_ERR_ARG, RT_ERR_IO, RT_ERR_STATE = 0, -1, -3, -4
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "rtx_amd.h")
CALLS = ("rt_get_texture_sets", "rt_upload_texture_set", "rt_upload_texture_set_device", "rt_set_material_textures",
         "rt_get_material_textures", "rt_reset_material_textures")
ALBEDO, NORMAL, HEIGHT = 0, 1, 2


@pytest.fixture()
def rt(rtx):
    r = rtx.RayTracer(64, 64, None)  # created, not inited: no device needed
    yield r
    r.cleanup()


def header_text():
    with open(HEADER) as f:
        return re.sub(r"/\*.*?\*/", "", f.read(), flags=re.S)


def test_constants_match_the_header(rtx):
    text = header_text()
    consts = {k: int(v, 0) for k, v in re.findall(r"#define\s+(RT_TEX\w+)\s+(\d+)\s", text)}
    assert consts["RT_TEXTURE_SETS_MAX"] == rtx.TEXTURE_SETS_MAX == 16
    assert consts["RT_TEX_FORMAT_U16"] == rtx.TEX_FORMAT_U16 == 0
    assert consts["RT_TEX_FORMAT_U8"] == rtx.TEX_FORMAT_U8 == 1
    assert consts["RT_TEX_SOIL_ALBEDO_AO"] == rtx.TEX["SOIL_ALBEDO_AO"] == ALBEDO
    assert consts["RT_TEX_SOIL_NORMAL_ROUGHNESS"] == rtx.TEX["SOIL_NORMAL_ROUGHNESS"] == NORMAL
    assert re.search(r"#define\s+RT_ARR_TEX_SET\(k\)\s+\(\(k\)\s*<<\s*8\)", text)
    assert max(rtx.ARR.values()) < 256  # the set index rides above every array name


def test_entries_are_declared_and_bound(rtx):
    text = header_text()
    lib = rtx.load_library()
    for name in CALLS:
        assert re.search(r"\bint\s+%s\s*\(" % name, text), name
        res, args = rtx.SIGNATURES[name]
        fn = getattr(lib, name)
        assert fn.restype is res and list(fn.argtypes) == args
    for name in ("upload_texture_device", "set_material_textures", "get_material_textures", "reset_material_textures"):
        assert callable(getattr(rtx.RayTracer, name))
    assert isinstance(rtx.RayTracer.texture_sets, property)


def test_upload_structure_matches_the_header(rtx):
    body = re.search(r"typedef\s+struct\s+rt_texture_upload\s*\{(.*?)\}\s*rt_texture_upload\s*;", header_text(), flags=re.S).group(1)
    fields = re.findall(r"\b(const void\*|void\*|uint32_t|int32_t)\s+(\w+)\s*;", body)
    assert [f[1] for f in fields] == ["texels", "set", "which", "format", "ready_event"]
    ctype = {"const void*": C.c_void_p, "void*": C.c_void_p, "uint32_t": C.c_uint32, "int32_t": C.c_int32}
    U = rtx.TextureUpload
    assert [(n, t) for n, t in U._fields_] == [(name, ctype[ty]) for ty, name in fields]
    assert [getattr(U, n).offset for n, _ in U._fields_] == [0, 8, 12, 16, 24]
    assert C.sizeof(U) == 32


@pytest.mark.parametrize("value", ['"x"', "x", "-1", "1.5", "[2]"])
def test_unparsable_texture_sets_is_an_io_error(rtx, tmp_path, value):
    cfg = rtx.write_config(str(tmp_path / "c.toml"), 64, 64, texture_sets=value)
    assert "textureSets = %s\n" % value in open(cfg).read()
    with pytest.raises(rtx.RtError, match="rt_create: RT_ERR_IO .*textureSets"):
        rtx.RayTracer(64, 64, cfg)


def test_too_many_sets_is_an_argument_error_of_init(rtx, tmp_path):
    """Raised before any device call: RT_ERR_ARG, not RT_ERR_NO_DEVICE, on a machine without a GPU too."""
    r = rtx.RayTracer(64, 64, rtx.write_config(str(tmp_path / "c.toml"), 64, 64, texture_sets=17))
    try:
        assert r.lib.rt_init(r.h) == RT_ERR_ARG
        assert b"textureSets" in r.lib.rt_last_error(r.h)
        assert r.texture_sets == 17  # as configured; rt_init is what refuses it
    finally:
        r.cleanup()


@pytest.mark.parametrize("value,count", [(None, 1), (0, 1), (1, 1), (3, 3), (16, 16)])
def test_accepted_counts(rtx, tmp_path, value, count):
    cfg = rtx.write_config(str(tmp_path / "c.toml"), 64, 64, texture_sets=value)
    assert ("textureSets" in open(cfg).read()) == (value is not None)
    r = rtx.RayTracer(64, 64, cfg)
    try:
        assert r.texture_sets == count
        n = C.c_uint32(99)
        assert r.lib.rt_get_texture_sets(None, C.byref(n)) == RT_ERR_ARG
        assert r.lib.rt_get_texture_sets(r.h, None) == RT_ERR_ARG
        assert n.value == 99
    finally:
        r.cleanup()


def test_host_upload_checks_come_before_the_init_state(rtx, rt):
    L = rt.lib
    img = np.zeros((1024, 1024, 4), np.uint16)
    p = img.ctypes.data
    assert L.rt_upload_texture_set(None, 0, ALBEDO, p, 1024, 1024, 4) == RT_ERR_ARG
    assert L.rt_upload_texture_set(rt.h, 0, ALBEDO, None, 1024, 1024, 4) == RT_ERR_ARG
    for which in (-1, 3, 99):
        assert L.rt_upload_texture_set(rt.h, 0, which, p, 1024, 1024, 4) == RT_ERR_ARG, which
    assert L.rt_upload_texture_set(rt.h, 1, HEIGHT, p, 1024, 1024, 1) == RT_ERR_ARG  # the height map is set 0's
    for w, h, c in ((512, 1024, 4), (1024, 512, 4), (1024, 1024, 3), (1024, 1024, 1), (0, 0, 4)):
        assert L.rt_upload_texture_set(rt.h, 0, NORMAL, p, w, h, c) == RT_ERR_ARG, (w, h, c)
    assert L.rt_upload_texture_set(rt.h, 0, HEIGHT, p, 1024, 1024, 4) == RT_ERR_ARG
    # valid arguments: the state; the set index is checked against the inited context only
    for s in (0, 1, 15, 16, 0xFFFFFFFF):
        assert L.rt_upload_texture_set(rt.h, s, ALBEDO, p, 1024, 1024, 4) == RT_ERR_STATE, s
        assert b"before rt_init" in L.rt_last_error(rt.h)
    assert L.rt_upload_texture_set(rt.h, 0, HEIGHT, p, 1024, 1024, 1) == RT_ERR_STATE


def test_device_upload_checks_come_before_the_init_state(rtx, rt):
    L = rt.lib
    U = rtx.TextureUpload
    ok = dict(texels=0x1000, set=0, which=ALBEDO, format=rtx.TEX_FORMAT_U8, ready_event=None)

    def call(**kw):
        return L.rt_upload_texture_set_device(rt.h, C.byref(U(**dict(ok, **kw))))

    assert L.rt_upload_texture_set_device(None, C.byref(U(**ok))) == RT_ERR_ARG
    assert L.rt_upload_texture_set_device(rt.h, None) == RT_ERR_ARG
    assert call(texels=None) == RT_ERR_ARG
    for which in (-1, HEIGHT, 3):
        assert call(which=which) == RT_ERR_ARG, which
    for fmt in (2, 0xFFFFFFFF):
        assert call(format=fmt) == RT_ERR_ARG, fmt
    for ptr in (0x1001, 0x1002, 0x1003):
        assert call(texels=ptr) == RT_ERR_ARG, ptr
        assert b"aligned" in L.rt_last_error(rt.h)
    for fmt in (rtx.TEX_FORMAT_U16, rtx.TEX_FORMAT_U8):
        for which in (ALBEDO, NORMAL):
            for s in (0, 2, 16, 0xFFFFFFFF):
                assert call(format=fmt, which=which, set=s, texels=0x1004) == RT_ERR_STATE
    assert b"before rt_init" in L.rt_last_error(rt.h)


def test_binding_checks_come_before_the_init_state(rtx, rt):
    L = rt.lib
    sets = np.zeros(256, np.uint8)
    p = sets.ctypes.data
    for fn in (L.rt_set_material_textures, L.rt_get_material_textures):
        assert fn(None, 0, 1, p) == RT_ERR_ARG
        assert fn(rt.h, 0, 1, None) == RT_ERR_ARG
        assert fn(rt.h, 0, 0, p) == RT_ERR_ARG
        assert fn(rt.h, 256, 1, p) == RT_ERR_ARG
        assert fn(rt.h, 1, 256, p) == RT_ERR_ARG
        assert fn(rt.h, 0xFFFFFFFF, 2, p) == RT_ERR_ARG
        assert fn(rt.h, 0, 256, p) == RT_ERR_STATE
        assert fn(rt.h, 255, 1, p) == RT_ERR_STATE
    sets[:] = 200  # an entry past the sets is checked against the inited context only
    assert L.rt_set_material_textures(rt.h, 0, 256, p) == RT_ERR_STATE
    assert b"before rt_init" in L.rt_last_error(rt.h)
    assert L.rt_reset_material_textures(None) == RT_ERR_ARG
    assert L.rt_reset_material_textures(rt.h) == RT_ERR_STATE


def test_wrappers_validate_their_arguments(rtx, rt):
    img = np.zeros((1024, 1024, 4), np.uint16)
    with pytest.raises(rtx.RtError, match="rt_upload_texture_set: RT_ERR_STATE"):
        rt.upload_texture("SOIL_ALBEDO_AO", img, set=2)
    with pytest.raises(rtx.RtError, match="rt_upload_texture: RT_ERR_STATE"):
        rt.upload_texture("SOIL_ALBEDO_AO", img)
    with pytest.raises(rtx.RtError, match="rt_upload_texture_set: RT_ERR_ARG"):
        rt.upload_texture("SOIL_HEIGHT", img[:, :, 0], set=1)
    with pytest.raises(ValueError):
        rt.upload_texture("SOIL_ALBEDO_AO", img, set=-1)
    with pytest.raises(ValueError):
        rt.upload_texture("SOIL_ALBEDO_AO", np.zeros(16, np.uint16))
    with pytest.raises(ValueError):
        rt.upload_texture_device("SOIL_HEIGHT", 0x1000, 0, rtx.TEX_FORMAT_U16)
    with pytest.raises(ValueError):
        rt.upload_texture_device("SOIL_ALBEDO_AO", 0x1000, 0, 2)
    with pytest.raises(ValueError):
        rt.upload_texture_device("SOIL_ALBEDO_AO", 0x1000, -1, rtx.TEX_FORMAT_U8)
    with pytest.raises(rtx.RtError, match="rt_upload_texture_set_device: RT_ERR_ARG"):
        rt.upload_texture_device("SOIL_ALBEDO_AO", 0x1002, 0, rtx.TEX_FORMAT_U8)
    with pytest.raises(rtx.RtError, match="rt_upload_texture_set_device: RT_ERR_STATE"):
        rt.upload_texture_device("SOIL_NORMAL_ROUGHNESS", 0x1000, 1, rtx.TEX_FORMAT_U16)

    class Tensor:  # what the wrapper asks of a tensor
        def __init__(self, nbytes, contiguous=True):
            self.n, self.c = nbytes, contiguous

        def data_ptr(self):
            return 0x2000

        def numel(self):
            return self.n

        def element_size(self):
            return 1

        def is_contiguous(self):
            return self.c

    with pytest.raises(ValueError):
        rt.upload_texture_device("SOIL_ALBEDO_AO", Tensor(1024 * 1024 * 4), 0, rtx.TEX_FORMAT_U16)  # half the bytes
    with pytest.raises(ValueError):
        rt.upload_texture_device("SOIL_ALBEDO_AO", Tensor(1024 * 1024 * 8), 0, rtx.TEX_FORMAT_U8)
    with pytest.raises(ValueError):
        rt.upload_texture_device("SOIL_ALBEDO_AO", Tensor(1024 * 1024 * 4, False), 0, rtx.TEX_FORMAT_U8)
    with pytest.raises(rtx.RtError, match="RT_ERR_STATE"):
        rt.upload_texture_device("SOIL_ALBEDO_AO", Tensor(1024 * 1024 * 4), 0, rtx.TEX_FORMAT_U8)
    for bad in ([256], [-1], [[0, 1]], [0.5], ["a"]):
        with pytest.raises(ValueError):
            rt.set_material_textures(0, bad)
    with pytest.raises(ValueError):
        rt.set_material_textures(-1, [0])
    with pytest.raises(rtx.RtError, match="rt_set_material_textures: RT_ERR_ARG"):
        rt.set_material_textures(0, [])
    with pytest.raises(rtx.RtError, match="rt_set_material_textures: RT_ERR_ARG"):
        rt.set_material_textures(255, [0, 0])
    with pytest.raises(rtx.RtError, match="rt_set_material_textures: RT_ERR_STATE"):
        rt.set_material_textures(0, [0] * 256)
    with pytest.raises(ValueError):
        rt.get_material_textures(0, -1)
    with pytest.raises(rtx.RtError, match="rt_get_material_textures: RT_ERR_ARG"):
        rt.get_material_textures(0, 257)
    with pytest.raises(rtx.RtError, match="rt_get_material_textures: RT_ERR_STATE"):
        rt.get_material_textures()
    with pytest.raises(rtx.RtError, match="rt_reset_material_textures: RT_ERR_STATE"):
        rt.reset_material_textures()
    with pytest.raises(ValueError):
        rt.download("VERTICES", set=1)
    with pytest.raises(ValueError):
        rt.download("TEX_HEIGHT", set=1)
    with pytest.raises(ValueError):
        rt.download("TEX_ALBEDO_AO", set=-1)
    with pytest.raises(rtx.RtError, match="RT_ERR_STATE"):
        rt.download("TEX_ALBEDO_AO", set=1)
    assert rt.lib.rt_array_bytes(rt.h, rtx.ARR["TEX_ALBEDO_AO"] | (16 << 8)) == 0
    assert rt.lib.rt_array_bytes(rt.h, rtx.ARR["TEX_HEIGHT"] | (1 << 8)) == 0
    assert rt.lib.rt_array_bytes(rt.h, rtx.ARR["VERTICES"] | (1 << 8)) == 0
