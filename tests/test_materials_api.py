"""Per-triangle materials at the C-ABI boundary, without a GPU: argument and state checks of
rt_set_triangle_materials / rt_reset_triangle_materials (include/rtx_amd.h), rt_material_classes (the
one statement of which ids select which kernel class) over every id, the input checks of the Python
wrapper, and the oracle-side premise of the cube scene the GPU tests compare mixed frames on."""
import ctypes as C

import numpy as np
import pytest

import material_scenes as M
from scene_bin import bin_bvh, write_bin

RT_OK, RT_ERR_ARG, RT_ERR_STATE = 0, -1, -4
GLOSSY, MICROFACET = 1, 2


@pytest.fixture()
def rt(rtx):
    r = rtx.RayTracer(64, 64, None)  # created, not inited: no device needed
    yield r
    r.cleanup()


def test_set_and_reset_before_init_are_state_errors(rt):
    ids = np.full(4, 5, np.uint8)
    assert rt.lib.rt_set_triangle_materials(rt.h, ids.ctypes.data, 0, 4) == RT_ERR_STATE
    assert b"before rt_init" in rt.lib.rt_last_error(rt.h)
    assert rt.lib.rt_reset_triangle_materials(rt.h) == RT_ERR_STATE
    assert b"before rt_init" in rt.lib.rt_last_error(rt.h)


def test_null_arguments_and_empty_ranges_are_argument_errors(rt):
    ids = np.full(4, 5, np.uint8)
    L = rt.lib
    assert L.rt_set_triangle_materials(None, ids.ctypes.data, 0, 4) == RT_ERR_ARG
    assert L.rt_set_triangle_materials(rt.h, None, 0, 4) == RT_ERR_ARG
    assert L.rt_set_triangle_materials(rt.h, ids.ctypes.data, 0, 0) == RT_ERR_ARG
    assert L.rt_set_triangle_materials(rt.h, ids.ctypes.data, 3, 0) == RT_ERR_ARG
    assert L.rt_reset_triangle_materials(None) == RT_ERR_ARG
    c = C.c_uint32(77)
    assert L.rt_material_classes(ids.ctypes.data, 4, None) == RT_ERR_ARG
    assert L.rt_material_classes(None, 4, C.byref(c)) == RT_ERR_ARG
    assert c.value == 77
    assert L.rt_material_classes(None, 0, C.byref(c)) == RT_OK and c.value == 0  # the empty set


def expected_class(i):
    """The table of the issue: mirror / glass ids (1, 5, every id >= 10) are glossy, 4 is the microfacet
    material, the Lambertian and emissive ids (0, 2, 3, 6..9) select nothing."""
    if i in (1, 5) or i >= 10:
        return GLOSSY
    return MICROFACET if i == 4 else 0


def test_material_classes_of_every_id(rtx):
    for i in range(256):
        assert rtx.material_classes(np.array([i], np.uint8)) == expected_class(i), i
    assert (rtx.MAT_CLASS_GLOSSY, rtx.MAT_CLASS_MICROFACET) == (GLOSSY, MICROFACET)


@pytest.mark.parametrize("ids,want", [
    ([3, 7, 9, 0, 2, 6, 8], 0),
    ([3, 3, 4], MICROFACET),
    ([3, 5, 3], GLOSSY),
    ([0, 1], GLOSSY),
    ([3, 12, 255], GLOSSY),
    ([5, 3, 4], GLOSSY | MICROFACET),
    ([3, 3, 3, 5, 4, 1, 0, 7], GLOSSY | MICROFACET),
    ([], 0),
], ids=["lambert-emissive", "microfacet", "mirror", "glass", "out-of-table", "mirror-microfacet", "eight-way", "empty"])
def test_material_classes_of_mixed_arrays(rtx, ids, want):
    assert rtx.material_classes(np.array(ids, np.uint8)) == want
    big = np.full(100000, 3, np.uint8)  # one id among many decides
    if ids:
        big[54321] = ids[-1]
        assert rtx.material_classes(big) == expected_class(ids[-1])


class _NoLibrary:
    """Stands in for librtx: any call through it fails the test."""

    def __getattr__(self, name):
        raise AssertionError("the wrapper called %s for an array it must refuse" % name)


@pytest.mark.parametrize("bad", [
    np.zeros(8, np.int32),
    np.zeros(8, np.int8),
    np.zeros((4, 2), np.uint8),
    np.zeros(16, np.uint8)[::2],
    [3, 3, 5],
    bytes(8),
], ids=["int32", "int8", "2d", "strided", "list", "bytes"])
def test_wrapper_refuses_bad_arrays_before_the_library(rt, bad):
    lib = rt.lib
    rt.lib = _NoLibrary()
    try:
        with pytest.raises(ValueError):
            rt.set_triangle_materials(bad)
        with pytest.raises(ValueError):
            rt.set_triangle_materials(np.zeros(4, np.uint8), first=-1)
    finally:
        rt.lib = lib


def test_cube_faces_do_not_see_each_other_on_the_oracle(oracle, tmp_path):
    """The premise of the GPU cube tests (material_scenes.py): the camera sees faces x+, y+ and z-,
    and for the overrides those tests assign (emissive 0, Lambertian 3, microfacet 4, mirror 5 and its
    out-of-table twin 12) the frame of the whole cube equals, on every pixel of a face, the frame of
    that face alone, in every buffer and in the ray counts.  Glass (1) is not part of it."""
    w, h = M.CUBE_W, M.CUBE_H
    tris = M.cube_triangles()
    assert tris.shape == (768, 3, 3)
    b, _, _, n = bin_bvh(oracle, write_bin(str(tmp_path / "cube.bin"), tris))
    assert n == 768
    cam, _ = M.cube_camera(None, oracle)
    face = M.primary_triangles(oracle, b, w, h, cam)
    face = np.where(face >= 0, face // M.CUBE_FACE_TRIS, -1)
    assert {M.CUBE_FACES[f]: int((face == f).sum()) for f in range(6) if (face == f).any()} == M.CUBE_VISIBLE
    s, tex = oracle.sky(), oracle.textures()
    alone = {}
    for name in M.CUBE_VISIBLE:
        f = M.CUBE_FACES.index(name)
        path = write_bin(str(tmp_path / ("face%d.bin" % f)), tris[f * M.CUBE_FACE_TRIS:(f + 1) * M.CUBE_FACE_TRIS])
        alone[f] = bin_bvh(oracle, path)[0]
    for m in (0, 3, 4, 5, 12):
        whole = oracle.pathtrace(b, w, h, frame_num=1, cam=cam, sky_out=s, tex=tex, material_override=m)
        for f, bf in alone.items():
            one = oracle.pathtrace(bf, w, h, frame_num=1, cam=cam, sky_out=s, tex=tex, material_override=m)
            sel = face == f
            for k in whole:
                assert np.array_equal(whole[k][sel], one[k][sel]), (m, M.CUBE_FACES[f], k)
    # ids of one type render alike but for the mask (what the same-type GPU test builds on)
    for a, twin in ((5, 12), (3, 7), (0, 2)):
        ga = oracle.pathtrace(b, w, h, frame_num=1, cam=cam, sky_out=s, tex=tex, material_override=a)
        gb = oracle.pathtrace(b, w, h, frame_num=1, cam=cam, sky_out=s, tex=tex, material_override=twin)
        for k in ga:
            x, y = (ga[k][:, :3], gb[k][:, :3]) if k == "color" else (ga[k], gb[k])
            assert np.array_equal(x, y), (a, twin, k)
        hit = face >= 0
        assert (ga["color"][hit, 3] == a).all() and (gb["color"][hit, 3] == twin).all()
        assert (ga["color"][~hit, 3] == M.SKY_MASK).all()
