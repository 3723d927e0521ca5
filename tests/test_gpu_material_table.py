"""The material table on the GPU (rt_set_materials).

The oracle knows the reference's constants only, so every expectation is exact by construction: the
defaults passed through the table are the identity; a type moved to another id is the override frame
of that type; parameters are compared between entries, faces of the cube whose faces do not see each
other (tests/material_scenes.py), or against arithmetic that is exact in half precision (a scale by a
power of two, an emission that needs no rounding).  Every comparison is bit for bit, and the path
tracer's error counter (PT_QUEUE[10]) is 0 after every launch (trace()).
"""
import numpy as np
import pytest

import material_scenes as M
from scene_bin import bin_bvh, write_bin
from test_gpu_materials import MIX8, terrain_rt, trace, with_mask
from test_gpu_pathtrace import assert_gbuffers_equal, terrain_camera

pytestmark = pytest.mark.gpu

W, H = 96, 54
DT = 16.667
GBUF = ("color", "normal", "albedo", "depth", "motion", "rays")
HALF_MIN_NORMAL = 2.0 ** -14


@pytest.fixture(scope="module")
def sky_tex(oracle):
    return oracle.sky(), oracle.textures()


@pytest.fixture(scope="module")
def cube(oracle, tmp_path_factory):
    path = write_bin(str(tmp_path_factory.mktemp("cube") / "cube.bin"), M.cube_triangles())
    bvh, _, _, n = bin_bvh(oracle, path)
    cam, _ = M.cube_camera(None, oracle)
    tri = M.primary_triangles(oracle, bvh, M.CUBE_W, M.CUBE_H, cam)
    face = np.where(tri >= 0, tri // M.CUBE_FACE_TRIS, -1)
    return dict(path=path, bvh=bvh, n=n, tri=tri, face=face)


def cube_ctx(rtx, oracle, tmp_path, cube, spp=1, name="cube"):
    """The cube at its camera, LBVH built."""
    cfg = rtx.write_config(str(tmp_path / (name + ".toml")), M.CUBE_W, M.CUBE_H, mesh_file=cube["path"], spp=spp)
    rt = rtx.RayTracer(M.CUBE_W, M.CUBE_H, cfg).init()
    rt.set_delta_time(DT)
    assert rt.info().triCount == cube["n"] == 768
    _, rcam = M.cube_camera(rtx, oracle)
    rt.camera = rcam
    rt.build_bvh()
    return rt


def ctrace(rt, frame=1):
    return trace(rt, frame, M.CUBE_W, M.CUBE_H)


def on_face(cube, name):
    sel = cube["face"] == M.CUBE_FACES.index(name)
    assert sel.sum() == M.CUBE_VISIBLE[name]
    return sel


def mat(rtx, base, **kw):
    """default_material(base) with fields replaced."""
    m = rtx.default_material(base)
    for k, v in kw.items():
        if isinstance(v, tuple):
            getattr(m, k)[:] = v
        else:
            setattr(m, k, v)
    return m


def defaults(rtx):
    return [rtx.default_material(i) for i in range(256)]


def assert_equal_but_mask(a, b):
    x = {k: v.copy() for k, v in a.items()}
    x["color"][:, 3] = b["color"][:, 3]
    assert_gbuffers_equal(x, b)


def differing(a, b, sel):
    """Pixels of sel whose colour (without the mask) differs."""
    return int(((a["color"][:, :3] != b["color"][:, :3]).any(axis=1) & sel).sum())


# ---------------------------------------------------------------- 1: defaults are the identity
def test_default_table_is_the_identity_on_the_terrain(rtx, oracle, tmp_path):
    """Terrain under hashed_ids(MIX8), spp 2 (all five types, paths crossing between them): the frame
    with the defaults passed through rt_set_materials equals, in every G-buffer and RAYS, the same
    context's frame before the call, and again after rt_reset_materials."""
    rt, _ = terrain_rt(rtx, oracle, tmp_path, "id", spp=2)
    rt.set_triangle_materials(M.hashed_ids(rt.info().triCount, MIX8))
    before = trace(rt, 1)
    assert len(set(before["color"][:, 3].tolist()) & set(MIX8)) == len(set(MIX8))  # every id is on screen
    assert rt.get_materials() == defaults(rtx)
    rt.set_materials(0, defaults(rtx))
    assert rt.get_materials() == defaults(rtx)
    table = trace(rt, 1)
    assert rt.info().lastChain == 0
    rt.reset_materials()
    assert rt.get_materials() == defaults(rtx)
    after = trace(rt, 1)
    rt.cleanup()
    assert_gbuffers_equal(table, before)
    assert_gbuffers_equal(after, before)


def test_default_table_is_the_identity_on_the_cube(rtx, oracle, tmp_path, cube):
    """The cube with (x+, y+, z-) = (5, 3, 4); a partial set keeps the other entries; get returns what
    was set."""
    rt = cube_ctx(rtx, oracle, tmp_path, cube)
    rt.set_triangle_materials(M.face_table({"x+": 5, "y+": 3, "z-": 4}))
    before = ctrace(rt)
    rt.set_materials(3, defaults(rtx)[3:6])  # the first set: the other entries are the defaults
    assert rt.get_materials() == defaults(rtx)
    table = ctrace(rt)
    custom = mat(rtx, 200, type=rtx.MAT_GLASS, ior=1.7, alpha=0.5, f0=(0.1, 0.2, 0.3), color=(0.5, 2.0, 0.0),
                 emission=(1.0, 0.0, 3.0), flags=rtx.MAT_FLAG_FLAT)
    rt.set_materials(200, [custom])  # an id no triangle has
    got = rt.get_materials()
    assert got[200] == custom and got[:200] + got[201:] == defaults(rtx)[:200] + defaults(rtx)[201:]
    assert rt.get_materials(199, 3) == [rtx.default_material(199), custom, rtx.default_material(201)]
    unused = ctrace(rt)
    rt.reset_materials()
    assert rt.get_materials() == defaults(rtx)
    after = ctrace(rt)
    rt.cleanup()
    assert set(before["color"][:, 3].tolist()) == {3, 4, 5, M.SKY_MASK}
    for g in (table, unused, after):
        assert_gbuffers_equal(g, before)


# ---------------------------------------------------------------- 2: type by table
def test_type_follows_the_entry(rtx, oracle, tmp_path, default_scene, sky_tex):
    """Entry 7 a mirror, entry 8 the microfacet material: the terrain with every triangle on 7 (8) is
    the oracle's materialOverride = 5 (4) frame with the mask 7 (8)."""
    s, tex = sky_tex
    rt, ocam = terrain_rt(rtx, oracle, tmp_path, "ty")
    n = rt.info().triCount
    rt.set_materials(7, [mat(rtx, 7, type=rtx.MAT_MIRROR),
                         mat(rtx, 8, type=rtx.MAT_MICROFACET, alpha=0.05, f0=(0.56, 0.57, 0.58))])
    tri = M.primary_triangles(oracle, default_scene["bvh"], W, H, ocam)
    for mid, override in ((7, 5), (8, 4)):
        ids = M.hashed_ids(n, (mid,))
        rt.set_triangle_materials(ids)
        g = trace(rt, 1)
        o = oracle.pathtrace(default_scene["bvh"], W, H, frame_num=1, cam=ocam, sky_out=s, tex=tex, material_override=override)
        mask = np.where(tri >= 0, mid, M.SKY_MASK).astype(np.uint16)
        assert_gbuffers_equal(g, with_mask(o, mask))
    rt.cleanup()


# ---------------------------------------------------------------- 3: per-id lookup
def test_each_hit_reads_its_own_entry(rtx, oracle, tmp_path, cube):
    """Entry 4 (alpha 0.05) on x+ and entry 8 (microfacet, alpha 0.25, f0 (0.9, 0.5, 0.1)) on z-: at every
    pixel the frame of that pixel's entry on both faces; the two single-entry frames differ on z-."""
    rt = cube_ctx(rtx, oracle, tmp_path, cube)
    rt.set_materials(4, [mat(rtx, 4, alpha=0.05)])
    rt.set_materials(8, [mat(rtx, 8, type=rtx.MAT_MICROFACET, alpha=0.25, f0=(0.9, 0.5, 0.1))])
    frames = {}
    for mid in (4, 8):
        rt.set_triangle_materials(M.face_table({"x+": mid, "z-": mid}))
        frames[mid] = ctrace(rt)
    rt.set_triangle_materials(M.face_table({"x+": 4, "z-": 8}))
    mixed = ctrace(rt)
    rt.cleanup()
    zm = on_face(cube, "z-")
    pick = np.where(zm, 8, 4).astype(np.int64)  # y+ (id 3) and the sky are every frame's
    expect = M.compose_by_pixel(frames, pick)
    assert set(expect["color"][:, 3].tolist()) == {3, 4, 8, M.SKY_MASK}  # the mask is the table's
    assert_gbuffers_equal(mixed, expect)
    assert differing(frames[4], frames[8], zm) > zm.sum() // 2


# ---------------------------------------------------------------- 4: glass
def test_index_of_refraction(rtx, oracle, tmp_path, cube):
    """Entry 1 at ior 1.5 on x+ against entry 11 made glass of ior 1.5 on the same face: equal but for
    the mask; and ior 1.5 differs from the reference's 1.33 on that face."""
    rt = cube_ctx(rtx, oracle, tmp_path, cube)
    rt.set_triangle_materials(M.face_table({"x+": 1}))
    g133 = ctrace(rt)
    rt.set_materials(1, [mat(rtx, 1, ior=1.5)])
    g1 = ctrace(rt)
    rt.set_materials(11, [mat(rtx, 11, type=rtx.MAT_GLASS, ior=1.5)])
    rt.set_triangle_materials(M.face_table({"x+": 11}))
    g11 = ctrace(rt)
    rt.cleanup()
    xp = on_face(cube, "x+")
    assert set(g1["color"][xp, 3].tolist()) == {1} and set(g11["color"][xp, 3].tolist()) == {11}
    assert_equal_but_mask(g1, g11)
    assert differing(g1, g133, xp) > 0
    assert not differing(g1, g133, ~xp)  # no path from another face enters the glass


# ---------------------------------------------------------------- 5: colour, textured
def scaled_equal(oracle, got, ref, scale, sel):
    """Half bit patterns `got` == RN_half(ref * scale) on sel, scale a power of two: exact where the
    scaled half is normal (or zero); returns the count of pixels skipped for a subnormal."""
    want = oracle.h2f(np.ascontiguousarray(ref)).astype(np.float32) * np.float32(scale)
    sub = (np.abs(want) < HALF_MIN_NORMAL) & (want != 0)
    ok = oracle.f2h(np.ascontiguousarray(want)) == got
    bad = sel & ~sub & ~ok
    assert not bad.any(), "scale %g: %d pixels differ, first %s" % (scale, bad.sum(), np.nonzero(bad)[0][:5])
    return sel & sub


def test_colour_multiplies_the_textured_albedo(rtx, oracle, tmp_path, default_scene):
    """Terrain, every triangle on id 3, entry 3 with colour (0.5, 0.25, 1): the albedo channels are the
    untinted ones times 0.5, 0.25 and 1 (a power of two commutes with both roundings); normal, depth,
    motion and mask are bit-identical."""
    rt, ocam = terrain_rt(rtx, oracle, tmp_path, "co")
    rt.set_materials(3, [mat(rtx, 3, color=(1.0, 1.0, 1.0))])
    plain = trace(rt, 1)
    rt.set_materials(3, [mat(rtx, 3, color=(0.5, 0.25, 1.0))])
    tint = trace(rt, 1)
    rt.cleanup()
    hit = M.primary_triangles(oracle, default_scene["bvh"], W, H, ocam) >= 0
    assert hit.sum() > W * H // 4
    skipped = np.zeros(W * H, bool)
    for ch, scale in enumerate((0.5, 0.25, 1.0)):
        skipped |= scaled_equal(oracle, tint["albedo"][:, ch], plain["albedo"][:, ch], scale, hit)
    print("subnormal albedo pixels skipped: %d of %d" % (skipped.sum(), hit.sum()))
    assert skipped.sum() <= hit.sum() // 100
    assert (plain["albedo"][hit, :3] != 0).all(axis=1).sum() > hit.sum() // 2  # the comparison is not of zeros
    for k in ("normal", "depth", "motion", "rays"):
        assert np.array_equal(tint[k], plain[k]), k
    assert np.array_equal(tint["color"][:, 3], plain["color"][:, 3])
    assert np.array_equal(tint["albedo"][~hit], plain["albedo"][~hit])


# ---------------------------------------------------------------- 6: flat
def test_flat_entry_skips_the_texture(rtx, oracle, tmp_path, cube):
    """Face y+ on entry 6, flat with colour (1, 0.5, 0.25): its albedo is colour * (1 + |n.d|), so
    g = r / 2 and b = r / 4 exactly with 1 <= r <= 2; its normal is the hit's smooth normal, which
    the oracle's intersection gives; the other pixels are the frame without the flag."""
    rt = cube_ctx(rtx, oracle, tmp_path, cube)
    rt.set_triangle_materials(M.face_table({"y+": 6}))
    rt.set_materials(6, [mat(rtx, 6, color=(1.0, 0.5, 0.25))])
    textured = ctrace(rt)
    rt.set_materials(6, [mat(rtx, 6, color=(1.0, 0.5, 0.25), flags=rtx.MAT_FLAG_FLAT)])
    flat = ctrace(rt)
    rt.cleanup()
    yp = on_face(cube, "y+")
    a = oracle.h2f(np.ascontiguousarray(flat["albedo"][yp, :3]))
    assert ((a[:, 0] >= 1.0) & (a[:, 0] <= 2.0)).all()
    assert np.array_equal(a[:, 1], a[:, 0] * np.float32(0.5)) and np.array_equal(a[:, 2], a[:, 0] * np.float32(0.25))
    assert len(np.unique(a[:, 0])) > 8  # the factor varies over the face
    ocam, _ = M.cube_camera(None, oracle)
    rays, _ = oracle.primary_rays(M.CUBE_W, M.CUBE_H, 1, ocam)
    hits = oracle.intersect(cube["bvh"], rays)
    # the half conversion of the comparison is the kernel's: the depth buffer is the kernel's half of
    # the hit distance the oracle computes too
    hit = cube["tri"] >= 0
    assert np.array_equal(oracle.f2h(np.ascontiguousarray(hits["t"][hit])), flat["depth"][hit])
    want = oracle.f2h(np.ascontiguousarray(hits["fakeNormal"][yp])).reshape(-1, 3)
    assert np.array_equal(flat["normal"][yp, :3], want)
    assert (flat["normal"][yp, 3] == 0).all()
    assert (textured["normal"][yp, :3] != want).any()  # the texture block does move the normal
    for k in GBUF:
        assert np.array_equal(flat[k][~yp], textured[k][~yp]), k
    for k in ("depth", "motion"):
        assert np.array_equal(flat[k], textured[k]), k


# ---------------------------------------------------------------- 7: emission, direct
EMIT = (0.5, 2.0, 12.0)
SEEN = (0.5, 2.0, 10.0)  # behind the path tracer's clamp at 10; all three are halfs


@pytest.mark.parametrize("spp", [1, 4])
def test_emission_of_a_camera_hit(rtx, oracle, tmp_path, cube, spp):
    """Face x+ on id 0 with emission (0.5, 2, 12): a pixel whose samples all land on the face shows
    exactly (0.5, 2, 10); every other buffer, and every pixel no sample of which sees the face, is
    the frame at emission 0."""
    rt = cube_ctx(rtx, oracle, tmp_path, cube, spp=spp, name="em%d" % spp)
    rt.set_triangle_materials(M.face_table({"x+": 0}))
    rt.set_materials(0, [mat(rtx, 0, emission=(0.0, 0.0, 0.0))])
    dark = ctrace(rt)
    rt.set_materials(0, [mat(rtx, 0, emission=EMIT)])
    lit = ctrace(rt)
    rt.cleanup()
    ocam, _ = M.cube_camera(None, oracle)
    f = M.CUBE_FACES.index("x+")
    faces = []
    for idx in range(spp * (1 - 1) + 1, spp * 1 + 1):  # the frame indices of frame 1's samples
        tri = M.primary_triangles(oracle, cube["bvh"], M.CUBE_W, M.CUBE_H, ocam, frame=idx)
        faces.append(np.where(tri >= 0, tri // M.CUBE_FACE_TRIS, -1) == f)
    every, some = np.logical_and.reduce(faces), np.logical_or.reduce(faces)
    assert every.sum() >= 100
    if spp == 1:
        assert np.array_equal(every, on_face(cube, "x+"))
    want = oracle.f2h(np.array(SEEN, np.float32))
    assert (lit["color"][every, :3] == want).all()
    assert (dark["color"][every, :3] == 0).all()
    for k in GBUF:
        if k != "color":
            assert np.array_equal(lit[k], dark[k]), k
    assert np.array_equal(lit["color"][:, 3], dark["color"][:, 3])
    assert np.array_equal(lit["color"][~some], dark["color"][~some])


# ---------------------------------------------------------------- 8: emission, indirect
def test_emission_reaches_other_surfaces_through_bounces(rtx, oracle, tmp_path, default_scene):
    """Terrain with a quarter of the triangles on id 0, emission E against 2 E: a path ends on an
    emitter or it does not and nothing else depends on the emission, so every colour channel is equal
    or exactly doubled; pixels that do not see an emitter directly are among the doubled ones (the
    queue tracers and the resume kernels carried it); against emission 0 nothing gets darker."""
    rt, ocam = terrain_rt(rtx, oracle, tmp_path, "ei")
    n = rt.info().triCount
    ids = M.hashed_ids(n, (3, 3, 3, 0))
    rt.set_triangle_materials(ids)
    frames = []
    for e in (0.0, 0.5, 1.0):
        rt.set_materials(0, [mat(rtx, 0, emission=(e, e, e))])
        frames.append(trace(rt, 1))
    rt.cleanup()
    zero, one, two = frames
    for k in GBUF:
        if k != "color":
            assert np.array_equal(one[k], two[k]) and np.array_equal(one[k], zero[k]), k
    c0, c1, c2 = (oracle.h2f(np.ascontiguousarray(g["color"][:, :3])) for g in (zero, one, two))
    same = one["color"][:, :3] == two["color"][:, :3]
    doubled = (c2 == c1 * np.float32(2.0)) & ~same
    sub = (np.abs(c1) < HALF_MIN_NORMAL) & (c1 != 0)
    tri = M.primary_triangles(oracle, default_scene["bvh"], W, H, ocam)
    hit = tri >= 0
    bad = ~(same | doubled | sub)
    assert not bad.any(), "%d channels neither equal nor doubled, first pixels %s" % (bad.sum(), np.nonzero(bad.any(axis=1))[0][:5])
    skipped = (sub & ~same & ~doubled).any(axis=1)
    print("subnormal colour pixels skipped: %d of %d" % (skipped.sum(), hit.sum()))
    assert skipped.sum() <= hit.sum() // 100
    direct = hit & (ids[np.maximum(tri, 0)] == 0)
    assert direct.sum() > 100 and doubled[direct].all(axis=1).sum() > direct.sum() // 2
    indirect = hit & ~direct
    assert doubled[indirect].any(axis=1).sum() >= 1
    print("pixels lit through a bounce: %d of %d" % (doubled[indirect].any(axis=1).sum(), indirect.sum()))
    assert (c1 >= c0).all() and (c2 >= c0).all()


# ---------------------------------------------------------------- 9: plans and streams
def launch_defaults_table(rtx, oracle, tmp_path, name, tuning=None, pipelined=False):
    rt, _ = terrain_rt(rtx, oracle, tmp_path, name, spp=2, tuning=tuning)
    if pipelined:
        import torch

        post = torch.cuda.Stream(device=0)
        rt.set_post_stream(post.cuda_stream)
    rt.set_triangle_materials(M.hashed_ids(rt.info().triCount, MIX8))
    rt.set_materials(0, defaults(rtx))
    g = trace(rt, 1)
    rt.cleanup()
    return g


def test_plans_and_streams_agree_under_a_table(rtx, oracle, tmp_path):
    ref = launch_defaults_table(rtx, oracle, tmp_path, "pa")
    assert_gbuffers_equal(launch_defaults_table(rtx, oracle, tmp_path, "pb", pipelined=True), ref)
    assert_gbuffers_equal(launch_defaults_table(rtx, oracle, tmp_path, "pc", tuning={"resumeSplit": 2}), ref)


def test_setter_drops_what_was_traced_ahead_and_outlives_the_mesh(rtx, oracle, tmp_path):
    """Synchronous draws trace (and shade) the next frame's camera rays ahead; a table set between two
    draws shows in the next frame: the sequence equals the one with syncSpec off, and differs from the
    one that never sets a table.  rt_set_mesh leaves the table alone."""
    w, h = 64, 36
    tinted = mat(rtx, 3, color=(0.25, 1.0, 0.25))

    def sequence(spec, set_table):
        rt, _ = terrain_rt(rtx, oracle, tmp_path, "d%d%d" % (spec, set_table), tuning={"syncSpec": spec}, w=w, h=h)
        rt.set_delta_time(DT)
        hdr = np.zeros((h, w, 4), np.float32)
        seq = []
        for k in range(5):
            if set_table and k == 2:
                rt.set_materials(3, [tinted])
            if set_table and k == 4:
                rt.reset_materials()
            rt.draw(None, hdr)
            seq.append(hdr.view(np.uint32).copy())
        assert rt.download("PT_QUEUE", np.uint32)[10] == 0
        if set_table:
            rt.set_materials(3, [tinted])
            want = rt.get_materials()
            tris = M.cube_triangles()
            rt.set_mesh(np.ascontiguousarray(tris.reshape(-1, 3)), np.arange(3 * len(tris), dtype=np.uint32).reshape(-1, 3))
            assert rt.info().triCount == len(tris)
            assert rt.get_materials() == want and want[3] == tinted
            assert (rt.download("TRI_MATERIALS") == 3).all()
        rt.cleanup()
        return seq

    off, on, never = sequence(False, True), sequence(True, True), sequence(True, False)
    for k, (x, y) in enumerate(zip(off, on)):
        assert np.array_equal(x, y), "draw %d" % k
    assert np.array_equal(on[1], never[1])
    assert not np.array_equal(on[2], never[2])
