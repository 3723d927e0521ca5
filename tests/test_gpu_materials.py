"""Per-triangle materials on the GPU (rt_set_triangle_materials).

The oracle renders one scene-wide material, so the mixed frames get exact expectations by
construction (tests/material_scenes.py): a uniform table against the override, ids of one type
against the override of the type with the mask from the table, and one type per face of a cube whose
faces do not see each other.  Paths that do cross between types (a mirror seeing Lambert, glass
seeing anything) have no oracle; they are covered by agreement, bit for bit, between the kernel plans
a frame can take.  Every comparison is bit-exact, and the path tracer's internal error counter
(PT_QUEUE[10]) must be 0 after every launch.
"""
import numpy as np
import pytest

import material_scenes as M
from scene_bin import bin_bvh, write_bin
from test_gpu_pathtrace import assert_gbuffers_equal, gpu_gbuffers, terrain_camera

pytestmark = pytest.mark.gpu

W, H = 96, 54
DT = 16.667
MIX8 = [3, 3, 3, 5, 4, 1, 0, 7]


@pytest.fixture(scope="module")
def sky_tex(oracle):
    return oracle.sky(), oracle.textures()


@pytest.fixture(scope="module")
def cube(oracle, tmp_path_factory):
    path = write_bin(str(tmp_path_factory.mktemp("cube") / "cube.bin"), M.cube_triangles())
    bvh, _, _, n = bin_bvh(oracle, path)
    cam, _ = M.cube_camera(None, oracle)
    tri = M.primary_triangles(oracle, bvh, M.CUBE_W, M.CUBE_H, cam)
    return dict(path=path, bvh=bvh, n=n, tri=tri)


def terrain_rt(rtx, oracle, tmp_path, name, spp=1, extra="", tuning=None, w=W, h=H):
    cfg = rtx.write_config(str(tmp_path / (name + ".toml")), w, h, spp=spp, extra=extra, tuning=tuning or {})
    rt = rtx.RayTracer(w, h, cfg).init()
    ocam, rcam = terrain_camera(rtx, oracle, w, h)
    rt.camera = rcam
    rt.build_bvh()
    return rt, ocam


def cube_rt(rtx, oracle, tmp_path, cube):
    cfg = rtx.write_config(str(tmp_path / "cube.toml"), M.CUBE_W, M.CUBE_H, mesh_file=cube["path"])
    rt = rtx.RayTracer(M.CUBE_W, M.CUBE_H, cfg).init()
    rt.set_delta_time(DT)
    assert rt.info().triCount == cube["n"] == 768
    return rt


def trace(rt, frame, w=W, h=H):
    """One detail launch: the G-buffers with RAYS; no internal error."""
    rt.path_trace(frame, detail=True)
    rt.sync()
    g = gpu_gbuffers(rt, w, h)
    assert rt.download("PT_QUEUE", np.uint32)[10] == 0  # kCntError
    return g


def with_mask(o, mask):
    """The oracle frame `o` with the material mask of the colour buffer replaced."""
    g = {k: v.copy() for k, v in o.items()}
    g["color"][:, 3] = mask
    return g


def test_uniform_table_equals_the_override(rtx, oracle, tmp_path, default_scene, sky_tex):
    """A table of all m is [render] materialOverride = m, which the oracle renders.  Tables are set
    whole and in two partial calls (first > 0); TRI_MATERIALS returns what was set; after the reset
    the frame is a fresh context's again."""
    s, tex = sky_tex
    rt, ocam = terrain_rt(rtx, oracle, tmp_path, "u")
    n = rt.info().triCount
    assert n == default_scene["tri_count"]
    before = rt.download("TRI_MATERIALS")
    assert before.shape == (n,) and (before == 3).all()
    fresh = trace(rt, 1)
    split = n // 3 + 1
    for k, m in enumerate((0, 1, 3, 4, 5)):
        ids = np.full(n, m, np.uint8)
        if k % 2 == 0:
            rt.set_triangle_materials(ids)
        else:  # the upper part first: in between the table is mixed
            rt.set_triangle_materials(ids[split:], first=split)
            mixed = rt.download("TRI_MATERIALS")
            assert (mixed[split:] == m).all() and (mixed[:split] != m).all()
            rt.set_triangle_materials(ids[:split])
        assert np.array_equal(rt.download("TRI_MATERIALS"), ids)
        g = trace(rt, 1)
        o = oracle.pathtrace(default_scene["bvh"], W, H, frame_num=1, cam=ocam, sky_out=s, tex=tex, material_override=m)
        assert_gbuffers_equal(g, o)
        assert rt.info().lastChain == (1 if m in (0, 3) else 0), m  # the plan follows the census
    rt.reset_triangle_materials()
    assert (rt.download("TRI_MATERIALS") == 3).all()
    g = trace(rt, 1)
    assert rt.info().lastChain == 1
    rt.cleanup()
    assert_gbuffers_equal(g, fresh)
    assert_gbuffers_equal(g, oracle.pathtrace(default_scene["bvh"], W, H, frame_num=1, cam=ocam, sky_out=s, tex=tex))


@pytest.mark.parametrize("palette,override", [((3, 7, 9), 3), ((5, 12), 5)], ids=["lambert-3-7-9", "mirror-5-12"])
def test_same_type_ids_render_as_the_type(rtx, oracle, tmp_path, default_scene, sky_tex, palette, override):
    """Ids of one type scattered over the terrain, spp 2: every buffer and the ray counts equal the
    oracle's override frame of the type, paths crossing freely between the ids; the mask alone differs,
    and it is the table's id at sample 0's triangle.  The Lambertian table keeps the default plan."""
    s, tex = sky_tex
    rt, ocam = terrain_rt(rtx, oracle, tmp_path, "t", spp=2)
    n = rt.info().triCount
    ids = M.hashed_ids(n, palette)
    assert set(np.unique(ids).tolist()) == set(palette)
    rt.set_triangle_materials(ids)
    g = trace(rt, 1)
    chain = rt.info().lastChain
    rt.cleanup()
    o = oracle.pathtrace(default_scene["bvh"], W, H, frame_num=1, spp=2, cam=ocam, sky_out=s, tex=tex,
                         material_override=override)
    tri = M.primary_triangles(oracle, default_scene["bvh"], W, H, ocam)
    mask = np.where(tri >= 0, ids.astype(np.int64)[np.maximum(tri, 0)], M.SKY_MASK).astype(np.uint16)
    assert len(set(mask[tri >= 0].tolist())) == len(palette)  # every id is on screen
    assert_gbuffers_equal(g, with_mask(o, mask))
    assert chain == (1 if override == 3 else 0)


@pytest.mark.parametrize("assign", [(5, 3, 4), (0, 4, 5), (3, 5, 12)], ids=["5-3-4", "0-4-5", "3-5-12"])
def test_cube_one_type_per_face(rtx, oracle, tmp_path, cube, sky_tex, assign):
    """(x+, y+, z-) = assign on the cube: at every pixel the oracle's override frame of that pixel's
    face.  (5, 3, 4) holds a mirror and the microfacet material at once: the <kGlossy, kMF> kernels."""
    s, tex = sky_tex
    w, h = M.CUBE_W, M.CUBE_H
    table = M.face_table(dict(zip(("x+", "y+", "z-"), assign)))
    rt = cube_rt(rtx, oracle, tmp_path, cube)
    ocam, rcam = M.cube_camera(rtx, oracle)
    rt.camera = rcam
    rt.build_bvh()
    rt.set_triangle_materials(table)
    assert rtx.material_classes(table) == rtx.material_classes(np.array(assign, np.uint8))
    g = trace(rt, 1, w, h)
    assert rt.info().lastChain == 0
    rt.cleanup()
    frames = {m: oracle.pathtrace(cube["bvh"], w, h, frame_num=1, cam=ocam, sky_out=s, tex=tex, material_override=m)
              for m in set(assign)}
    tri = cube["tri"]
    pick = np.where(tri >= 0, table[np.maximum(tri, 0)], assign[0]).astype(np.int64)  # the sky is every frame's
    seen = {M.CUBE_FACES[f] for f in np.unique(tri[tri >= 0] // M.CUBE_FACE_TRIS)}
    assert seen == {"x+", "y+", "z-"}
    assert_gbuffers_equal(g, M.compose_by_pixel(frames, pick))


def launch_mixed(rtx, oracle, tmp_path, name, palette, frame=2, extra="", tuning=None, pipelined=False):
    """Frame `frame` at spp 2 of the terrain under hashed_ids(palette), in one configuration."""
    rt, _ = terrain_rt(rtx, oracle, tmp_path, name, spp=2, extra=extra, tuning=tuning)
    if pipelined:
        import torch

        post = torch.cuda.Stream(device=0)
        rt.set_post_stream(post.cuda_stream)
    ids = M.hashed_ids(rt.info().triCount, palette)
    rt.set_triangle_materials(ids)
    g = trace(rt, frame)
    chain = rt.info().lastChain
    rt.cleanup()
    return g, chain


def test_plans_agree_on_crossing_cross_type_paths(rtx, oracle, tmp_path):
    """The eight-way mix (Lambert, mirror, microfacet, glass, emissive) scattered over the terrain: its
    paths cross between the types.  All G-buffers and RAYS are equal between the default serial path
    trace, resumeSplit = 0, a pipelined context, a contiguous strip and an interleaved one."""
    from rtx.dist import strip_blocks

    ref, chain = launch_mixed(rtx, oracle, tmp_path, "a", MIX8)
    assert chain == 0
    assert len(set(ref["color"][:, 3].tolist()) & set(MIX8)) == len(set(MIX8))  # every id is on screen
    assert ref["rays"].max() >= 4  # glossy steps traced inline
    g, _ = launch_mixed(rtx, oracle, tmp_path, "b", MIX8, tuning={"resumeSplit": 0})
    assert_gbuffers_equal(g, ref)
    g, _ = launch_mixed(rtx, oracle, tmp_path, "c", MIX8, pipelined=True)
    assert_gbuffers_equal(g, ref)
    g, _ = launch_mixed(rtx, oracle, tmp_path, "d", MIX8, extra="stripY0 = 16\nstripRows = 24\n")
    assert_gbuffers_equal(g, ref, rows=slice(16 * W, 40 * W))
    g, _ = launch_mixed(rtx, oracle, tmp_path, "e", MIX8, extra="stripCount = 3\nstripIndex = 1\n")
    owned = np.concatenate([np.arange(y0 * W, (y0 + rows) * W) for y0, rows in strip_blocks(H, 3, 1)])
    assert owned.size > 0
    assert_gbuffers_equal(g, ref, rows=owned)


def test_chain_and_four_kernels_agree_on_a_default_class_table(rtx, oracle, tmp_path):
    """A table without glossy or microfacet ids (Lambertian 3, 7, 9 and emissive 0, 2) keeps the fused
    chain: [tuning] chain = "always" against "off" (the split four kernels)."""
    palette = [3, 7, 9, 0, 2]
    a, chain_a = launch_mixed(rtx, oracle, tmp_path, "ca", palette, tuning={"chain": "always"})
    b, chain_b = launch_mixed(rtx, oracle, tmp_path, "cb", palette, tuning={"chain": "off"})
    assert (chain_a, chain_b) == (1, 0)
    assert len(set(a["color"][:, 3].tolist()) & set(palette)) == len(palette)
    assert_gbuffers_equal(a, b)


def test_setter_drops_the_camera_rays_traced_ahead(rtx, oracle, tmp_path):
    """Synchronous draws trace the next frame's camera rays (and shade them) ahead; a table set between
    two draws must not be met by what was traced under the previous table, also when the launch
    parameters do not change (a second table of the same classes at the same address).  The draws
    keep the lookahead alive up to each setter (no host read of the context in between); HDR of every
    frame and RGBA8 where a read does not disturb the sequence equal those with syncSpec off."""
    w, h = 64, 36
    outs = []
    for spec in (False, True):
        rt, _ = terrain_rt(rtx, oracle, tmp_path, "s%d" % spec, tuning={"syncSpec": spec}, w=w, h=h)
        rt.set_delta_time(DT)
        n = rt.info().triCount
        a = M.hashed_ids(n, MIX8)
        b = a[::-1].copy()
        assert rtx.material_classes(a) == rtx.material_classes(b) and not np.array_equal(a, b)
        hdr = np.zeros((h, w, 4), np.float32)
        seq = []

        def draw(read_rgba):
            rt.draw(None, hdr)
            seq.append(hdr.view(np.uint32).copy())
            if read_rgba:
                seq.append(rt.download("RGBA8").copy())

        draw(False)
        draw(False)
        rt.set_triangle_materials(a)          # the first set: the launch parameters change
        draw(False)
        rt.set_triangle_materials(b)          # the second: they do not
        draw(True)
        draw(False)
        rt.set_triangle_materials(a[:n // 2])  # a partial one
        draw(True)
        draw(False)
        rt.reset_triangle_materials()
        draw(True)
        assert rt.download("PT_QUEUE", np.uint32)[10] == 0
        rt.cleanup()
        outs.append(seq)
    assert len(outs[0]) == len(outs[1]) == 11
    for k, (x, y) in enumerate(zip(*outs)):
        assert np.array_equal(x, y), "output %d" % k


def test_denoiser_material_terms_on_a_mixed_frame(rtx, oracle, tmp_path, cube):
    """Three frames of the cube with (x+, y+, z-) = (5, 3, 4) and a moving camera: the denoiser's three
    *_sigma_material edge weights now see differing masks.  The GPU's G-buffers of each frame go
    through the oracle's denoiser (temporal passes included, its state carried over the frames), and
    RENDER_COLOR, SCALED_COLOR and RGBA8 are bit-equal."""
    w, h = M.CUBE_W, M.CUBE_H
    rt = cube_rt(rtx, oracle, tmp_path, cube)
    rt.set_triangle_materials(M.face_table({"x+": 5, "y+": 3, "z-": 4}))
    dn = oracle.Denoiser(w, h)
    masks = set()
    for f in (1, 2, 3):
        _, rcam = M.cube_camera(rtx, oracle, f - 1)
        rt.camera = rcam
        rt.build_bvh()
        rt.path_trace(f)
        rt.sync()
        gb = dict(color=rt.get_buffer("RENDER_COLOR", (w * h, 4), np.uint16),
                  normal=rt.get_buffer("NORMAL", (w * h, 4), np.uint16),
                  albedo=rt.get_buffer("ALBEDO", (w * h, 4), np.uint16),
                  depth=rt.get_buffer("DEPTH", (w * h,), np.uint16),
                  motion=rt.get_buffer("MOTION", (w * h, 2), np.uint16))
        assert rt.download("PT_QUEUE", np.uint32)[10] == 0
        masks |= set(gb["color"][:, 3].tolist())
        rt.denoise_post(f)
        rt.sync()
        o = dn.draw(gb, f, delta_time=DT)
        for name, ref in (("RENDER_COLOR", o["color"]), ("SCALED_COLOR", o["scaled"])):
            got = rt.get_buffer(name, ref.shape, np.uint16)
            assert np.array_equal(got, ref), (f, name, int((got != ref).any(axis=1).sum()))
        assert np.array_equal(rt.download("RGBA8").reshape(-1, 4), o["rgba"]), f
    rt.cleanup()
    assert masks == {3, 4, 5, M.SKY_MASK}
