"""Texture sets on the GPU (rt_upload_texture_set*, rt_set_material_textures).

The oracle renders with any texture pair, so a frame whose every textured hit samples one set has an
exact expectation; frames that mix sets get theirs by construction (the cube whose faces do not see
each other, tests/material_scenes.py) or from a context that holds the same pair in set 0.  Every
comparison is bit for bit, every path trace goes through trace() (PT_QUEUE[10] == 0), and the contexts
hold three sets so that set 2 tells 2 * stride from stride.
"""
import numpy as np
import pytest

import material_scenes as M
from test_gpu_material_table import cube, cube_ctx, ctrace, defaults, differing, mat, on_face  # noqa: F401 (cube: fixture)
from test_gpu_materials import MIX8, trace, with_mask
from test_gpu_pathtrace import assert_gbuffers_equal, terrain_camera
from test_gpu_texture import numpy_chain

pytestmark = pytest.mark.gpu

W, H = 96, 54
DT = 16.667
SETS = 3
MAPS = ("SOIL_ALBEDO_AO", "SOIL_NORMAL_ROUGHNESS")
ARRS = ("TEX_ALBEDO_AO", "TEX_NORMAL_ROUGHNESS")


def random_image(seed):
    img = np.random.default_rng(seed).integers(0, 65536, size=(1024, 1024, 4), dtype=np.uint16)
    img[:8, :8] = 65535  # a saturated corner: the min(65535) and the truncation at the top of the range
    return img


@pytest.fixture(scope="module")
def pairs(oracle):
    """Two texture pairs X and Y: level-0 images and the oracle's chains, computed once and never written."""
    out = {}
    for name, seeds in (("X", (11, 12)), ("Y", (21, 22))):
        imgs = [random_image(s) for s in seeds]
        chains = [oracle.mip_chain(i) for i in imgs]
        for a in imgs + chains:
            a.setflags(write=False)
        out[name] = dict(img=imgs, chain=tuple(chains))
    return out


@pytest.fixture(scope="module")
def sky(oracle):
    return oracle.sky()


def tex_rt(rtx, oracle, tmp_path, name, sets=SETS, spp=1, extra="", tuning=None, w=W, h=H):
    """The terrain at its camera with `sets` texture sets, LBVH built."""
    cfg = rtx.write_config(str(tmp_path / (name + ".toml")), w, h, spp=spp, extra=extra, tuning=tuning or {}, texture_sets=sets)
    rt = rtx.RayTracer(w, h, cfg).init()
    rt.set_delta_time(DT)
    ocam, rcam = terrain_camera(rtx, oracle, w, h)
    rt.camera = rcam
    rt.build_bvh()
    return rt, ocam


def cube_tex_ctx(rtx, oracle, tmp_path, cube, name="cube"):
    cfg = rtx.write_config(str(tmp_path / (name + ".toml")), M.CUBE_W, M.CUBE_H, mesh_file=cube["path"], texture_sets=SETS)
    rt = rtx.RayTracer(M.CUBE_W, M.CUBE_H, cfg).init()
    rt.set_delta_time(DT)
    assert rt.info().triCount == cube["n"] == 768
    rt.camera = M.cube_camera(rtx, oracle)[1]
    rt.build_bvh()
    return rt


def upload_pair(rt, pair, k):
    for name, img in zip(MAPS, pair["img"]):
        rt.upload_texture(name, img, set=k)


def chains_of(rt, k):
    return [rt.download(a, np.uint16, set=k).reshape(-1, 4) for a in ARRS]


def to_dev(a):
    """A device copy of a numpy array (uint16 as int16 bits), complete on return."""
    import torch

    a = np.array(a, order="C")  # a writable copy: the shared images are read-only
    t = torch.from_numpy(a.view(np.int16) if a.dtype == np.uint16 else a).cuda()
    torch.cuda.synchronize()
    return t


# ---------------------------------------------------------------- 1
def test_initial_contents_and_capacity(rtx, oracle, tmp_path):
    rt, _ = tex_rt(rtx, oracle, tmp_path, "a")
    assert rt.texture_sets == SETS
    base = list(oracle.textures())
    for k in range(SETS):
        for got, want in zip(chains_of(rt, k), base):
            assert np.array_equal(got, want), k
    assert (rt.get_material_textures() == 0).all()
    for a in ARRS:
        with pytest.raises(rtx.RtError, match="RT_ERR_ARG"):
            rt.download(a, np.uint16, set=SETS)
    with pytest.raises(rtx.RtError, match="rt_set_material_textures: RT_ERR_ARG"):
        rt.set_material_textures(5, [0, 2, SETS])
    assert (rt.get_material_textures() == 0).all()  # nothing changed
    rt.cleanup()
    one, _ = tex_rt(rtx, oracle, tmp_path, "b", sets=None)
    assert one.texture_sets == 1
    img = random_image(1)
    with pytest.raises(rtx.RtError, match="rt_upload_texture_set: RT_ERR_ARG"):
        one.upload_texture("SOIL_ALBEDO_AO", img, set=1)
    dev = to_dev(img)
    with pytest.raises(rtx.RtError, match="rt_upload_texture_set_device: RT_ERR_ARG"):
        one.upload_texture_device("SOIL_ALBEDO_AO", dev, 1, rtx.TEX_FORMAT_U16)
    with pytest.raises(rtx.RtError, match="rt_set_material_textures: RT_ERR_ARG"):
        one.set_material_textures(3, [1])
    with pytest.raises(rtx.RtError, match="RT_ERR_ARG"):
        one.download("TEX_ALBEDO_AO", np.uint16, set=1)
    for got, want in zip(chains_of(one, 0), base):
        assert np.array_equal(got, want)
    one.set_material_textures(0, [0] * 256)  # set 0 is every context's
    one.cleanup()


# ---------------------------------------------------------------- 2
def test_upload_lands_in_its_set_only(rtx, oracle, tmp_path, pairs):
    rt, _ = tex_rt(rtx, oracle, tmp_path, "u")
    upload_pair(rt, pairs["X"], 2)
    for got, img, want in zip(chains_of(rt, 2), pairs["X"]["img"], pairs["X"]["chain"]):
        assert np.array_equal(got, want)
        assert np.array_equal(got, numpy_chain(img))
    base = list(oracle.textures())
    for k in (0, 1):
        for got, want in zip(chains_of(rt, k), base):
            assert np.array_equal(got, want), k
    rt.cleanup()


# ---------------------------------------------------------------- 3
def test_unbound_and_never_uploaded_sets_are_the_identity(rtx, oracle, tmp_path):
    rt, _ = tex_rt(rtx, oracle, tmp_path, "i", spp=2)
    rt.set_triangle_materials(M.hashed_ids(rt.info().triCount, MIX8))
    before = trace(rt, 1)
    assert len(set(before["color"][:, 3].tolist()) & set(MIX8)) == len(set(MIX8))  # every id is on screen
    rt.set_material_textures(0, [1] * 256)
    assert (rt.get_material_textures() == 1).all()
    bound = trace(rt, 1)
    rt.reset_material_textures()
    assert (rt.get_material_textures() == 0).all()
    after = trace(rt, 1)
    rt.cleanup()
    assert_gbuffers_equal(bound, before)
    assert_gbuffers_equal(after, before)
    # the default materials, whose serial frame runs the fused chain: a binding of zeros is no binding
    rt, _ = tex_rt(rtx, oracle, tmp_path, "z", spp=2)
    plain = trace(rt, 1)
    assert rt.info().lastChain == 1
    rt.set_material_textures(0, [0] * 256)
    zeros = trace(rt, 1)
    assert rt.info().lastChain == 1
    rt.set_material_textures(3, [1])
    one = trace(rt, 1)
    assert rt.info().lastChain == 0  # the table-reading kernels, on the unsplit plan
    rt.cleanup()
    assert_gbuffers_equal(zeros, plain)
    assert_gbuffers_equal(one, plain)


# ---------------------------------------------------------------- 4
def test_bound_set_against_the_oracle(rtx, oracle, tmp_path, default_scene, pairs, sky):
    """Every triangle on id 7, id 7 bound to set 2 holding X: the oracle's frame under X.  More than half
    of the pixels that hit geometry differ from the frame under the soil atlas."""
    X = pairs["X"]
    rt, ocam = tex_rt(rtx, oracle, tmp_path, "o")
    tri = M.primary_triangles(oracle, default_scene["bvh"], W, H, ocam)
    hit = tri >= 0
    mask = np.where(hit, 7, M.SKY_MASK).astype(np.uint16)
    want = with_mask(oracle.pathtrace(default_scene["bvh"], W, H, frame_num=1, cam=ocam, sky_out=sky, tex=X["chain"]), mask)
    soil = with_mask(oracle.pathtrace(default_scene["bvh"], W, H, frame_num=1, cam=ocam, sky_out=sky, tex=oracle.textures()), mask)
    assert hit.sum() > W * H // 4
    assert differing(want, soil, hit) > hit.sum() // 2  # otherwise the comparison shows nothing
    upload_pair(rt, X, 2)
    upload_pair(rt, pairs["Y"], 1)  # the neighbour: an offset of one stride lands here
    rt.set_triangle_materials(np.full(rt.info().triCount, 7, np.uint8))
    assert_gbuffers_equal(trace(rt, 1), soil)
    rt.set_material_textures(7, [2])
    g = trace(rt, 1)
    rt.cleanup()
    assert_gbuffers_equal(g, want)
    ov, _ = tex_rt(rtx, oracle, tmp_path, "ov", extra="materialOverride = 7\n")
    upload_pair(ov, X, 2)
    ov.set_material_textures(7, [2])
    g = trace(ov, 1)
    ov.cleanup()
    assert_gbuffers_equal(g, want)


# ---------------------------------------------------------------- 5
def test_bounces_read_the_bounce_hits_set(rtx, oracle, tmp_path, pairs):
    """Mirrors, glass and GGX beside Lambertian: X as the soil atlas of context A against X in set 2 with
    every id bound to it in context B (sets 0 and 1 keep the soil atlas, which a hit reached through a
    bounce would sample if it took another hit's set, or none)."""
    frames = []
    for name, k in (("A", 0), ("B", 2)):
        rt, _ = tex_rt(rtx, oracle, tmp_path, name, spp=2)
        rt.set_triangle_materials(M.hashed_ids(rt.info().triCount, MIX8))
        upload_pair(rt, pairs["X"], k)
        if k:
            rt.set_material_textures(0, [k] * 256)
        frames.append(trace(rt, 1))
        rt.cleanup()
    assert_gbuffers_equal(frames[1], frames[0])


# ---------------------------------------------------------------- 6
FACE_IDS = {"x+": 3, "y+": 6, "z-": 7}
FACE_SETS = {"x+": 0, "y+": 1, "z-": 2}


def test_each_material_samples_its_own_set(rtx, oracle, tmp_path, cube, pairs):
    rt = cube_tex_ctx(rtx, oracle, tmp_path, cube)
    upload_pair(rt, pairs["X"], 1)
    upload_pair(rt, pairs["Y"], 2)
    rt.set_triangle_materials(M.face_table(FACE_IDS))
    frames = {}
    for k in range(SETS):  # every face on set k
        for mid in FACE_IDS.values():
            rt.set_material_textures(mid, [k])
        frames[k] = ctrace(rt)
    for face, mid in FACE_IDS.items():
        rt.set_material_textures(mid, [FACE_SETS[face]])
    got = rt.get_material_textures()
    assert [got[FACE_IDS[f]] for f in FACE_IDS] == [0, 1, 2] and got.sum() == 3
    mixed = ctrace(rt)
    rt.cleanup()
    pick = np.zeros(M.CUBE_W * M.CUBE_H, np.int64)  # the sky is every frame's
    for face, k in FACE_SETS.items():
        sel = on_face(cube, face)
        pick[sel] = k
        for other in range(SETS):
            if other != k:
                assert differing(frames[k], frames[other], sel) > sel.sum() // 2, (face, other)
    assert_gbuffers_equal(mixed, M.compose_by_pixel(frames, pick))


# ---------------------------------------------------------------- 7
def test_flat_ignores_the_binding_and_the_binding_outlives_table_and_mesh(rtx, oracle, tmp_path, cube, pairs):
    rt = cube_tex_ctx(rtx, oracle, tmp_path, cube)
    upload_pair(rt, pairs["X"], 2)
    rt.set_triangle_materials(M.face_table({"y+": 6}))
    unbound = ctrace(rt)
    rt.set_material_textures(6, [2])
    bound = ctrace(rt)
    yp = on_face(cube, "y+")
    assert differing(bound, unbound, yp) > yp.sum() // 2
    rt.set_materials(0, defaults(rtx))  # a custom table of the defaults: the binding still applies
    assert_gbuffers_equal(ctrace(rt), bound)
    flat6 = mat(rtx, 6, color=(1.0, 0.5, 0.25), flags=rtx.MAT_FLAG_FLAT)
    rt.set_materials(6, [flat6])
    flat_bound = ctrace(rt)
    rt.reset_material_textures()
    flat_unbound = ctrace(rt)
    assert_gbuffers_equal(flat_bound, flat_unbound)
    assert differing(flat_bound, bound, yp) > yp.sum() // 2
    rt.set_material_textures(6, [2])
    assert rt.get_materials()[6] == flat6  # the material table is unaffected
    rt.reset_materials()
    assert rt.get_material_textures()[6] == 2 and rt.get_material_textures().sum() == 2
    assert_gbuffers_equal(ctrace(rt), bound)
    tris = M.cube_triangles()
    rt.set_mesh(np.ascontiguousarray(tris.reshape(-1, 3)), np.arange(3 * len(tris), dtype=np.uint32).reshape(-1, 3))
    assert rt.get_material_textures()[6] == 2 and rt.get_material_textures().sum() == 2
    rt.build_bvh()
    rt.set_triangle_materials(M.face_table({"y+": 6}))
    assert_gbuffers_equal(ctrace(rt), bound)
    rt.cleanup()


# ---------------------------------------------------------------- 8
@pytest.mark.parametrize("fmt", ["U16", "U8"])
def test_device_upload_equals_the_host_upload(rtx, oracle, tmp_path, fmt):
    import torch

    rng = np.random.default_rng(31)
    if fmt == "U16":
        srcs = [random_image(s) for s in (41, 42)]
        imgs = srcs
    else:
        srcs = [rng.integers(0, 256, size=(1024, 1024, 4), dtype=np.uint8) for _ in range(2)]
        for s in srcs:
            s[:8, :8] = 255
        imgs = [s.astype(np.uint16) * 257 for s in srcs]
        assert imgs[0][0, 0, 0] == 65535
    rt, _ = tex_rt(rtx, oracle, tmp_path, "h")
    for name, img in zip(MAPS, imgs):
        rt.upload_texture(name, img, set=1)
    want = chains_of(rt, 1)
    main = torch.cuda.Stream(device=0)
    rt.set_stream(main.cuda_stream)
    devs = [to_dev(s) for s in srcs]
    for name, d in zip(MAPS, devs):
        rt.upload_texture_device(name, d, 2, getattr(rtx, "TEX_FORMAT_" + fmt))
        with torch.cuda.stream(main):  # the caller's later work on the context stream follows the read
            d.zero_()
    got = chains_of(rt, 2)
    base = list(oracle.textures())
    for k in range(2):
        assert np.array_equal(got[k], want[k]), MAPS[k]
        assert np.array_equal(got[k], oracle.mip_chain(imgs[k])), MAPS[k]
        assert np.array_equal(chains_of(rt, 0)[k], base[k])
        assert np.array_equal(chains_of(rt, 1)[k], want[k])
    assert all(int(d.count_nonzero()) == 0 for d in devs)
    rt.cleanup()
    torch.cuda.synchronize()


# ---------------------------------------------------------------- 9
def serial_frames(rtx, oracle, tmp_path, name, uploads):
    """RGBA8 of draws 1.. of a context with every id bound to set 1, which gets uploads[k] (a pair or
    None) through the host upload before draw k."""
    rt, _ = tex_rt(rtx, oracle, tmp_path, name)
    rt.set_material_textures(0, [1] * 256)
    out = []
    rgba = np.zeros((H, W, 4), np.uint8)
    for pair in uploads:
        if pair is not None:
            upload_pair(rt, pair, 1)
        rt.draw(rgba)
        out.append(rgba.copy())
    assert rt.download("PT_QUEUE", np.uint32)[10] == 0
    rt.cleanup()
    return out


def test_ordering_without_a_wait(rtx, oracle, tmp_path, pairs):
    """Pipelined frame 1, a device upload into the bound set, pipelined frame 2, one sync: frame 1 keeps
    the old texels, frame 2 has the new ones."""
    import torch

    X, Y = pairs["X"], pairs["Y"]
    want = serial_frames(rtx, oracle, tmp_path, "s", [X, Y])
    stale = serial_frames(rtx, oracle, tmp_path, "t", [X, None])
    assert np.array_equal(want[0], stale[0]) and not np.array_equal(want[1], stale[1])
    rt, _ = tex_rt(rtx, oracle, tmp_path, "p")
    rt.set_material_textures(0, [1] * 256)
    upload_pair(rt, X, 1)
    devs = [to_dev(i) for i in Y["img"]]
    targets = [torch.zeros((H, W, 4), dtype=torch.uint8, device="cuda") for _ in range(2)]
    torch.cuda.synchronize()
    rt.draw_device(targets[0].data_ptr(), asynchronous=True)
    for name, d in zip(MAPS, devs):
        rt.upload_texture_device(name, d, 1, rtx.TEX_FORMAT_U16)
    rt.draw_device(targets[1].data_ptr(), asynchronous=True)
    rt.sync()
    assert rt.download("PT_QUEUE", np.uint32)[10] == 0
    got = [t.cpu().numpy() for t in targets]
    for got_chain, chain in zip(chains_of(rt, 1), Y["chain"]):
        assert np.array_equal(got_chain, chain)
    rt.cleanup()
    assert np.array_equal(got[0], want[0])
    assert np.array_equal(got[1], want[1])


# ---------------------------------------------------------------- 10
@pytest.mark.parametrize("change", ["binding", "device_upload"])
def test_nothing_traced_ahead_leaks_into_a_synchronous_draw(rtx, oracle, tmp_path, pairs, change):
    """Synchronous draws trace and shade the next frame's camera rays ahead.  A binding change, or a
    device upload, between draws 2 and 3: draw 3's path-trace outputs (albedo, normal, depth: no history
    enters them) are those of a fresh context that had the new state from the start, and the whole
    sequence of frames equals the one of a context that traces nothing ahead."""
    X, Y = pairs["X"], pairs["Y"]
    w, h = 64, 36

    def sequence(spec, when, name):
        """when: the draw ahead of which the state changes (0: before the first, None: never)."""
        rt, _ = tex_rt(rtx, oracle, tmp_path, name, tuning={"syncSpec": spec}, w=w, h=h)
        upload_pair(rt, X, 1)
        if change == "device_upload":
            rt.set_material_textures(0, [1] * 256)
            devs = [to_dev(i) for i in Y["img"]]
        rgba = np.zeros((h, w, 4), np.uint8)
        seq = []
        for k in range(4):
            if when == k:
                if change == "binding":
                    rt.set_material_textures(0, [1] * 256)
                else:
                    for m, d in zip(MAPS, devs):
                        rt.upload_texture_device(m, d, 1, rtx.TEX_FORMAT_U16)
            rt.draw(rgba)
            seq.append(rgba.copy())
        gb = {k: rt.get_buffer(k.upper(), None, np.uint16).copy() for k in ("albedo", "normal", "depth")}
        assert rt.download("PT_QUEUE", np.uint32)[10] == 0
        rt.cleanup()
        return seq, gb

    off, _ = sequence(False, 2, "off")
    on, _ = sequence(True, 2, "on")
    never, _ = sequence(True, None, "nv")
    for k, (x, y) in enumerate(zip(off, on)):
        assert np.array_equal(x, y), "draw %d" % (k + 1)
    assert np.array_equal(on[1], never[1]) and not np.array_equal(on[2], never[2])
    # the last draw's path-trace outputs against a fresh context with the new state from the start
    _, late = sequence(True, 3, "lt")
    _, fresh = sequence(True, 0, "fr")
    _, old = sequence(True, None, "ol")
    for k in late:
        assert np.array_equal(late[k], fresh[k]), k
    assert not np.array_equal(late["albedo"], old["albedo"])


# ---------------------------------------------------------------- 11
def test_resume_split_runs_the_table_plan_under_a_binding(rtx, oracle, tmp_path, pairs):
    """Serial with resumeSplit 0 and 2, and pipelined with resumeSplit 2 (where the lean pass would run on
    a stream of its own): one frame, on the unsplit table plan."""
    import torch

    frames = []
    for split, pipelined in ((0, False), (2, False), (2, True)):
        rt, _ = tex_rt(rtx, oracle, tmp_path, "r%d%d" % (split, pipelined), spp=2, tuning={"resumeSplit": split})
        if pipelined:
            post = torch.cuda.Stream(device=0)
            rt.set_post_stream(post.cuda_stream)
        upload_pair(rt, pairs["X"], 1)
        upload_pair(rt, pairs["Y"], 2)
        n = rt.info().triCount
        rt.set_triangle_materials(M.hashed_ids(n, (3, 6, 7)))
        rt.set_material_textures(3, [0])
        rt.set_material_textures(6, [1, 2])
        frames.append(trace(rt, 1))
        assert rt.info().lastChain == 0
        assert rt.download("PT_QUEUE", np.uint32)[23] == 0  # no shading list: resume<3> ran unsplit
        rt.cleanup()
    assert_gbuffers_equal(frames[1], frames[0])
    assert_gbuffers_equal(frames[2], frames[0])
    assert len(set(frames[0]["color"][:, 3].tolist()) & {3, 6, 7}) == 3
