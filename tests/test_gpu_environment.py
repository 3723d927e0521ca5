"""Environment maps on the GPU (rt_set_environment*): the tables an image gives
against the host rule (rtx.environment_table) and the oracle's scan, and frames under an environment
against the oracle, which takes the sky table and its CDF as inputs (sky_out=).  Frames are 96 x 54 on
the default terrain.  Every comparison is bit-exact, and the path tracer's internal error counter
(PT_QUEUE[10]) must be 0 after every launch (trace())."""
import numpy as np
import pytest

import environment_inputs as E
from test_gpu_materials import terrain_rt, trace
from test_gpu_pathtrace import assert_gbuffers_equal, terrain_camera

pytestmark = pytest.mark.gpu

W, H = 96, 54
DT = 16.667
_tables = {}


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def tables(rtx, oracle, name):
    """(table, pdf, cdf) of a named source by the host rule and the oracle's scan; computed once."""
    if name not in _tables:
        img, layout = E.source(name)
        table, pdf = rtx.environment_table(img, layout, E.SCALES[name])
        cdf = oracle.scan(pdf.reshape(-1), 256)
        for a in (table, pdf, cdf):
            a.setflags(write=False)
        _tables[name] = (table, pdf, cdf)
    return _tables[name]


def sets_rt(rtx, oracle, tmp_path, name, sky_sets, spp=1, cam=None):
    """terrain_rt with [scene] skySets."""
    cfg = rtx.write_config(str(tmp_path / (name + ".toml")), W, H, spp=spp, sky_sets=sky_sets)
    rt = rtx.RayTracer(W, H, cfg).init()
    ocam, rcam = cam or terrain_camera(rtx, oracle, W, H)
    rt.camera = rcam
    rt.build_bvh()
    return rt, ocam


def to_dev(a):
    import torch

    t = torch.from_numpy(np.array(a, order="C")).cuda()
    torch.cuda.synchronize()
    return t


def fmt_of(rtx, img):
    return rtx.ENV_FORMAT_F32X4 if img.dtype == np.float32 else rtx.ENV_FORMAT_F16X4


def read_tables(rt):
    return dict(sky=rt.get_buffer("SKY", (256, 512, 4), np.float32), sun=rt.get_buffer("SUN", (32, 32, 4), np.float32),
                sky_pdf=rt.download("SKY_PDF", np.float32), sky_cdf=rt.download("SKY_CDF", np.float32),
                sun_pdf=rt.download("SUN_PDF", np.float32), sun_cdf=rt.download("SUN_CDF", np.float32))


def assert_tables(got, table, pdf, cdf, s, what):
    assert np.array_equal(bits(got["sky"]), bits(table)), what + ": sky table"
    assert np.array_equal(bits(got["sky_pdf"]), bits(pdf).reshape(-1)), what + ": sky pdf"
    assert np.array_equal(bits(got["sky_cdf"]), bits(cdf)), what + ": sky cdf"
    for k in ("sun", "sun_pdf", "sun_cdf"):
        assert np.array_equal(bits(got[k]).reshape(-1), bits(s[k]).reshape(-1)), what + ": " + k


@pytest.mark.parametrize("name", E.SOURCES)
def test_tables_of_every_source(rtx, oracle, tmp_path, name):
    """RT_BUF_SKY and SKY_PDF are the host rule's, SKY_CDF the oracle's scan of the pdf, the SUN arrays
    oracle.sky()'s; the host setter on a one-set context, the device and the host setter on a two-set
    context give the same bits."""
    img, layout = E.source(name)
    table, pdf, cdf = tables(rtx, oracle, name)
    s = oracle.sky()
    rt1 = sets_rt(rtx, oracle, tmp_path, "one", None)[0]
    assert rt1.sky_sets == 1 and not rt1.environment_active
    rt1.set_environment(img, layout, E.SCALES[name])
    assert rt1.environment_active
    got = read_tables(rt1)
    rt1.cleanup()
    assert_tables(got, table, pdf, cdf, s, "host setter, one set")
    rt2 = sets_rt(rtx, oracle, tmp_path, "two", 2)[0]
    assert rt2.sky_sets == 2
    d = to_dev(img)
    rt2.set_environment_device(d, img.shape[1], img.shape[0], fmt_of(rtx, img), layout, E.SCALES[name])
    assert rt2.environment_active
    got = read_tables(rt2)
    assert_tables(got, table, pdf, cdf, s, "device setter")
    rt2.reset_environment()
    assert np.array_equal(bits(rt2.get_buffer("SKY", (256, 512, 4), np.float32)), bits(s["sky"]))
    rt2.set_environment(img, layout, E.SCALES[name])
    got = read_tables(rt2)
    rt2.cleanup()
    assert_tables(got, table, pdf, cdf, s, "host setter, two sets")


def pitched_up(rtx, oracle):
    return terrain_camera(rtx, oracle, W, H, pos=(8.0, 6.0, -6.0), pitch=0.35)


@pytest.mark.parametrize("name,override,up", [
    ("latlong_2048x1024_f16", -1, False), ("latlong_2048x1024_f16", -1, True), ("table_f32", 5, False),
    ("latlong_1000x500_f32", -1, True), ("bright_texel", -1, False), ("zeros", -1, False)],
    ids=["f16-terrain", "f16-sky", "table-mirror", "f32-sky", "bright", "zeros"])
def test_frames_against_the_oracle(rtx, oracle, tmp_path, default_scene, name, override, up):
    """Frame 1 at spp 1 and frame 3 at spp 4 under an environment against the oracle fed the same table
    and CDF: the terrain camera and one pitched up so that most pixels are sky, the mirror override whose
    inline bounces read the table, one bright texel and the all-zero table (every light sample the sun's)."""
    img, layout = E.source(name)
    table, pdf, cdf = tables(rtx, oracle, name)
    sky_out = dict(oracle.sky(), sky=table, sky_cdf=cdf)
    tex = oracle.textures()
    extra = "materialOverride = %d\n" % override if override >= 0 else ""
    for frame, spp in ((1, 1), (3, 4)):
        rt, ocam = terrain_rt(rtx, oracle, tmp_path, "f%d" % frame, spp=spp, extra=extra)
        if up:
            ocam, rcam = pitched_up(rtx, oracle)
            rt.camera = rcam
        rt.set_environment(img, layout, E.SCALES[name])
        g = trace(rt, frame)
        rt.cleanup()
        o = oracle.pathtrace(default_scene["bvh"], W, H, frame_num=frame, spp=spp, cam=ocam, sky_out=sky_out, tex=tex,
                             material_override=override)
        assert_gbuffers_equal(g, o)
        if up:  # most pixels are sky (depth 0x7C00)
            assert float((g["depth"] == 0x7C00).mean()) > 0.5


def test_identity_and_reset(rtx, oracle, tmp_path):
    """The downloaded Hosek table set as a TABLE environment at scale 1 renders the frames of no
    environment, and so does the context after rt_reset_environment; on one set and on two."""
    for sets in (None, 2):
        rt, _ = sets_rt(rtx, oracle, tmp_path, "id%s" % sets, sets, spp=2)
        plain = [trace(rt, f) for f in (1, 3)]
        hosek = rt.get_buffer("SKY", (256, 512, 4), np.float32)
        cdf = rt.download("SKY_CDF", np.float32)
        assert np.isfinite(hosek).all() and hosek.min() >= 0 and hosek.max() < 65504.0
        rt.set_environment(hosek, rtx.ENV_LAYOUT_TABLE, 1.0)
        assert rt.environment_active
        assert np.array_equal(rt.get_buffer("SKY", (256, 512, 4), np.float32), hosek)
        assert np.array_equal(bits(rt.download("SKY_CDF", np.float32)), bits(cdf))
        under = [trace(rt, f) for f in (1, 3)]
        rt.reset_environment()
        assert not rt.environment_active
        assert np.array_equal(bits(rt.get_buffer("SKY", (256, 512, 4), np.float32)), bits(hosek))
        after = [trace(rt, f) for f in (1, 3)]
        rt.reset_environment()  # nothing to reset: still fine
        rt.cleanup()
        for a, b, c in zip(plain, under, after):
            assert_gbuffers_equal(b, a)
            assert_gbuffers_equal(c, a)


def test_sky_parameters_under_an_environment(rtx, oracle, tmp_path, default_scene):
    """timeOfDay and sunScalar change while an environment is active: the sun arrays follow
    oracle.sky(params), the sky table stays the environment's, and the frame matches the oracle."""
    name = "latlong_1000x500_f32"
    img, layout = E.source(name)
    table, pdf, cdf = tables(rtx, oracle, name)
    tex = oracle.textures()
    for sets in (None, 2):
        rt, ocam = sets_rt(rtx, oracle, tmp_path, "sp%s" % sets, sets, spp=2)
        rt.set_environment(img, layout, E.SCALES[name])
        trace(rt, 1)
        p = rt.params
        p.sky.timeOfDay = 0.31
        p.sky.sunScalar = p.sky.sunScalar * 2
        rt.params = p
        g = trace(rt, 2)
        assert rt.environment_active
        got = read_tables(rt)
        rt.cleanup()
        s = oracle.sky(dict(timeOfDay=float(np.float32(0.31)), sunScalar=float(np.float32(oracle.SKY_DEFAULTS["sunScalar"]) * 2)))
        assert not np.array_equal(bits(s["sun"]), bits(oracle.sky()["sun"]))
        assert_tables(got, table, pdf, cdf, s, "sets %s" % sets)
        o = oracle.pathtrace(default_scene["bvh"], W, H, frame_num=2, spp=2, cam=ocam, sky_out=dict(s, sky=table, sky_cdf=cdf),
                             tex=tex)
        assert_gbuffers_equal(g, o)


def test_full_draw_under_an_environment(rtx, oracle, tmp_path, default_scene):
    """Three rt_draw frames under an environment against the oracle's draw: RGBA8 and HDR."""
    name = "latlong_2048x1024_f16"
    img, layout = E.source(name)
    table, pdf, cdf = tables(rtx, oracle, name)
    sky_out = dict(oracle.sky(), sky=table, sky_cdf=cdf)
    tex = oracle.textures()
    rt, ocam = sets_rt(rtx, oracle, tmp_path, "draw", 2, spp=2)
    rt.set_delta_time(DT)
    rt.set_environment(img, layout, E.SCALES[name])
    dn = oracle.Denoiser(W, H)
    frames = []
    for f in (1, 2, 3):
        rgba = np.zeros((H, W, 4), np.uint8)
        hdr = np.zeros((H, W, 4), np.float32)
        rt.draw(rgba, hdr)
        frames.append((rgba, hdr.view(np.uint32)))
    errors = int(rt.download("PT_QUEUE", np.uint32)[10])
    rt.cleanup()
    assert errors == 0
    for f, (rgba, hdr) in zip((1, 2, 3), frames):
        gb = oracle.pathtrace(default_scene["bvh"], W, H, frame_num=f, spp=2, cam=ocam, hist_cam=ocam, sky_out=sky_out, tex=tex)
        o = dn.draw(gb, f, delta_time=DT)
        ref = o["color"][:, :3].view(np.float16).astype(np.float32).view(np.uint32)
        assert np.array_equal(hdr.reshape(-1, 4)[:, :3], ref), "HDR of frame %d" % f
        assert np.array_equal(rgba.reshape(-1, 4), o["rgba"]), "RGBA8 of frame %d" % f
