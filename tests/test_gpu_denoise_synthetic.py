"""GPU denoiser + post chain on synthetic G-buffers (tests/denoise_inputs.py), bit for bit against
the oracle and, for the uniform family, against constants that do not come from the oracle.

Every other denoise test feeds the stage what the path tracer produced: frames of at least 64x36,
render : screen ratios of 0.8, 1.0 and 1.2, both noise thresholds at the default.  Here the five
G-buffers of set 0 are caller memory (rt_bind_buffer) filled from seeded arrays, and
rt_denoise_post runs on them directly (it needs rt_init only), so the cases reach

- frames below one 8x8, 16x16 and 64x64 unit, and sizes that are no multiple of any of them;
- unequal, zero, infinite and NaN noise thresholds: TemporalFilter's append to list 1 of a tile that
  SpatialFilter7x7 skips (`else if (act5) list_append(P, 1, tile)`), a filtered tile that stays off
  list 1, both lists at capacity, both empty;
- value classes the path tracer never emits (the families of denoise_inputs.py);
- every read path of k_scale_post (the small LDS tile, the large one, unstaged reads, up-scaling).

tests/test_denoise_synthetic.py asserts on the CPU, from the oracle's outputs and the arrays, that
each case reaches what it is meant to reach.  Every case makes its own context (under 0.1 s at
these sizes), so no state passes from case to case; three frames each: frame 1 takes the
non-temporal path, frames 2 and 3 the list chain on both tile-list parities.

Where the reference decides a case.

- Motion of +Inf.  The reference's TemporalFilter2 returns at its out-of-frame test
  (temporalDenoising.cuh:1022) before it samples the history (:1028, :1053); the product's
  temporal2_pixel issues the history loads for every pixel and selects afterwards.  At huv = +Inf the
  footprint's first texel converts to INT_MAX, the second texel's `+ 1` overflowed, and the compiled
  clamp let INT_MIN through: an illegal address, found by the motion-wild family.  The GPU side was
  wrong; off screen it now reads at the pixel's own position.
- A NaN motion vector passes that test (every comparison is false), in the reference too
  (temporalDenoising.cuh:805, :1022), and the history is read at texel (int)NaN.  The reference's
  conversions are cvt.rzi.s32.f32 (NaN -> 0, saturating), as v_cvt_i32_f32; the oracle's plain casts
  gave INT_MIN on the host and now go through ocommon.h f2i.  No output can tell the two apart today:
  the blend of a NaN coordinate is NaN, which both passes store as black, and ApplyAlbedo has set
  every mask TemporalFilter2 compares to half(1.0).  The helper is pinned directly
  (test_denoise_synthetic.py) instead.
- A NaN colour: the reference returns before a barrier and leaves LDS undefined, so DESIGN.md §5
  deviation 3 is the expectation: the pixel is left unchanged by TemporalFilter and SpatialFilter7x7
  (test_nan_colour_is_left_unchanged).

No class of the families is left out.
"""
import numpy as np
import pytest

import denoise_inputs as D
from test_gpu_denoise import assert_state, gpu_state
from test_gpu_denoise_variants import SIGMAS, TUNINGS, tweak

pytestmark = pytest.mark.gpu

DT = 16.667
FRAMES = 3
GBUFFERS = (("RENDER_COLOR", "color"), ("NORMAL", "normal"), ("ALBEDO", "albedo"), ("DEPTH", "depth"),
            ("MOTION", "motion"))
PASS_SWITCHES = ("enableWideSpatialFilter", "enableLocalSpatialFilter", "enableTemporalDenoising",
                 "enableTemporalDenoising2", "enableDownScalePasses")


class Context:
    """A renderer at render size (w, h) whose set-0 G-buffers are torch tensors."""

    def __init__(self, rtx, tmp_path, w, h, ws, hs, tuning):
        import torch

        path = str(tmp_path / "synthetic.toml")
        if ws is None:
            self.rt = rtx.RayTracer(w, h, rtx.write_config(path, w, h, extra=TUNINGS[tuning])).init()
        else:  # a context made this way starts at its maximum render size, and rt_denoise_post never resizes
            cfg = rtx.write_config(path, ws, hs, dynamic=True, max_size=(w, h), min_size=(w, h), extra=TUNINGS[tuning])
            self.rt = rtx.RayTracer(ws, hs, cfg).init()
        info = self.rt.info()
        assert (info.renderWidth, info.renderHeight) == (w, h)
        assert (info.screenWidth, info.screenHeight) == (ws or w, hs or h)
        self.bufs = {}
        for name, _ in GBUFFERS:
            t = torch.zeros(self.rt.buffer_bytes(name), dtype=torch.uint8, device="cuda:0")
            self.rt.bind_buffer(name, t.data_ptr(), t.numel())
            self.bufs[name] = t
        torch.cuda.synchronize()

    def upload(self, arrays):
        import torch

        for name, key in GBUFFERS:
            host = torch.from_numpy(arrays[key].reshape(-1).view(np.uint8).copy())
            assert host.numel() == self.bufs[name].numel(), name
            self.bufs[name].copy_(host)
        torch.cuda.synchronize()

    def close(self):
        self.rt.sync()
        self.rt.cleanup()
        self.bufs = {}


def frames_of(rtx, oracle, tmp_path, family, w, h, ws=None, hs=None, tuning="default", params_fn=None, frames=FRAMES):
    """Run `frames` frames of the family on a new context and on the oracle; yields (frame, input
    arrays, GPU state, oracle outputs, oracle Denoiser) after each."""
    c = None
    try:
        c = Context(rtx, tmp_path, w, h, ws, hs, tuning)
        rt = c.rt
        p, op = rt.params, oracle.default_params()
        if params_fn:
            params_fn(p, op)
        rt.params = p
        rt.set_delta_time(DT)
        dn = oracle.Denoiser(w, h, ws, hs)
        for f in range(1, frames + 1):
            arrays = D.FAMILIES[family](w, h, f)
            c.upload(arrays)  # all five every frame: the colour buffer is the chain's ping-pong
            rt.denoise_post(f)
            rt.sync()
            g = gpu_state(rt, w, h, ws or w, hs or h)
            o = dn.draw(arrays, f, params=op, delta_time=DT)
            yield f, arrays, g, o, dn
        c.close()
    except BaseException as e:
        if isinstance(e, rtx.RtError) and "RT_ERR_HIP" in str(e):  # a device error: nothing more may be launched on it
            pytest.exit("device error in %s at %dx%d: %s" % (family, w, h, e), returncode=3)
        if c is not None:
            c.close()
        raise


def check(rtx, oracle, tmp_path, family, w, h, **kw):
    """The case bit for bit against the oracle: colour, accumulation, both histories, both noise
    grids, the DownScale4 levels, histogram, exposure, scaled image and RGBA8."""
    for f, _, g, o, dn in frames_of(rtx, oracle, tmp_path, family, w, h, **kw):
        try:
            assert_state(g, o, dn)
        except AssertionError as e:
            raise AssertionError("%s; %dx%d %s frame %d: %s" % (D.FAMILIES[family].describe(), w, h, kw, f, e)) from None


def thresholds(name):
    local, large = D.THRESHOLDS[name]

    def fn(p, op):
        p.denoise.noise_threshold_local = op.noise_threshold_local = local
        p.denoise.noise_threshold_large = op.noise_threshold_large = large
    return fn


# ---------------------------------------------------------------- anchor: no oracle
@pytest.mark.parametrize("size", D.ANCHOR_SIZES, ids=lambda s: "%dx%d-%sx%s" % s)
@pytest.mark.parametrize("family", ["uniform", "uniform-shift"])
def test_anchor_constants(rtx, oracle, tmp_path, family, size):
    """Uniform colour (0.75, 0.5, 0.25), albedo 0.5, depth 5, normal +y, motion zero or a uniform
    sub-pixel shift: every pass is a normalised weighted mean and every product is exact in half,
    so for frames 1..5 RENDER_COLOR is exactly (0.375, 0.25, 0.125), the accumulation exactly the
    colour, and the histogram has one non-zero bin whose count is W64 * H64.  Asserted of the GPU
    from these constants; 48x27 -> 32x18 and 33x19 -> 64x36 also resample."""
    w, h, ws, hs = size
    d = lambda n: (n + 3) // 4
    color = np.array([0.375, 0.25, 0.125], np.float16).view(np.uint16)
    accum = np.array(D.BASE, np.float16).view(np.uint16)
    for f, _, g, _, _ in frames_of(rtx, oracle, tmp_path, family, w, h, ws=ws, hs=hs, frames=5):
        what = (D.FAMILIES[family].describe(), size, f)
        assert (g["color"][:, :3] == color).all(), what
        assert (g["accum"] == np.append(accum, 1)).all(), what  # and the mask
        assert (g["hist_color"][:, :3] == color).all(), what
        assert (g["hist_depth"] == D.half(5.0)).all(), what
        assert np.count_nonzero(g["histogram"]) == 1 and g["histogram"].max() == d(d(d(w))) * d(d(d(h))), what
        assert (g["noise16"] == 0).all() and (g["noise8"] == 0).all(), what
        assert (g["scaled"] == g["scaled"][0]).all() and (g["rgba"][:, 3] == 1).all(), what


# ---------------------------------------------------------------- sizes
@pytest.mark.parametrize("size", D.SIZES, ids=lambda s: "%dx%d" % s)
@pytest.mark.parametrize("family", ["regions", "uniform"])
def test_sizes(rtx, oracle, tmp_path, family, size):
    """From one pixel up: below one 8x8 noise tile (1x1, 3x5, 7x7), exactly one (8x8), below and at
    one 16x16 list tile (9x17, 16x16, 17x9), 40x24, one 64-block crossed in x (65x33), and 150x86
    (60 tiles: several entries in each of the 16 list partitions, no multiple of 16)."""
    check(rtx, oracle, tmp_path, family, *size)


# ---------------------------------------------------------------- thresholds
@pytest.mark.parametrize("size", D.VALUE_SIZES, ids=lambda s: "%dx%d" % s)
@pytest.mark.parametrize("tuning", ["default", "fold", "split"])
@pytest.mark.parametrize("name", list(D.THRESHOLDS))
def test_thresholds(rtx, oracle, tmp_path, name, tuning, size):
    """noise_threshold_local / _large unequal in both orders (the regions family has tiles in all
    three classes at frames 2 and 3), both 0 (every tile on both lists), both +inf (none) and NaN
    (`!(n16 < thr)`: every tile), in the default, folded and two-threads-per-pixel list chains."""
    check(rtx, oracle, tmp_path, "regions", *size, tuning=tuning, params_fn=thresholds(name))


# ---------------------------------------------------------------- value families
@pytest.mark.parametrize("size", D.VALUE_SIZES, ids=lambda s: "%dx%d" % s)
@pytest.mark.parametrize("family", D.VALUE_FAMILIES)
def test_value_families(rtx, oracle, tmp_path, family, size):
    check(rtx, oracle, tmp_path, family, *size)


@pytest.mark.parametrize("size", D.VALUE_SIZES, ids=lambda s: "%dx%d" % s)
@pytest.mark.parametrize("sigma", list(SIGMAS))
@pytest.mark.parametrize("family", ["depth", "depth-sky", "normals"])
def test_depth_and_normal_families_without_rcp_and_pairs(rtx, oracle, tmp_path, family, sigma, size):
    """kRcp off (the depth ratio as a division) and kPk off (scalar normal weights) on zero, subnormal
    and sky depths and on zero, long, opposite and NaN normals."""
    check(rtx, oracle, tmp_path, family, *size, params_fn=tweak(SIGMAS[sigma]))


@pytest.mark.parametrize("size", D.VALUE_SIZES, ids=lambda s: "%dx%d" % s)
@pytest.mark.parametrize("off", PASS_SWITCHES)
def test_pass_switches(rtx, oracle, tmp_path, off, size):
    """The frame-wide kernels (one of the three filters off) and the tails without TemporalFilter2 or
    the downscale passes, on the regions family."""
    check(rtx, oracle, tmp_path, "regions", *size, params_fn=tweak(**{off: 0}))


@pytest.mark.parametrize("size", D.VALUE_SIZES, ids=lambda s: "%dx%d" % s)
def test_nan_colour_is_left_unchanged(rtx, oracle, tmp_path, size):
    """DESIGN.md §5 deviation 3: a pixel whose own colour is NaN is left unchanged by TemporalFilter
    and SpatialFilter7x7 (the reference returns before a barrier there and leaves LDS undefined).
    With the a-trous passes and TemporalFilter2 off, what reaches RENDER_COLOR of such a pixel is its
    input times the albedo: NaN where a channel was NaN, and the accumulation keeps the input bits."""
    w, h = size
    fn = tweak(enableWideSpatialFilter=0, enableTemporalDenoising2=0)
    for f, arrays, g, o, dn in frames_of(rtx, oracle, tmp_path, "color-values", w, h, params_fn=fn):
        c = arrays["color"]
        nan = np.isnan(c[:, :3].view(np.float16)).any(axis=1)
        assert nan.sum() >= 64
        assert np.array_equal(g["accum"][nan], c[nan]), f
        cin = np.isnan(c[nan][:, :3].view(np.float16))
        assert np.array_equal(np.isnan(g["color"][nan][:, :3].view(np.float16)), cin), f
        assert_state(g, o, dn)


# ---------------------------------------------------------------- scale ratios
@pytest.mark.parametrize("case", list(D.SCALES), ids=lambda c: "%dx%d-%dx%d" % c)
def test_scale_ratios(rtx, oracle, tmp_path, case):
    """render -> screen, and the k_scale_post path each takes (scale_lds_small on the host, the
    footprint TW * TH against the LDS tile in the kernel; tests/test_denoise_synthetic.py derives
    the same from denoise_inputs.scale_branches):

    36x18 -> 34x17   17 * 36 + 5 * 34 = 782 = 24 * 34 - 34: the last ratio with the small tile; staged
    37x18 -> 34x17   the first ratio without it: the large tile, staged
    96x54 -> 32x18   ratio 3, large tile: screen tile row 0 covers 50 x 50 > 48 x 48 render texels and
                     reads unstaged, row 1 (two screen rows, 52 x 10) is staged
    36x54 -> 34x18   small in x, 3 in y: the large tile (24 x 56 at most), staged
    16x9  -> 64x36   up-scaling by 4: the small tile, staged
    1x1   -> 16x16   one render texel under a whole screen tile: the small tile, staged
    50x30 -> 33x17   no common factor, ratio ~1.5 and ~1.76: the large tile, staged"""
    w, h, ws, hs = case
    check(rtx, oracle, tmp_path, "regions", w, h, ws=ws, hs=hs)


# ---------------------------------------------------------------- the histogram off
@pytest.mark.parametrize("size", D.VALUE_SIZES, ids=lambda s: "%dx%d" % s)
def test_histogram_off(rtx, oracle, tmp_path, size):
    """enableHistogram = 0, the case test_tail_paths leaves out: three k_downscale4 launches and a
    cleared histogram, on which AutoExposure divides 0 by 0.  Every image matches bit for bit; the
    NaN the exposure state then holds has its sign clear on the GPU and set in the oracle (the
    default NaN of the two instruction sets), so the four exposure floats are compared bit for bit
    where they are not NaN and as "both NaN" where they are."""
    w, h = size
    for f, _, g, o, dn in frames_of(rtx, oracle, tmp_path, "regions", w, h, params_fn=tweak(enableHistogram=0)):
        ge, oe = g["exposure"], o["exposure"]
        nan = np.isnan(oe)
        assert np.array_equal(np.isnan(ge), nan), (f, ge, oe)
        assert np.array_equal(ge.view(np.uint32)[~nan], oe.view(np.uint32)[~nan]), (f, ge, oe)
        assert (g["histogram"] == 0).all()
        assert_state(dict(g, exposure=oe), o, dn)
