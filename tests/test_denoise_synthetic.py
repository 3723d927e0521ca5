"""The synthetic denoise / post inputs (tests/denoise_inputs.py) on the CPU oracle: the conditions
that make each case of tests/test_gpu_denoise_synthetic.py mean something, computed from the
oracle's outputs and from the arrays, and the anchor that does not depend on the oracle's
arithmetic.

Anchor: the uniform family (colour (0.75, 0.5, 0.25), albedo 0.5, depth 5, normal +y, motion zero
or a uniform sub-pixel shift).  Every pass is a normalised weighted mean and every product is exact
in half, so RENDER_COLOR is exactly (0.375, 0.25, 0.125), the accumulation exactly the colour, and
the histogram has one non-zero bin whose count is W64 * H64, in every frame and at every size.
"""
import math

import numpy as np
import pytest

import denoise_inputs as D

DT = 16.667
INT_MAX, INT_MIN = 2 ** 31 - 1, -2 ** 31
ANCHOR_COLOR = np.array([0.375, 0.25, 0.125], np.float16).view(np.uint16)  # BASE * albedo 0.5
ANCHOR_ACCUM = np.array(D.BASE, np.float16).view(np.uint16)


def sequence(oracle, family, w, h, frames, params=None, ws=None, hs=None):
    """[(input arrays, oracle outputs, accumulation after the frame)] of `frames` frames."""
    dn = oracle.Denoiser(w, h, ws, hs)
    out = []
    for f in range(1, frames + 1):
        g = D.FAMILIES[family](w, h, f)
        o = dn.draw(g, f, params=params, delta_time=DT)
        out.append((g, o, dn.accum.copy()))
    return out


def level64(w, h):
    d = lambda n: (n + 3) // 4
    return d(d(d(w))) * d(d(d(h)))


# ---------------------------------------------------------------- the oracle's float -> int conversion
@pytest.mark.parametrize("x, want", [
    (float("nan"), 0), (float("inf"), INT_MAX), (-float("inf"), INT_MIN), (2.0 ** 31, INT_MAX), (-2.0 ** 31, INT_MIN),
    (2.0 ** 31 - 128, 2 ** 31 - 128), (-(2.0 ** 31 - 128), -(2 ** 31 - 128)), (-0.0, 0), (2.0 ** 32, INT_MAX),
    (-3.0e38, INT_MIN), (2.9, 2), (-2.9, -2), (-0.9, 0), (16777215.0, 16777215)])
def test_oracle_float_to_int_is_cvt_rzi(oracle, x, want):
    """ocommon.h f2i restates cvt.rzi.s32.f32 (and v_cvt_i32_f32): truncate, saturate, NaN -> 0,
    where the host's plain cast gives INT_MIN for every one of the special values."""
    assert oracle.f2i(x) == want


# ---------------------------------------------------------------- the generators themselves
@pytest.mark.parametrize("size", [(1, 1), (9, 17), (40, 24)])
@pytest.mark.parametrize("family", list(D.FAMILIES))
def test_family_layout_and_description(family, size):
    w, h = size
    fam = D.FAMILIES[family]
    assert fam.describe().startswith(family + ": ") and len(fam.describe()) > len(family) + 10
    g = fam(w, h, 2)
    shapes = dict(color=(w * h, 4), normal=(w * h, 4), albedo=(w * h, 4), depth=(w * h,), motion=(w * h, 2))
    assert set(g) == set(shapes)
    for k, s in shapes.items():
        assert g[k].dtype == np.uint16 and g[k].shape == s and g[k].flags.c_contiguous, (fam.describe(), k)
    again = fam(w, h, 2)
    assert all(np.array_equal(g[k], again[k]) for k in g), fam.describe()  # seeded


@pytest.mark.parametrize("size", D.VALUE_SIZES)
def test_value_classes_are_in_the_arrays(size):
    """Each value family holds the classes its description names, at both sizes the GPU runs."""
    w, h = size
    c = D.FAMILIES["color-values"](w, h, 2)["color"].reshape(h, w, 4)
    for name, bits in D.COLOR_SPECIALS:
        hit = (c[:, :, :3] == bits).all(axis=2)
        assert hit.any(), name
        tiles = [hit[y:y + 8, x:x + 8].all() for y in range(0, h - 7, 8) for x in range(0, w - 7, 8)]
        assert any(tiles), "no whole 8x8 tile of " + name
        assert ((c[:, :, :3] == bits).sum(axis=2) == 1).any(), "no single channel of " + name
        assert hit[15, :].any() and hit[:, 16].any(), "not on the tile edge: " + name
    d = D.FAMILIES["depth"](w, h, 2)["depth"].reshape(h, w)
    sky = d == D.SKY
    frac = {float(sky[y:y + 8, x:x + 8].mean()) for y in range(0, h - 7, 8) for x in range(0, w - 7, 8)}
    assert {0.0, 0.5, 1.0} <= frac, frac  # the notSky fractions of whole tiles
    assert (d == 0).any() and all((d == k).any() for k in range(1, 8))  # zero, steps of one subnormal half
    assert (D.FAMILIES["depth-sky"](w, h, 2)["depth"] == D.SKY).all()
    n = D.unhalf(D.FAMILIES["normals"](w, h, 2)["normal"][:, :3])
    ln = np.linalg.norm(n, axis=1)
    assert (ln == 0).any() and (ln > 1.5).any() and ((ln > 0) & (ln < 0.5)).any() and np.isnan(ln).any()
    nn = n.reshape(h, w, 3)
    assert ((nn[:, 1:, 1] == -nn[:, :-1, 1]) & (np.abs(nn[:, 1:, 1]) == 1)).any()  # opposite neighbours
    a = D.unhalf(D.FAMILIES["albedo"](w, h, 2)["albedo"][:, :3])
    assert (a == 0).all(axis=1).any() and (a > 1).any() and np.isinf(a).any() and np.isnan(a).any()
    m = D.FAMILIES["masks"](w, h, 2)["color"][:, 3].reshape(h, w)
    assert {0, 0xFFFF} <= set(np.unique(m).tolist())
    inner = m[:, 1:] != m[:, :-1]
    assert inner[:, [x for x in range(w - 1) if x % 16 not in (15,)]].any()  # an edge inside a tile
    mw = D.FAMILIES["motion-wild"](w, h, 2)["motion"]
    for name, bits in D.MOTION_WILD:
        assert (mw == bits).any(), name


# ---------------------------------------------------------------- anchor
@pytest.mark.parametrize("size", D.ANCHOR_SIZES, ids=lambda s: "%dx%d-%sx%s" % s)
@pytest.mark.parametrize("family", ["uniform", "uniform-shift"])
def test_anchor_on_the_oracle(oracle, family, size):
    w, h, ws, hs = size
    for f, (g, o, accum) in enumerate(sequence(oracle, family, w, h, 5, ws=ws, hs=hs), start=1):
        what = (D.FAMILIES[family].describe(), size, f)
        assert (o["color"][:, :3] == ANCHOR_COLOR).all(), what
        assert (accum[:, :3] == ANCHOR_ACCUM).all(), what
        assert np.count_nonzero(o["histogram"]) == 1 and o["histogram"].max() == level64(w, h), what
    if family == "uniform-shift":
        mv = D.unhalf(g["motion"]) - np.float32(0.5)
        px = np.abs(mv * np.array([w, h], np.float32))
        assert (px > 0).all() and (px < 1).all(), px.max()  # a shift, and sub-pixel


# ---------------------------------------------------------------- regions and the thresholds
def noise16(o):
    return o["noise16"].view(np.float16).astype(np.float32)


@pytest.mark.parametrize("size", D.VALUE_SIZES)
@pytest.mark.parametrize("order", ["local>large", "large>local"])
def test_regions_reach_all_three_threshold_classes(oracle, order, size):
    """With unequal thresholds, frames 2 and 3 have a tile at or above the higher one, a tile between
    the two and a tile below the lower one: local > large reaches TemporalFilter's append to list 1
    of a tile SpatialFilter7x7 skips, large > local a filtered tile that stays off list 1."""
    w, h = size
    p = oracle.default_params()
    p.noise_threshold_local, p.noise_threshold_large = D.THRESHOLDS[order]
    seq = sequence(oracle, "regions", w, h, 3, params=p)
    for f in (2, 3):
        n = noise16(seq[f - 1][1])
        top, mid, low = n >= D.THRESHOLD_HI, (n >= D.THRESHOLD_LO) & (n < D.THRESHOLD_HI), n < D.THRESHOLD_LO
        assert top.any() and mid.any() and low.any(), (D.FAMILIES["regions"].describe(), order, size, f, np.sort(n))


@pytest.mark.parametrize("size", D.SIZES, ids=lambda s: "%dx%d" % s)
def test_regions_flat_third_stays_off_the_lists(oracle, size):
    """Under the default thresholds every 16x16 tile wholly inside the flat third is below them in
    every frame, and from 40x24 on frames 2 and 3 also have tiles above them."""
    w, h = size
    thr = oracle.default_params().noise_threshold_local
    assert thr == oracle.default_params().noise_threshold_large
    W16 = (w + 15) // 16
    flat = D.region_of(w, h)[0] == 2
    inside = np.array([flat[tx * 16:min(w, tx * 16 + 16)].all() for tx in range(W16)])
    for f, (_, o, _) in enumerate(sequence(oracle, "regions", w, h, 3), start=1):
        n = noise16(o).reshape(-1, W16)
        assert (n[:, inside] < thr).all(), (size, f, n)
        if w >= 40 and f > 1:
            assert inside.any() and (n >= thr).any(), (size, f, n)


@pytest.mark.parametrize("size", D.VALUE_SIZES)
@pytest.mark.parametrize("name", ["zero", "inf", "nan"])
def test_extreme_thresholds_take_all_or_no_tiles(oracle, name, size):
    """`!(n16 < thr)` over the regions family's finite noise levels: every tile with thresholds 0
    (both lists at capacity) or NaN (the comparison is false), none with +inf."""
    w, h = size
    p = oracle.default_params()
    p.noise_threshold_local, p.noise_threshold_large = D.THRESHOLDS[name]
    for f, (_, o, _) in enumerate(sequence(oracle, "regions", w, h, 3, params=p), start=1):
        n = noise16(o)
        assert np.isfinite(n).all(), (name, size, f)
        on = ~(n < np.float32(p.noise_threshold_large))
        assert on.all() if name in ("zero", "nan") else not on.any(), (name, size, f)
    if name == "zero":  # more tiles than list partitions at 150x86: several entries in each
        assert (n.size > 16) == (size == (150, 86))


# ---------------------------------------------------------------- reprojection
@pytest.mark.parametrize("size", D.VALUE_SIZES)
@pytest.mark.parametrize("family", [k for k in D.FAMILIES if k not in D.OUT_OF_FRAME])
def test_history_is_read(family, size):
    """At least half the pixels of every case but the out-of-frame ones reproject inside the frame.
    (A motion array of zero bits is mv = -0.5, which never reads the history: no family is that.)"""
    w, h = size
    for f in (1, 2, 3):
        g = D.FAMILIES[family](w, h, f)
        assert g["motion"].any(), D.FAMILIES[family].describe()
        u = D.huv_of(g["motion"], w, h)
        inside = ((u >= 0) & (u <= 1)).all(axis=1)
        assert inside.mean() >= 0.5, (D.FAMILIES[family].describe(), size, f, inside.mean())


@pytest.mark.parametrize("size", D.VALUE_SIZES)
def test_out_of_frame_family_has_every_kind(size):
    w, h = size
    g = D.FAMILIES["motion-wild"](w, h, 2)
    u = D.huv_of(g["motion"], w, h)
    assert np.isnan(u).any() and np.isposinf(u).any() and np.isneginf(u).any()
    assert (u[np.isfinite(u)] > 2).any() and (u[np.isfinite(u)] < -1).any()
    inside = ((u >= 0) & (u <= 1)).all(axis=1)
    assert 0.25 <= inside.mean() <= 0.9  # the in-frame neighbours of the wild pixels still read it
    # a NaN coordinate passes the out-of-frame test (every comparison is false): the history is read
    assert (D.huv_inside(g["motion"], w, h) & np.isnan(u).any(axis=1)).any()


@pytest.mark.parametrize("size", D.VALUE_SIZES)
def test_border_motion_hits_both_sides_exactly(size):
    """huv exactly 0.0 and exactly 1.0 (history read: `huv.x < 0 || ... > 1.0f` is false), and at the
    border pixels the nearest stored motion inside and outside the frame, in x and in y."""
    w, h = size
    g = D.FAMILIES["motion-border"](w, h, 2)
    u = D.huv_of(g["motion"], w, h).reshape(h, w, 2)
    read = D.huv_inside(g["motion"], w, h).reshape(h, w)
    for axis in (0, 1):
        assert ((u[..., axis] == 0.0) & read).any() and ((u[..., axis] == 1.0) & read).any(), (size, axis)
    for line, vals in ((u[:, 0, 0], "x0"), (u[:, w - 1, 0], "x1"), (u[0, :, 1], "y0"), (u[h - 1, :, 1], "y1")):
        lo = vals in ("x0", "y0")
        inside = (line >= 0) & (line <= 1)
        assert inside.any() and (~inside).any(), (size, vals)
        # one stored step from the edge: within a pixel of it
        edge = 0.0 if lo else 1.0
        assert np.abs(line - edge).max() <= 1.0 / min(w, h), (size, vals, line)


@pytest.mark.parametrize("size", D.VALUE_SIZES)
def test_moving_masks_take_every_discard_fraction(oracle, size):
    """The accumulation buffer carries each frame's masks unchanged, so the four history texels of a
    pixel hold the previous frame's pattern: 0, 1/4, 1/2, 3/4 and 1 of them differ, each somewhere,
    in frames 2 and 3."""
    w, h = size
    seq = sequence(oracle, "masks", w, h, 3)
    for f in (2, 3):
        g, _, _ = seq[f - 1]
        prev_in, _, prev_accum = seq[f - 2]
        assert np.array_equal(prev_accum[:, 3], prev_in["color"][:, 3]), f
        fr = D.discard_fractions(g["color"][:, 3], prev_accum[:, 3], g["motion"], w, h)
        assert set(np.unique(fr).tolist()) == {0.0, 0.25, 0.5, 0.75, 1.0}, (size, f, np.unique(fr))


# ---------------------------------------------------------------- the scale kernel's read paths
@pytest.mark.parametrize("case", list(D.SCALES), ids=lambda c: "%dx%d-%dx%d" % c)
def test_scale_cases_take_the_stated_branch(case):
    """Each render -> screen ratio takes the k_scale_post path its GPU case states (the host's tile
    choice and the kernel's footprint test, restated in denoise_inputs.scale_branches)."""
    assert D.scale_branches(*case) == D.SCALES[case]


def test_scale_boundary_is_18_over_17():
    """36 -> 34 is the last ratio that picks the small LDS tile (17 * 36 + 5 * 34 = 782 = 24 * 34 - 34)
    and 37 -> 34 the first that does not; the ratios the path-traced tests run take the small tile
    (1.0, 0.8) or the large one staged (1.2): none of them reads unstaged."""
    assert 17 * 36 + 5 * 34 == 24 * 34 - 34
    assert D.scale_branches(36, 18, 34, 17)[0] == "small" and D.scale_branches(37, 18, 34, 17)[0] == "large"
    assert D.scale_branches(160, 96, 160, 96) == ("small", "staged")
    assert D.scale_branches(128, 72, 160, 90) == ("small", "staged")
    assert D.scale_branches(192, 108, 160, 90) == ("large", "staged")
    assert math.isclose(36 / 34, 18 / 17)


# ---------------------------------------------------------------- DESIGN.md §5 deviation 3
@pytest.mark.parametrize("size", D.VALUE_SIZES)
def test_nan_colour_is_left_unchanged_by_the_oracle(oracle, size):
    """A pixel whose own colour is NaN is left unchanged by TemporalFilter and SpatialFilter7x7: with
    the a-trous passes and TemporalFilter2 off the accumulation keeps its input bits, and
    RENDER_COLOR is NaN exactly in the channels that were."""
    w, h = size
    p = oracle.default_params()
    p.enableWideSpatialFilter = p.enableTemporalDenoising2 = 0
    for f, (g, o, accum) in enumerate(sequence(oracle, "color-values", w, h, 3, params=p), start=1):
        c = g["color"]
        nan = np.isnan(c[:, :3].view(np.float16)).any(axis=1)
        assert nan.sum() >= 64
        assert np.array_equal(accum[nan], c[nan]), f
        assert np.array_equal(np.isnan(o["color"][nan][:, :3].view(np.float16)),
                              np.isnan(c[nan][:, :3].view(np.float16))), f
