"""Synthetic G-buffers for the denoise / post stage: seeded numpy generators, no GPU and no oracle.

Every family is a callable `family(w, h, frame)` that returns the five G-buffer arrays of one frame
in the product's bit layout, as `oracle.pathtrace` returns them:

    color   uint16 (P, 4)   half r, g, b and a ushort material mask
    normal  uint16 (P, 4)   half4
    albedo  uint16 (P, 4)   half4
    depth   uint16 (P,)     half; 0x7C00 (+Inf) is the sky sentinel
    motion  uint16 (P, 2)   half(mv + 0.5): the history is read at uv + mv (denoise.hip temporal_tail)

and has a `describe()` line that the tests quote, so a failure names its input.  The value classes
are the ones the path tracer never emits (non-finite and negative colours, degenerate normals,
zero and subnormal depths, non-finite and out-of-frame motion), on which the kernels' shortcuts
(rgb_mul's +0 sums, rt_div_rcp's depth differences, the rtmath_pk.h selects) rest.
"""
import numpy as np

BASE = (0.75, 0.5, 0.25)  # every product with the albedo 0.5 and every tap sum is exact in half
SKY = 0x7C00
H_ONE = 0x3C00


def half(x):
    """float -> half bit patterns (round to nearest even)."""
    return np.asarray(x, np.float32).astype(np.float16).view(np.uint16)


def unhalf(b):
    """half bit patterns -> float32 (exact)."""
    return np.asarray(b, np.uint16).view(np.float16).astype(np.float32)


def motion_bits(mv):
    """mv (…, 2) in frame fractions -> the stored half(mv + 0.5)."""
    return half(np.asarray(mv, np.float32) + np.float32(0.5))


def huv_of(motion, w, h):
    """The history coordinate TemporalFilter and TemporalFilter2 compute for every pixel, with their
    float32 operations in their order (denoise.hip temporal_tail): (P, 2) float32."""
    mv = unhalf(motion).reshape(h, w, 2) - np.float32(0.5)
    inv = np.float32(1.0) / np.array([w, h], np.float32)
    x = (np.arange(w, dtype=np.float32) + np.float32(0.5)) * inv[0]
    y = (np.arange(h, dtype=np.float32) + np.float32(0.5)) * inv[1]
    uv = np.stack(np.broadcast_arrays(x[None, :], y[:, None]), axis=-1).astype(np.float32)
    return (uv + mv).astype(np.float32).reshape(-1, 2)


def huv_inside(motion, w, h):
    """Per pixel: the history is read (the `huv.x < 0 || ... > 1.0f` test fails; a NaN passes it)."""
    u = huv_of(motion, w, h)
    return ~((u[:, 0] < 0) | (u[:, 1] < 0) | (u[:, 0] > 1) | (u[:, 1] > 1))


def discard_fractions(mask_now, mask_hist, motion, w, h):
    """The four-texel history discard of every pixel whose history is read: the fraction of the
    texels (hx + i, hy + j), i, j in {0, 1}, clamped, whose mask differs from the pixel's."""
    u = huv_of(motion, w, h)
    ok = huv_inside(motion, w, h) & ~np.isnan(u).any(axis=1)
    hx = np.floor(u[:, 0] * np.float32(w)).astype(np.int64)
    hy = np.floor(u[:, 1] * np.float32(h)).astype(np.int64)
    mh = mask_hist.reshape(h, w)
    n = np.zeros(w * h, np.int64)
    for i in range(4):
        xs = np.clip(np.where(ok, hx, 0) + i % 2, 0, w - 1)
        ys = np.clip(np.where(ok, hy, 0) + i // 2, 0, h - 1)
        n += mh[ys, xs] != mask_now.reshape(-1)
    return (n / 4.0)[ok]


def frame(w, h, color=BASE, mask=1, normal=(0.0, 1.0, 0.0), albedo=0.5, depth=5.0, mv=(0.0, 0.0)):
    """One uniform frame; every argument broadcasts over (h, w[, c])."""
    P = w * h
    c = np.empty((P, 4), np.uint16)
    c[:, :3] = half(np.broadcast_to(np.asarray(color, np.float32), (h, w, 3))).reshape(P, 3)
    c[:, 3] = np.broadcast_to(np.asarray(mask, np.uint16), (h, w)).reshape(P)
    n = np.empty((P, 4), np.uint16)
    n[:, :3] = half(np.broadcast_to(np.asarray(normal, np.float32), (h, w, 3))).reshape(P, 3)
    n[:, 3] = 0
    a = np.empty((P, 4), np.uint16)
    a[:, :3] = half(np.broadcast_to(np.asarray(albedo, np.float32), (h, w, 3))).reshape(P, 3)
    a[:, 3] = H_ONE
    d = half(np.broadcast_to(np.asarray(depth, np.float32), (h, w))).reshape(P).copy()
    m = motion_bits(np.broadcast_to(np.asarray(mv, np.float32), (h, w, 2))).reshape(P, 2).copy()
    return dict(color=c, normal=n, albedo=a, depth=d, motion=m)


def subpixel_shift(w, h):
    """A uniform motion of about 0.3 pixels in x and y, as stored (half(mv + 0.5) rounds it)."""
    return unhalf(motion_bits((0.3 / w, 0.3 / h))) - np.float32(0.5)


def noisy_color(rng, w, h, amp):
    """BASE scaled per pixel by 1 + amp * U(-1, 1); amp broadcasts over (h, w)."""
    s = 1.0 + np.broadcast_to(np.asarray(amp, np.float32), (h, w)) * rng.uniform(-1.0, 1.0, (h, w))
    return np.asarray(BASE, np.float32)[None, None, :] * s[:, :, None].astype(np.float32)


def background(seed, w, h, f, amp=0.5):
    """The value families' common ground: noisy colour (so the tile lists fill), two materials in
    vertical halves, mild depth and normal variation, per-pixel sub-pixel motion; every family
    overwrites the buffer it stresses."""
    rng = np.random.default_rng([seed, w, h, f])
    x = np.arange(w)[None, :] + np.zeros((h, 1), np.int64)
    nrm = np.zeros((h, w, 3), np.float32)
    nrm[..., 1] = 1.0
    nrm[..., 0] = rng.uniform(-0.2, 0.2, (h, w))
    nrm /= np.linalg.norm(nrm, axis=2, keepdims=True)
    mv = rng.uniform(-0.4, 0.4, (h, w, 2)) / np.array([w, h])
    return frame(w, h, color=noisy_color(rng, w, h, amp), mask=np.where(x < w // 2, 1, 2), normal=nrm,
                 albedo=rng.uniform(0.25, 0.9, (h, w, 3)), depth=5.0 + rng.uniform(0.0, 0.02, (h, w)), mv=mv)


class Family:
    def __init__(self, name, fn, text):
        self.name, self._fn, self._text = name, fn, text

    def __call__(self, w, h, f):
        g = self._fn(w, h, f)
        for a in g.values():
            a.setflags(write=False)
        return g

    def describe(self):
        return "%s: %s" % (self.name, self._text)

    def __repr__(self):
        return self.name


# ---------------------------------------------------------------- uniform (the anchor)
def _uniform(shift):
    def fn(w, h, f):
        return frame(w, h, mv=subpixel_shift(w, h) if shift else (0.0, 0.0))
    return fn


# ---------------------------------------------------------------- regions
REGION_AMPS = (1.0, 0.05, 0.0)


def region_of(w, h):
    """0 strong noise, 1 mild noise, 2 exactly flat: vertical thirds."""
    x = np.arange(w)
    return np.broadcast_to(np.where(x < w // 3, 0, np.where(x < 2 * w // 3, 1, 2))[None, :], (h, w))


def _regions(w, h, f):
    rng = np.random.default_rng([11, w, h, f])
    reg = region_of(w, h)
    amp = np.asarray(REGION_AMPS, np.float32)[reg]
    noisy = reg < 2
    nrm = np.zeros((h, w, 3), np.float32)
    nrm[..., 1] = 1.0
    nrm[..., 2] = np.where(noisy, rng.uniform(-0.3, 0.3, (h, w)), 0.0)
    nrm /= np.linalg.norm(nrm, axis=2, keepdims=True)
    alb = np.where(noisy[..., None], rng.uniform(0.25, 0.9, (h, w, 3)), 0.5)
    dep = np.where(noisy, 5.0 + rng.uniform(0.0, 0.05, (h, w)), 5.0)
    mv = np.where(noisy[..., None], rng.uniform(-0.4, 0.4, (h, w, 2)) / np.array([w, h]), 0.0)
    return frame(w, h, color=noisy_color(rng, w, h, amp), mask=1 + reg, normal=nrm, albedo=alb, depth=dep, mv=mv)


# ---------------------------------------------------------------- colour values
COLOR_SPECIALS = (("65504", 0x7BFF), ("+Inf", 0x7C00), ("NaN", 0x7E00), ("-0", 0x8000), ("-1", 0xBC00),
                  ("-65504", 0xFBFF), ("min subnormal", 0x0001), ("max subnormal", 0x03FF))


def _color_values(w, h, f):
    g = background(21, w, h, f)
    c = g["color"].reshape(h, w, 4).copy()
    used = np.zeros((h, w), bool)
    n = len(COLOR_SPECIALS)
    ey, ex = min(15, h - 1), min(16, w - 1)  # a tile edge: the last row of tile row 0, the first column of tile column 1
    for i, (_, bits) in enumerate(COLOR_SPECIALS):
        c[ey, i::n, :3][: max(1, w // 16)] = bits
        c[i::n, ex, :3][: max(1, h // 16)] = bits
    used[ey, :] = used[:, ex] = True
    # whole 8x8 tiles (their variance is Inf / NaN): full tiles clear of the edge lines, spread over the frame
    slots = [(tx, ty) for ty in range(max(1, h // 8)) for tx in range(max(1, w // 8)) if ty != ey // 8 and tx != ex // 8]
    slots = slots or [(0, 0)]
    step = max(1, len(slots) // n)
    for i, (_, bits) in enumerate(COLOR_SPECIALS):
        tx, ty = slots[i * step % len(slots)]
        c[ty * 8:ty * 8 + 8, tx * 8:tx * 8 + 8, :3] = bits
        used[ty * 8:ty * 8 + 8, tx * 8:tx * 8 + 8] = True

    def free(k):  # the first pixel from k on, in raster order, that nothing above took
        order = (np.arange(w * h) + k) % (w * h)
        rest = order[~used.reshape(-1)[order]]
        p = int(rest[0]) if rest.size else k % (w * h)
        used.reshape(-1)[p] = True
        return divmod(p, w)

    for i, (_, bits) in enumerate(COLOR_SPECIALS):
        y, x = free(((3 + 7 * i) % h) * w + (5 + 11 * i) % w)
        c[y, x, i % 3] = bits  # one channel of a single pixel
        y, x = free(((11 + 5 * i) % h) * w + (2 + 13 * i) % w)
        c[y, x, :3] = bits     # a whole single pixel
    g["color"] = c.reshape(-1, 4)
    return g


# ---------------------------------------------------------------- depth
def _depth(all_sky):
    def fn(w, h, f):
        g = background(31, w, h, f)
        if all_sky:
            g["depth"] = np.full(w * h, SKY, np.uint16)
            return g
        d = g["depth"].reshape(h, w).copy()
        x = np.arange(w)[None, :] + np.zeros((h, 1), np.int64)
        y = np.arange(h)[:, None] + np.zeros((1, w), np.int64)
        band = x * 5 // w  # five vertical bands
        d[(band == 0) & ((x + y) % 2 == 0)] = SKY                      # per-pixel checkerboard
        d[(band == 1) & ((x // 8 + y // 8) % 2 == 0)] = SKY            # whole 8x8 tiles
        d[band == 2] = 0                                               # zero depth, equal neighbours
        d[band == 3] = ((x + 2 * y) % 8).astype(np.uint16)[band == 3]  # steps of one subnormal half
        d[(band == 4) & (y % 16 < 8)] = half(5.0)                      # equal neighbours
        g["depth"] = d.reshape(-1)
        return g
    return fn


# ---------------------------------------------------------------- normals
def _normals(w, h, f):
    g = background(41, w, h, f)
    n = g["normal"].reshape(h, w, 4).copy()
    x = np.arange(w)[None, :] + np.zeros((h, 1), np.int64)
    y = np.arange(h)[:, None] + np.zeros((1, w), np.int64)
    band = x * 6 // w
    n[band == 0, :3] = half((0.0, 0.0, 0.0))                             # zero vector
    n[band == 1, :3] = half((2.0, 0.5, 0.0))                             # non-unit, long
    n[band == 2, :3] = half((0.1, 0.1, 0.1))                             # non-unit, short
    n[(band == 3) & ((x + y) % 2 == 0), :3] = half((0.0, -1.0, 0.0))     # opposite of its neighbours
    n[(band == 3) & ((x + y) % 2 == 1), :3] = half((0.0, 1.0, 0.0))
    n[(band == 4) & ((x + 3 * y) % 5 == 0), 0] = 0x7E00                  # NaN in one component
    n[(band == 5) & (y % 4 == 0), :3] = 0x7E00                           # NaN rows
    g["normal"] = n.reshape(-1, 4)
    return g


# ---------------------------------------------------------------- masks
def mask_pattern(w, h):
    """The fixed pattern the masks family moves one pixel per frame: left half two materials per
    pixel at random (every 2x2 neighbourhood mix occurs), then stripes of 0, 0xFFFF and 7 whose
    edges lie inside the 16x16 tiles, the last band alternating per pixel."""
    rng = np.random.default_rng([51, w, h])
    x = np.arange(w)[None, :] + np.zeros((h, 1), np.int64)
    y = np.arange(h)[:, None] + np.zeros((1, w), np.int64)
    m = np.where(rng.integers(0, 2, (h, w)) == 1, 3, 4).astype(np.uint16)
    right = x >= w // 2
    stripe = ((x - w // 2) // 5) % 3
    m[right] = np.asarray([0, 0xFFFF, 7], np.uint16)[stripe][right]
    alt = x >= w - max(1, w // 8)
    m[alt] = np.where((x + y) % 2 == 0, 0, 0xFFFF).astype(np.uint16)[alt]
    return m


def _masks(w, h, f):
    g = background(52, w, h, f)
    c = g["color"].copy()
    c[:, 3] = np.roll(mask_pattern(w, h), f, axis=1).reshape(-1)
    g["color"] = c
    g["motion"] = motion_bits(np.zeros((w * h, 2), np.float32))  # mv = 0: the history texel is the pixel
    return g


# ---------------------------------------------------------------- motion
def exact_huv_hits(w, h):
    """[(axis, pixel coordinate, stored half bits, target)] with huv[axis] exactly `target` (0.0 or 1.0)
    in the kernel's float32 arithmetic: every (coordinate, half) pair of each axis is tried."""
    hv = unhalf(np.arange(0x7C00, dtype=np.uint16)) - np.float32(0.5)  # every finite non-negative half
    out = []
    for axis, n in ((0, w), (1, h)):
        inv = np.float32(1.0) / np.float32(n)
        uv = (np.arange(n, dtype=np.float32) + np.float32(0.5)) * inv
        s = (uv[:, None] + hv[None, :]).astype(np.float32)
        for target in (0.0, 1.0):
            for c, b in zip(*np.nonzero(s == np.float32(target))):
                out.append((axis, int(c), int(b), target))
    return out


def _motion_random(w, h, f):
    g = background(61, w, h, f)
    rng = np.random.default_rng([62, w, h, f])
    px = rng.uniform(-1.0, 1.0, (w * h, 2)) * np.where(rng.integers(0, 3, (w * h, 1)) == 0, 4.0, 0.9)
    g["motion"] = motion_bits(px / np.array([w, h]))
    return g


def _motion_border(w, h, f):
    """Border pixels at the nearest stored motion on either side of huv = 0 and huv = 1, and
    every (pixel, half) pair of each axis that makes huv exactly 0.0 or exactly 1.0."""
    g = background(63, w, h, f)
    m = g["motion"].reshape(h, w, 2).copy()
    for axis, n in ((0, w), (1, h)):
        inv = np.float32(1.0) / np.float32(n)
        for coord, target in ((0, 0.0), (n - 1, 1.0)):  # the border: just inside on even, just outside on odd lines
            uv = (np.float32(coord) + np.float32(0.5)) * inv
            b0 = int(half(np.float32(target) - uv + np.float32(0.5)))
            o0 = b0 if b0 < 0x8000 else -(b0 & 0x7FFF)  # the halves in value order, across zero
            cands = [o if o >= 0 else 0x8000 | -o for o in range(o0 - 2, o0 + 3)]
            s = (uv + (unhalf(np.array(cands, np.uint16)) - np.float32(0.5))).astype(np.float32)
            inside = [b for b, v in zip(cands, s) if 0.0 <= v <= 1.0]
            outside = [b for b, v in zip(cands, s) if not 0.0 <= v <= 1.0]
            near_in = min(inside, key=lambda b: abs(cands.index(b) - 2))
            near_out = min(outside, key=lambda b: abs(cands.index(b) - 2))
            line = m[:, coord, 0] if axis == 0 else m[coord, :, 1]
            line[0::2] = near_in
            line[1::2] = near_out
    for k, (axis, c, b, _) in enumerate(exact_huv_hits(w, h)):
        if axis == 0:
            m[k % h, c, 0] = b
            m[k % h, c, 1] = half(0.5)
        else:
            m[c, k % w, 1] = b
            m[c, k % w, 0] = half(0.5)
    g["motion"] = m.reshape(-1, 2)
    return g


MOTION_WILD = (("far out of frame", half(3.5)), ("far out of frame, negative", half(-2.5)), ("+Inf", 0x7C00),
               ("-Inf", 0xFC00), ("NaN", 0x7E00), ("65504", 0x7BFF), ("-65504", 0xFBFF))


def _motion_wild(w, h, f):
    g = background(64, w, h, f)
    m = g["motion"].reshape(h, w, 2).copy()
    x = np.arange(w)[None, :] + np.zeros((h, 1), np.int64)
    y = np.arange(h)[:, None] + np.zeros((1, w), np.int64)
    k = (x + 3 * y) % (3 * len(MOTION_WILD))  # one pixel in three is wild, in x, y or both
    for i, (_, bits) in enumerate(MOTION_WILD):
        sel = k == i
        m[sel & (y % 3 != 1), 0] = bits
        m[sel & (y % 3 != 0), 1] = bits
    g["motion"] = m.reshape(-1, 2)
    return g


# ---------------------------------------------------------------- albedo
def _albedo(w, h, f):
    g = background(71, w, h, f)
    a = g["albedo"].reshape(h, w, 4).copy()
    x = np.arange(w)[None, :] + np.zeros((h, 1), np.int64)
    y = np.arange(h)[:, None] + np.zeros((1, w), np.int64)
    band = x * 5 // w
    a[band == 0, :3] = 0                                   # black
    a[band == 1, :3] = half((2.0, 100.0, 1.5))             # above 1
    a[(band == 2) & ((x + y) % 3 == 0), :3] = 0x7C00       # Inf
    a[(band == 3) & ((x + y) % 3 == 0), 1] = 0x7E00        # NaN in one channel
    a[(band == 4) & (y % 8 == 0), :3] = 0x7E00             # NaN rows
    g["albedo"] = a.reshape(-1, 4)
    return g


FAMILIES = {f.name: f for f in (
    Family("uniform", _uniform(False), "colour %s, albedo 0.5, depth 5, normal +y, mask 1, motion 0" % (BASE,)),
    Family("uniform-shift", _uniform(True), "the uniform frame under a uniform ~0.3-pixel motion"),
    Family("regions", _regions, "vertical thirds of noise amplitude %s / %s / exactly flat (constant normal, "
           "depth, albedo), masks 1 / 2 / 3" % REGION_AMPS[:2]),
    Family("color-values", _color_values, "%s as single channels, single pixels, whole 8x8 tiles and along a tile "
           "edge, on noisy ground" % ", ".join(n for n, _ in COLOR_SPECIALS)),
    Family("depth", _depth(False), "bands of sky per pixel (checkerboard), sky in whole 8x8 tiles, zero, steps of "
           "one subnormal half, equal neighbours"),
    Family("depth-sky", _depth(True), "every pixel the sky sentinel 0x7C00"),
    Family("normals", _normals, "bands of zero, long, short, opposite per pixel, NaN component, NaN rows"),
    Family("masks", _masks, "two materials per pixel at random, stripes of 0 / 0xFFFF / 7 with edges inside "
           "tiles, per-pixel alternation; the pattern moves one pixel per frame, motion 0"),
    Family("motion-random", _motion_random, "per-pixel random motion, sub-pixel to four pixels"),
    Family("motion-border", _motion_border, "border pixels one stored step inside / outside huv = 0 and 1, and "
           "every pixel that reaches huv exactly 0.0 or 1.0"),
    Family("motion-wild", _motion_wild, "one pixel in three with %s in x, y or both" %
           ", ".join(n for n, _ in MOTION_WILD)),
    Family("albedo", _albedo, "bands of 0, above 1, Inf, NaN channel, NaN rows"),
)}
VALUE_FAMILIES = ("color-values", "depth", "depth-sky", "normals", "masks", "motion-random", "motion-border",
                  "motion-wild", "albedo")
OUT_OF_FRAME = ("motion-wild",)  # exempt from the reprojection condition


# ---------------------------------------------------------------- the cases both test files run
# (render W, H, screen Ws, Hs); a screen of None is the render size
SIZES = ((1, 1), (3, 5), (7, 7), (8, 8), (9, 17), (16, 16), (17, 9), (40, 24), (65, 33), (150, 86))
VALUE_SIZES = ((40, 24), (150, 86))
ANCHOR_SIZES = ((1, 1, None, None), (3, 5, None, None), (17, 9, None, None), (40, 24, None, None),
                (150, 86, None, None), (48, 27, 32, 18), (33, 19, 64, 36))
THRESHOLD_HI, THRESHOLD_LO = 0.005, 2e-5
# name -> (noise_threshold_local, noise_threshold_large)
THRESHOLDS = {"local>large": (THRESHOLD_HI, THRESHOLD_LO), "large>local": (THRESHOLD_LO, THRESHOLD_HI),
              "zero": (0.0, 0.0), "inf": (float("inf"), float("inf")), "nan": (float("nan"), float("nan"))}
# (W, H, Ws, Hs) -> (k_scale_post's LDS tile, whether its workgroups stage their reads: all of them,
# none, or "mixed": 96x54 -> 32x18 reads unstaged in screen tile row 0 (footprint 50 x 50 > 48 x 48)
# and staged in row 1, whose two screen rows cover 52 x 10 render texels)
SCALES = {(36, 18, 34, 17): ("small", "staged"), (37, 18, 34, 17): ("large", "staged"),
          (96, 54, 32, 18): ("large", "mixed"), (36, 54, 34, 18): ("large", "staged"),
          (16, 9, 64, 36): ("small", "staged"), (1, 1, 16, 16): ("small", "staged"),
          (50, 30, 33, 17): ("large", "staged")}


def scale_branches(W, H, Ws, Hs):
    """k_scale_post's read path per workgroup, restated from denoise.hip: the host's choice of
    the LDS tile (scale_lds_small) and, for every 16x16 screen tile, whether the footprint
    TW * TH of its 18x18 apron fits it.  Returns ("small" | "large", "staged" | "unstaged" | "mixed")."""
    def small(render, screen):
        return 17 * render + 5 * screen <= 24 * screen - screen

    def t1(x, S, R):  # bicubic_axis's first tap
        uv = np.float32(x) / np.float32(S)
        return int(np.floor(uv * np.float32(R) - np.float32(0.5)))

    def span(o, S, R):
        lo = int(np.clip(t1(int(np.clip(o, 0, S - 1)), S, R) - 1, 0, R - 1))
        hi = int(np.clip(t1(int(np.clip(o + 17, 0, S - 1)), S, R) + 2, 0, R - 1))
        return hi - lo + 1

    lds = 24 * 24 if small(W, Ws) and small(H, Hs) else 48 * 48
    staged = {span(tx * 16 - 1, Ws, W) * span(ty * 16 - 1, Hs, H) <= lds
              for ty in range((Hs + 15) // 16) for tx in range((Ws + 15) // 16)}
    return ("small" if lds == 24 * 24 else "large",
            "mixed" if len(staged) == 2 else "staged" if staged == {True} else "unstaged")
