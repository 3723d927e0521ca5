"""Environment-map test inputs (rt_set_environment): seeded source images and a
float64 restatement of the rule that turns an image into the 512 x 256 equal-area sky table.

The restatement takes the memberships and the row weights through the oracle's rtmath (oracle.rtmath
"cos" / "sin" / "acos", the functions the rule names), so it owns the texels the fp32 rule owns; the
sums, the mean, the scale and the clamp are float64.  restate() also returns `terms`, the most source
texels one table cell owns in that source, from which the comparison's tolerance is derived."""
import functools

import numpy as np

TW, TH = 512, 256
MAXV = 65504.0
LAYOUT_TABLE, LAYOUT_LATLONG = 0, 1
F32 = np.float32
PI = F32(3.1415926535897932384626422832795028841971)


def _scatter(img, rng, upper_rows):
    """NaN, -1, -0, +Inf and 1e6 texels through the rows the rule reads (1e6 is +Inf as a half)."""
    h, w = upper_rows, img.shape[1]
    for k, v in enumerate((np.nan, -1.0, -0.0, np.inf, 1e6)):
        ys = rng.integers(0, h, 200)
        xs = rng.integers(0, w, 200)
        with np.errstate(over="ignore"):
            v = img.dtype.type(v)
        img[ys, xs, k % 3] = v       # one channel of 200 texels
        img[ys[:20], xs[:20], :] = v  # ... and 20 whole texels
    return img


@functools.lru_cache(maxsize=None)
def source(name):
    """(image (h, w, 4), layout) of a named source; the same arrays on every call."""
    rng = np.random.default_rng(sum(map(ord, name)) + 7)
    if name == "table_f32":
        img, layout = (rng.random((TH, TW, 4)) * 6.0).astype(np.float32), LAYOUT_TABLE
    elif name == "table_f16":
        img, layout = (rng.random((TH, TW, 4)) * 6.0).astype(np.float16), LAYOUT_TABLE
    elif name == "latlong_8x4_f32":  # the nearest-texel rule on both axes
        img, layout = (rng.random((4, 8, 4)) * 3.0 + 0.25).astype(np.float32), LAYOUT_LATLONG
    elif name == "latlong_1000x500_f32":  # one or two columns per cell; owned and empty table rows
        img = (rng.random((500, 1000, 4)) * 4.0).astype(np.float32)
        img, layout = _scatter(img, rng, 250), LAYOUT_LATLONG
    elif name == "latlong_2048x1024_f16":  # four columns per cell, long zenith runs
        img = (rng.random((1024, 2048, 4)) * 4.0).astype(np.float16)
        img, layout = _scatter(img, rng, 512), LAYOUT_LATLONG
    elif name == "bright_texel":
        img = np.full((TH, TW, 4), 0.01, np.float32)
        img[200, 100, :3] = 60000.0
        layout = LAYOUT_TABLE
    elif name == "zeros":
        img, layout = np.zeros((TH, TW, 4), np.float32), LAYOUT_TABLE
    else:
        raise KeyError(name)
    img.setflags(write=False)
    return img, layout


SOURCES = ("table_f32", "table_f16", "latlong_8x4_f32", "latlong_1000x500_f32", "latlong_2048x1024_f16",
           "bright_texel", "zeros")
SCALES = {"table_f32": 1.0, "table_f16": 0.75, "latlong_8x4_f32": 1.0, "latlong_1000x500_f32": 1.5,
          "latlong_2048x1024_f16": 2.0, "bright_texel": 1.0, "zeros": 1.0}


def sanitize(x):
    """The rule's source value, in float64: NaN, negatives and -0 are 0, everything else at most 65504."""
    x = np.asarray(x, np.float64)
    with np.errstate(invalid="ignore"):
        return np.where((x == x) & (x > 0), np.minimum(x, MAXV), 0.0)


def row_theta(r, hs):
    return F32(F32(PI * F32(2 * r + 1)) / F32(2 * hs))


def row_cells(oracle, hs):
    """(y_r, w_r) of the upper rows of a source of hs rows, through the oracle's rtmath."""
    ys, ws = [], []
    for r in range(hs // 2):
        th = float(row_theta(r, hs))
        ys.append(min(255, int(F32(F32(oracle.rtmath("cos", th)) * F32(256.0)))))
        ws.append(float(F32(oracle.rtmath("sin", th))))
    return np.array(ys), np.array(ws, np.float64)


def nearest_row(oracle, y, hs):
    a = F32(oracle.rtmath("acos", float(F32(F32(y) + F32(0.5)) / F32(256.0))))
    return min(hs // 2 - 1, int(F32(F32(a * F32(hs)) / PI)))


def restate(oracle, img, layout, scale):
    """(table (256, 512, 3) float64, terms) of the rule applied to `img`."""
    src = sanitize(np.asarray(img)[:, :, :3].astype(np.float64))
    scale = float(F32(scale))
    if layout == LAYOUT_TABLE:
        assert src.shape[:2] == (TH, TW)
        return np.minimum(src * scale, MAXV), 1
    hs, ws_ = src.shape[:2]
    col_cell = ((2 * np.arange(ws_) + 1) * 256) // ws_
    ncol = np.bincount(col_cell, minlength=TW)
    # per upper row: the sum over each table column's source columns (or its single nearest one)
    upper = src[:hs // 2]
    sums = np.zeros((hs // 2, TW, 3))
    starts = np.flatnonzero(np.r_[True, np.diff(col_cell) > 0])  # the cells ascend with the column
    sums[:, col_cell[starts]] = np.add.reduceat(upper, starts, axis=1)
    empty_cols = np.flatnonzero(ncol == 0)
    sums[:, empty_cols] = upper[:, ((2 * empty_cols + 1) * ws_) // 1024]
    n_c = np.maximum(ncol, 1).astype(np.float64)
    ys, wr = row_cells(oracle, hs)
    table = np.zeros((TH, TW, 3))
    terms = 1
    for y in range(TH):
        rows = np.flatnonzero(ys == y)
        if rows.size:
            w = wr[rows]
            table[y] = (w[:, None, None] * sums[rows]).sum(0) / (n_c[:, None] * w.sum())
        else:
            rows = np.array([nearest_row(oracle, y, hs)])
            table[y] = sums[rows[0]] / n_c[:, None]
        terms = max(terms, int(rows.size * n_c.max()))
    return np.minimum(table * scale, MAXV), terms


def pdf_of(table32):
    """dot(rgb, (0.3, 0.6, 0.1)) of a float32 table in float64, the constants as fp32 literals."""
    t = np.asarray(table32, np.float64)
    return t[..., 0] * float(F32(0.3)) + t[..., 1] * float(F32(0.6)) + t[..., 2] * float(F32(0.1))
