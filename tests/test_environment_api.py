"""Sky sets and environment maps at the C-ABI boundary, without a GPU (rt_set_environment*, [scene]
skySets; include/rtx_amd.h): the header against the Python mirror, every argument
check that precedes the init state, in the stated order, on a context that is created but not inited,
the skySets parse and range errors, and the rule itself: rtx.environment_table (rt_environment_table,
the host build of csrc/env_kernels.h) against the float64 restatement of tests/environment_inputs.py."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import environment_inputs as E

RT_OK, RT_ERR_ARG, RT_ERR_IO, RT_ERR_STATE = 0, -1, -3, -4
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "rtx_amd.h")
CALLS = ("rt_get_sky_sets", "rt_set_environment", "rt_set_environment_device", "rt_reset_environment",
         "rt_get_environment", "rt_environment_table")


@pytest.fixture()
def rt(rtx):
    r = rtx.RayTracer(64, 64, None)  # created, not inited: no device needed
    yield r
    r.cleanup()


def header_text():
    with open(HEADER) as f:
        return re.sub(r"/\*.*?\*/", "", f.read(), flags=re.S)


def test_constants_and_entries_match_the_header(rtx):
    text = header_text()
    consts = {k: int(v, 0) for k, v in re.findall(r"#define\s+(RT_(?:ENV|SKY)\w+)\s+(\d+)\s", text)}
    assert consts["RT_SKY_SETS_MAX"] == rtx.SKY_SETS_MAX == 8
    assert consts["RT_ENV_FORMAT_F32X4"] == rtx.ENV_FORMAT_F32X4 == 0
    assert consts["RT_ENV_FORMAT_F16X4"] == rtx.ENV_FORMAT_F16X4 == 1
    assert consts["RT_ENV_LAYOUT_TABLE"] == rtx.ENV_LAYOUT_TABLE == E.LAYOUT_TABLE == 0
    assert consts["RT_ENV_LAYOUT_LATLONG"] == rtx.ENV_LAYOUT_LATLONG == E.LAYOUT_LATLONG == 1
    lib = rtx.load_library()
    for name in CALLS:
        assert re.search(r"\bint\s+%s\s*\(" % name, text), name
        res, args = rtx.SIGNATURES[name]
        fn = getattr(lib, name)
        assert fn.restype is res and list(fn.argtypes) == args
    for name in ("set_environment", "set_environment_device", "reset_environment"):
        assert callable(getattr(rtx.RayTracer, name))
    assert isinstance(rtx.RayTracer.sky_sets, property) and isinstance(rtx.RayTracer.environment_active, property)


def test_structure_matches_the_header(rtx):
    body = re.search(r"typedef\s+struct\s+rt_environment\s*\{(.*?)\}\s*rt_environment\s*;", header_text(), flags=re.S).group(1)
    fields = []
    for ty, names in re.findall(r"\b(const void\*|void\*|uint32_t|float)\s+([\w,\s]+?)\s*;", body):
        fields += [(ty, n.strip()) for n in names.split(",")]
    assert [n for _, n in fields] == ["texels", "width", "height", "format", "layout", "scale", "ready_event"]
    ctype = {"const void*": C.c_void_p, "void*": C.c_void_p, "uint32_t": C.c_uint32, "float": C.c_float}
    S = rtx.Environment
    assert [(n, t) for n, t in S._fields_] == [(name, ctype[ty]) for ty, name in fields]
    assert [getattr(S, n).offset for n, _ in S._fields_] == [0, 8, 12, 16, 20, 24, 32]
    assert C.sizeof(S) == 40


@pytest.mark.parametrize("value", ['"x"', "x", "-1", "1.5", "[2]"])
def test_unparsable_sky_sets_is_an_io_error(rtx, tmp_path, value):
    cfg = rtx.write_config(str(tmp_path / "c.toml"), 64, 64, sky_sets=value)
    assert "skySets = %s\n" % value in open(cfg).read()
    with pytest.raises(rtx.RtError, match="rt_create: RT_ERR_IO .*skySets"):
        rtx.RayTracer(64, 64, cfg)


def test_too_many_sky_sets_is_an_argument_error_of_init(rtx, tmp_path):
    """Raised before any device call: RT_ERR_ARG, not RT_ERR_NO_DEVICE, on a machine without a GPU too."""
    r = rtx.RayTracer(64, 64, rtx.write_config(str(tmp_path / "c.toml"), 64, 64, sky_sets=9))
    try:
        assert r.lib.rt_init(r.h) == RT_ERR_ARG
        assert b"skySets" in r.lib.rt_last_error(r.h)
        assert r.sky_sets == 9  # as configured; rt_init is what refuses it
    finally:
        r.cleanup()


@pytest.mark.parametrize("value,count", [(None, 1), (0, 1), (1, 1), (2, 2), (8, 8)])
def test_accepted_counts(rtx, tmp_path, value, count):
    cfg = rtx.write_config(str(tmp_path / "c.toml"), 64, 64, sky_sets=value)
    assert ("skySets" in open(cfg).read()) == (value is not None)
    r = rtx.RayTracer(64, 64, cfg)
    try:
        assert r.sky_sets == count
        n = C.c_uint32(99)
        assert r.lib.rt_get_sky_sets(None, C.byref(n)) == RT_ERR_ARG
        assert r.lib.rt_get_sky_sets(r.h, None) == RT_ERR_ARG
        assert n.value == 99
    finally:
        r.cleanup()


OK_TABLE = dict(texels=0x1000, width=512, height=256, format=0, layout=0, scale=1.0, ready_event=None)
BAD = [dict(texels=None), dict(format=2), dict(format=0xFFFFFFFF), dict(layout=2), dict(layout=0xFFFFFFFF),
       dict(width=511), dict(height=255), dict(width=256, height=512), dict(width=0, height=0),
       dict(layout=1, width=3, height=4), dict(layout=1, width=8, height=1), dict(layout=1, width=16385, height=8),
       dict(layout=1, width=8, height=16385), dict(scale=0.0), dict(scale=-1.0), dict(scale=float("inf")),
       dict(scale=float("nan"))]


@pytest.mark.parametrize("device", [False, True], ids=["host", "device"])
def test_checks_come_before_the_init_state(rtx, rt, device):
    L = rt.lib
    S = rtx.Environment
    fn = L.rt_set_environment_device if device else L.rt_set_environment
    assert fn(None, C.byref(S(**OK_TABLE))) == RT_ERR_ARG
    assert fn(rt.h, None) == RT_ERR_ARG
    for bad in BAD:
        assert fn(rt.h, C.byref(S(**dict(OK_TABLE, **bad)))) == RT_ERR_ARG, bad
    # alignment is the device pointer's: 16 B for f32x4, 8 B for f16x4
    for fmt, ptr, ok in ((0, 0x1008, False), (0, 0x1004, False), (0, 0x1010, True), (1, 0x1004, False), (1, 0x1008, True)):
        want = RT_ERR_ARG if device and not ok else RT_ERR_STATE
        assert fn(rt.h, C.byref(S(**dict(OK_TABLE, format=fmt, texels=ptr)))) == want, (fmt, hex(ptr))
        if want == RT_ERR_ARG:
            assert b"aligned" in L.rt_last_error(rt.h)
    # valid arguments of either layout: the state
    for ok in (OK_TABLE, dict(OK_TABLE, layout=1, width=4, height=2), dict(OK_TABLE, layout=1, width=16384, height=16384),
               dict(OK_TABLE, layout=1, width=1000, height=501, format=1, scale=1e-3)):
        assert fn(rt.h, C.byref(S(**ok))) == RT_ERR_STATE, ok
        assert b"before rt_init" in L.rt_last_error(rt.h)


def test_reset_get_and_table_checks(rtx, rt):
    L = rt.lib
    assert L.rt_reset_environment(None) == RT_ERR_ARG
    assert L.rt_reset_environment(rt.h) == RT_ERR_STATE
    on = C.c_int(7)
    assert L.rt_get_environment(None, C.byref(on)) == RT_ERR_ARG
    assert L.rt_get_environment(rt.h, None) == RT_ERR_ARG
    assert on.value == 7
    assert L.rt_get_environment(rt.h, C.byref(on)) == RT_OK and on.value == 0
    assert rt.environment_active is False
    table = np.zeros((256, 512, 4), np.float32)
    pdf = np.zeros((256, 512), np.float32)
    img = np.zeros((256, 512, 4), np.float32)
    S = rtx.Environment
    ok = dict(OK_TABLE, texels=img.ctypes.data)
    assert L.rt_environment_table(None, table.ctypes.data, pdf.ctypes.data) == RT_ERR_ARG
    assert L.rt_environment_table(C.byref(S(**ok)), None, pdf.ctypes.data) == RT_ERR_ARG
    assert L.rt_environment_table(C.byref(S(**ok)), table.ctypes.data, None) == RT_ERR_ARG
    for bad in BAD:
        assert L.rt_environment_table(C.byref(S(**dict(ok, **bad))), table.ctypes.data, pdf.ctypes.data) == RT_ERR_ARG, bad
    assert L.rt_environment_table(C.byref(S(**ok)), table.ctypes.data, pdf.ctypes.data) == RT_OK


def test_wrappers_validate_their_arguments(rtx, rt):
    with pytest.raises(ValueError):
        rtx.environment_table(np.zeros((256, 512, 4), np.float64), 0)
    with pytest.raises(ValueError):
        rtx.environment_table(np.zeros((256, 512, 3), np.float32), 0)
    with pytest.raises(rtx.RtError, match="rt_environment_table: RT_ERR_ARG"):
        rtx.environment_table(np.zeros((16, 16, 4), np.float32), 0)
    with pytest.raises(rtx.RtError, match="rt_set_environment: RT_ERR_STATE"):
        rt.set_environment(np.zeros((16, 16, 4), np.float16), 1)
    with pytest.raises(rtx.RtError, match="rt_set_environment: RT_ERR_ARG"):
        rt.set_environment(np.zeros((16, 16, 4), np.float16), 1, scale=0.0)
    with pytest.raises(ValueError):
        rt.set_environment_device(0x1000, 512, 256, 2, 0)
    with pytest.raises(rtx.RtError, match="rt_set_environment_device: RT_ERR_ARG"):
        rt.set_environment_device(0x1008, 512, 256, rtx.ENV_FORMAT_F32X4, 0)
    with pytest.raises(rtx.RtError, match="rt_set_environment_device: RT_ERR_STATE"):
        rt.set_environment_device(0x1008, 512, 256, rtx.ENV_FORMAT_F16X4, 0)
    with pytest.raises(rtx.RtError, match="rt_reset_environment: RT_ERR_STATE"):
        rt.reset_environment()


@pytest.mark.parametrize("name", E.SOURCES)
def test_table_against_the_float64_restatement(rtx, oracle, name):
    """The fp32 rule against its float64 restatement over the same memberships and weights.

    Tolerance, derived: a cell's value is a weighted sum of at most `terms` sanitised, non-negative source
    values over the sum of the weights, times n_c and the scale.  With u = 2^-24, summing non-negative
    terms in any order errs by at most (terms - 1) u relative, each product, the weight sum's own
    (terms - 1) u at most, the product with n_c, the division and the scale one u each: below
    (2 terms + 4) u.  (terms + 8) 2^-23 = (2 terms + 16) u bounds that; the factor 2 in 2^-23 is also
    what a weight 1 ulp off (rt_sinf, pinned by tests/test_rtmath.py) would cost, had the restatement
    not taken the same weights.  The clamp at 65504 and the sanitiser are monotonic and 1-Lipschitz."""
    img, layout = E.source(name)
    scale = E.SCALES[name]
    table, pdf = rtx.environment_table(img, layout, scale)
    assert table.shape == (256, 512, 4) and pdf.shape == (256, 512)
    assert not table[..., 3].any() and np.isfinite(table).all() and (table >= 0).all() and table.max() <= 65504.0
    ref, terms = E.restate(oracle, img, layout, scale)
    expect = {"latlong_8x4_f32": 1, "latlong_1000x500_f32": 2 * 14, "latlong_2048x1024_f16": 4 * 29}
    assert terms == expect.get(name, 1)
    tol = (terms + 8) * 2.0 ** -23  # 1.07e-6 for one term, 4.29e-6 for 28, 1.48e-5 for 116
    got = table[..., :3].astype(np.float64)
    assert np.array_equal(got == 0, ref == 0)
    assert (np.abs(got - ref) <= tol * ref).all(), float((np.abs(got - ref) / np.where(ref > 0, ref, 1)).max())
    # the pdf: a compensated dot product of three terms, within 2 ulp of the exact one
    p64 = E.pdf_of(table)
    assert (np.abs(pdf - p64) <= 2.0 ** -22 * p64).all()
    if name == "zeros":
        assert not table.any() and not pdf.any()
    if layout == E.LAYOUT_TABLE and name != "table_f16":  # scale 1: the sanitised source itself
        assert np.array_equal(table[..., :3], E.sanitize(img[..., :3]).astype(np.float32))


def test_sanitiser_cases_exactly(rtx):
    vals = [np.nan, -np.nan, -1.0, -0.0, 0.0, np.inf, -np.inf, 1e6, 65504.0, 65505.0, 70000.0, 40000.0, 1.5, 1e-30, -1e-30]
    for dtype in (np.float32, np.float16):
        img = np.full((256, 512, 4), 0.25, dtype)
        with np.errstate(over="ignore"):
            v = np.array(vals, np.float64).astype(dtype)
        img[0, :len(vals), 0] = v
        img[1, :len(vals), 1] = v
        img[2, :len(vals), 2] = v
        img[..., 3] = dtype(123.0)  # alpha is ignored: .w is 0
        for scale in (1.0, 2.0, 0.5):
            table, pdf = rtx.environment_table(img, E.LAYOUT_TABLE, scale)
            f = v.astype(np.float32)
            with np.errstate(invalid="ignore"):
                src = np.where((f == f) & (f > 0), np.minimum(f, np.float32(65504.0)), np.float32(0.0)).astype(np.float32)
            want = np.minimum(src * np.float32(scale), np.float32(65504.0))
            for ch in range(3):
                got = table[ch, :len(vals), ch]
                assert got.tobytes() == want.tobytes(), (dtype, scale, ch)  # -0, NaN and negatives are +0
            assert not table[..., 3].any()
            assert table[5, 5].tolist() == [0.25 * scale] * 3 + [0.0]
    # what the cases are, spelled out for fp32 at scale 2
    img = np.zeros((256, 512, 4), np.float32)
    img[0, :8, 0] = [np.nan, -1.0, -0.0, np.inf, 1e6, 40000.0, 30000.0, 1.5]
    table, _ = rtx.environment_table(img, E.LAYOUT_TABLE, 2.0)
    assert table[0, :8, 0].tolist() == [0.0, 0.0, 0.0, 65504.0, 65504.0, 65504.0, 60000.0, 3.0]
    assert not np.signbit(table).any()


@pytest.mark.parametrize("hs", [2, 4, 500, 501, 1024, 2048, 4096, 16384])
def test_row_ownership_never_increases(oracle, hs):
    """y_r is non-increasing in r for the heights the tests and the probe use (and the extremes), so
    each table row's source rows are one run, every y is in [0, 255], and the nearest row of a table
    row that owns none is an upper row."""
    ys, ws = E.row_cells(oracle, hs)
    assert len(ys) == hs // 2 and (np.diff(ys) <= 0).all()
    assert ys.min() >= 0 and ys.max() <= 255 and (ws > 0).all() and (ws <= 1).all()
    for y in sorted(set(range(256)) - set(ys.tolist()))[:: max(1, 256 // 16)]:
        assert 0 <= E.nearest_row(oracle, y, hs) <= hs // 2 - 1
