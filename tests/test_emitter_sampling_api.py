"""Emitter sampling at the C-ABI boundary, without a GPU: rt_set_emitter_sampling /
rt_get_emitter_sampling (include/rtx_amd.h) are bound and check their arguments in the documented order,
the [render] emitterSampling / emitterProbability config keys set the initial state (bad values are
refused by rt_create with RT_ERR_IO), and the two host-only rules, rt_emitter_weight and
rt_emitter_select, which are the device kernels' own functions compiled for the host, do what the header
says."""
import ctypes as C
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RT_OK, RT_ERR_ARG, RT_ERR_IO, RT_ERR_STATE = 0, -1, -3, -4
EPS = 2.0 ** -24


@pytest.fixture()
def rt(rtx):
    r = rtx.RayTracer(64, 64, None)  # created, not inited: no device needed
    yield r
    r.cleanup()


def test_header_entries_are_bound(rtx):
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "rtx_amd.h")).read(), flags=re.S)
    for name in ("rt_set_emitter_sampling", "rt_get_emitter_sampling", "rt_emitter_weight", "rt_emitter_select"):
        assert re.search(r"\bint\s+%s\s*\(" % name, text), name
        assert name in rtx.SIGNATURES and hasattr(rtx.load_library(), name), name
    for name, value in (("EMITTER_TRIS", 46), ("EMITTER_WEIGHTS", 47), ("EMITTER_CDF", 48), ("PT_Q3_BETA", 49)):
        assert rtx.ARR[name] == value
        assert re.search(r"\bRT_ARR_%s\s*=\s*%d\b" % (name, value), text), name


def test_argument_order_and_codes(rtx, rt):
    L = rt.lib
    on, q = C.c_int(7), C.c_float(7.0)
    assert L.rt_set_emitter_sampling(None, 1, 0.5) == RT_ERR_ARG
    assert L.rt_get_emitter_sampling(None, C.byref(on), C.byref(q)) == RT_ERR_ARG
    assert L.rt_get_emitter_sampling(rt.h, None, C.byref(q)) == RT_ERR_ARG
    assert L.rt_get_emitter_sampling(rt.h, C.byref(on), None) == RT_ERR_ARG
    assert on.value == 7 and q.value == 7.0
    # the probability is checked ahead of the state
    for bad in (float("nan"), float("inf"), -0.25, 1.5, -float("inf")):
        assert L.rt_set_emitter_sampling(rt.h, 1, bad) == RT_ERR_ARG, bad
        assert b"probability" in L.rt_last_error(rt.h)
    for good in (0.0, 0.5, 1.0):
        assert L.rt_set_emitter_sampling(rt.h, 1, good) == RT_ERR_STATE
        assert b"before rt_init" in L.rt_last_error(rt.h)
    assert L.rt_set_emitter_sampling(rt.h, 0, 0.5) == RT_ERR_STATE
    with pytest.raises(rtx.RtError, match="RT_ERR_STATE"):
        rt.set_emitter_sampling(True, 0.25)
    # nothing changed on an error: off and 0.5 by default
    assert L.rt_get_emitter_sampling(rt.h, C.byref(on), C.byref(q)) == RT_OK
    assert on.value == 0 and q.value == 0.5
    assert rt.emitter_sampling == (False, 0.5)


def test_off_by_default_and_keys_not_written(rtx, tmp_path):
    cfg = rtx.write_config(str(tmp_path / "plain.toml"), 64, 64)
    assert "emitter" not in open(cfg).read()
    r = rtx.RayTracer(64, 64, cfg)
    assert r.emitter_sampling == (False, 0.5)
    r.cleanup()


@pytest.mark.parametrize("on,q", [(True, 0.25), (False, 1.0), (True, 0.0), (True, None), (None, 0.75)])
def test_config_keys_set_the_initial_state(rtx, tmp_path, on, q):
    cfg = rtx.write_config(str(tmp_path / "e.toml"), 64, 64, emitter_sampling=on, emitter_probability=q)
    r = rtx.RayTracer(64, 64, cfg)
    assert r.emitter_sampling == (bool(on), 0.5 if q is None else q)
    r.cleanup()


def test_config_keys_are_read_from_the_render_table_only(rtx, tmp_path):
    cfg = rtx.write_config(str(tmp_path / "t.toml"), 64, 64, tuning={"emitterSampling": True, "emitterProbability": 0.25})
    r = rtx.RayTracer(64, 64, cfg)
    assert r.emitter_sampling == (False, 0.5)
    r.cleanup()


@pytest.mark.parametrize("line", ["emitterSampling = 1", 'emitterSampling = "true"', "emitterSampling = yes",
                                  "emitterProbability = half", 'emitterProbability = "0.5"', "emitterProbability = 0.5x",
                                  "emitterProbability = 1.5", "emitterProbability = -0.25", "emitterProbability = nan",
                                  'emitterProbability = ["0.5"]'],
                         ids=["on-int", "on-string", "on-yes", "q-word", "q-string", "q-trailing", "q-above", "q-negative",
                              "q-nan", "q-array"])
def test_config_refuses_bad_values(rtx, tmp_path, line):
    cfg = rtx.write_config(str(tmp_path / "bad.toml"), 64, 64, extra=line + "\n")
    h = C.c_void_p()
    assert rtx.load_library().rt_create(64, 64, cfg.encode(), C.byref(h)) == RT_ERR_IO
    assert not h.value
    assert line.split()[0].encode() in rtx.load_library().rt_last_error(None)
    with pytest.raises(rtx.RtError, match="RT_ERR_IO"):
        rtx.RayTracer(64, 64, cfg)


# ---------------------------------------------------------------- rt_emitter_weight

def well_shaped_triangles(n, seed):
    """n triangles with edge lengths in [0.1, 10] and smallest angle >= 20 degrees, anywhere within
    +-20 of the origin, in any orientation (rejection sampling in float64, returned as float32)."""
    rng = np.random.default_rng(seed)
    out = []
    while len(out) < n:
        scale = 10.0 ** rng.uniform(-0.7, 0.9)
        t = rng.uniform(-20.0, 20.0, 3) + rng.normal(size=(3, 3)) * scale
        t = t.astype(np.float32).astype(np.float64)
        e = [t[1] - t[0], t[2] - t[1], t[0] - t[2]]
        ln = [np.linalg.norm(x) for x in e]
        if min(ln) < 0.1 or max(ln) > 10.0:
            continue
        cos = [np.dot(-e[k - 1], e[k]) / (ln[k - 1] * ln[k]) for k in range(3)]
        if np.degrees(np.arccos(np.clip(max(cos), -1, 1))) < 20.0:
            continue
        out.append(t.astype(np.float32))
    return out


def weight64(t, e):
    t = np.asarray(t, np.float64)
    e = np.asarray(e, np.float32).astype(np.float64)
    area = 0.5 * np.linalg.norm(np.cross(t[1] - t[0], t[2] - t[0]))
    # the rule's fp32 coefficients, exactly
    lum = float(np.float32(0.2126)) * e[0] + float(np.float32(0.7152)) * e[1] + float(np.float32(0.0722)) * e[2]
    return area * lum


def test_weight_against_float64(rtx):
    rng = np.random.default_rng(11)
    worst = 0.0
    for t in well_shaped_triangles(200, 5):
        e = rng.uniform(0.0, 8.0, 3).astype(np.float32)
        e[rng.integers(0, 3)] = max(e.max(), np.float32(0.5))  # not black
        w = float(rtx.emitter_weight(t, e))
        ref = weight64(t, e)
        worst = max(worst, abs(w - ref) / ref)
    print("worst relative error %.3g (bound %.3g)" % (worst, 16 * EPS))
    assert worst <= 16 * EPS


def test_weight_scales_exactly_and_vanishes_without_emission(rtx):
    rng = np.random.default_rng(12)
    for t in well_shaped_triangles(50, 6):
        e = rng.uniform(0.1, 8.0, 3).astype(np.float32)
        w = rtx.emitter_weight(t, e)
        assert w > 0
        assert rtx.emitter_weight(t * np.float32(2.0), e) == np.float32(4.0) * w  # powers of two: exact
        assert rtx.emitter_weight(t, np.zeros(3, np.float32)) == 0.0


def test_weight_null_arguments(rtx):
    L = rtx.load_library()
    a, e, w = (C.c_float * 9)(), (C.c_float * 3)(), C.c_float(7.0)
    assert L.rt_emitter_weight(None, e, C.byref(w)) == RT_ERR_ARG
    assert L.rt_emitter_weight(a, None, C.byref(w)) == RT_ERR_ARG
    assert L.rt_emitter_weight(a, e, None) == RT_ERR_ARG
    assert w.value == 7.0


# ---------------------------------------------------------------- rt_emitter_select

R256 = [(k + 0.5) / 256.0 for k in range(256)]


def test_select_single_emitter(rtx):
    for w in (1.0, 3.5e-7, 8.25e5):
        for r in [0.0] + R256 + [float(np.nextafter(np.float32(1.0), np.float32(0.0)))]:
            assert rtx.emitter_select([w], r) == (0, 1.0)


def test_select_skips_zero_weight_slots_and_reports_the_cdf_share(rtx):
    weights = np.array([0.0, 2.0, 0.0, 0.0, 0.5, 1.25, 0.0, 4.0, 0.0], np.float32)
    cdf = np.cumsum(weights, dtype=np.float32)
    total = cdf[-1]
    seen = {}
    for r in R256:
        slot, prob = rtx.emitter_select(cdf, r)
        assert weights[slot] > 0, (r, slot)
        below = cdf[slot - 1] if slot else np.float32(0.0)
        assert prob == np.float32(cdf[slot] - below) / total  # the fp32 CDF difference over the total
        # the first slot whose CDF value reaches the target, restated
        assert slot == int(np.argmax(cdf >= np.float32(r) * total))
        seen[slot] = float(prob)
    assert sorted(seen) == [1, 4, 5, 7]
    assert abs(sum(seen.values()) - 1.0) <= 4 * EPS * len(cdf)


def test_select_reaches_slot_zero_and_the_last_slot(rtx):
    rng = np.random.default_rng(3)
    weights = rng.uniform(0.1, 2.0, 37).astype(np.float32)
    cdf = np.cumsum(weights, dtype=np.float32)
    assert rtx.emitter_select(cdf, 0.0)[0] == 0
    assert rtx.emitter_select(cdf, 0.5 / 256)[0] == 0
    assert rtx.emitter_select(cdf, float(np.nextafter(np.float32(1.0), np.float32(0.0))))[0] == 36
    assert rtx.emitter_select(cdf, 1.0)[0] == 36  # the search ends inside the list for any r
    probs = {}
    for r in np.linspace(0.0, 1.0, 4001)[:-1]:
        s, p = rtx.emitter_select(cdf, float(r))
        probs[s] = float(p)
    assert len(probs) == 37
    assert abs(sum(probs.values()) - 1.0) <= 4 * EPS * len(cdf)


def test_select_null_arguments_and_empty_list(rtx):
    L = rtx.load_library()
    cdf, slot, prob = (C.c_float * 2)(1.0, 2.0), C.c_uint32(7), C.c_float(7.0)
    assert L.rt_emitter_select(None, 2, 0.5, C.byref(slot), C.byref(prob)) == RT_ERR_ARG
    assert L.rt_emitter_select(cdf, 2, 0.5, None, C.byref(prob)) == RT_ERR_ARG
    assert L.rt_emitter_select(cdf, 2, 0.5, C.byref(slot), None) == RT_ERR_ARG
    assert L.rt_emitter_select(cdf, 0, 0.5, C.byref(slot), C.byref(prob)) == RT_ERR_ARG
    assert slot.value == 7 and prob.value == 7.0
