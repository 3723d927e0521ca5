"""Linear-blend skinning without a GPU: rt_skin_vertices (the rule of include/rtx_amd.h compiled for the
host, the text the kernel compiles) against numpy restatements of the rule, its argument checks, the
state checks of rt_set_skin / rt_pose_skin* / rt_reset_skin / rt_get_skin / rt_time_stage(8) on a context
that was never inited, and the input checks of the Python wrappers."""
import ctypes as C

import numpy as np
import pytest

from skin_scenes import F, identity, random_pose, random_skin, rule32, rule64, slot_patterns, translation

RT_OK, RT_ERR_ARG, RT_ERR_STATE = 0, -1, -4


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


@pytest.fixture()
def rt(rtx):
    r = rtx.RayTracer(64, 64, None)  # created, not inited: no device needed
    yield r
    r.cleanup()


@pytest.mark.parametrize("nj", [1, 2, 4096])
@pytest.mark.parametrize("nv", [1, 6, 255, 256, 257])
def test_host_rule_equals_the_float32_restatement(rtx, nv, nj):
    """Bit for bit on seeded skins, and within the derived bound of the float64 sums: the chain to an
    output is at most 12 roundings deep (6 in t, one product, four sums, one spare), each relative
    2^-24 of a partial result that the magnitude sum bounds."""
    rest, joints, weights = random_skin(nv, nj, seed=100 * nv + nj)
    pose = random_pose(nj, seed=nj)
    if nv >= 255:  # 1, 2, 3 and 4 non-zero slots, starting in every position
        assert slot_patterns(weights) == {1, 2, 4, 8, 3, 6, 12, 9, 7, 14, 13, 11, 15}
        assert nj == 1 or (joints[weights != 0] == nj - 1).any()
    got = rtx.skin_vertices(rest, joints, weights, pose)
    assert got.dtype == np.float32 and got.shape == (nv, 3)
    assert np.array_equal(bits(got), bits(rule32(rest, joints, weights, pose)))
    ref, mag = rule64(rest, joints, weights, pose)
    err = np.abs(got.astype(np.float64) - ref)
    bound = 12.0 * 2.0 ** -24 * mag
    assert (err <= bound).all(), float((err / bound).max())
    assert np.array_equal(got, rtx.skin_vertices(rest, joints, weights, pose.reshape(nj, 12)))  # (J, 12) alike


def test_exact_translation_with_weight_one(rtx):
    rng = np.random.default_rng(5)
    rest = (rng.integers(-4096, 4096, size=(300, 3)) / 64.0).astype(F)  # multiples of 2^-6 below 64
    joints = np.zeros((300, 4), np.uint16)
    joints[:, 2] = np.arange(300) % 3
    weights = np.zeros((300, 4), F)
    weights[:, 2] = 1
    offs = np.asarray([(0.5, -1.25, 3.0), (-7.0, 0.015625, 2.5), (100.0, -0.75, 0.0)], F)
    pose = np.stack([translation(o) for o in offs])
    got = rtx.skin_vertices(rest, joints, weights, pose)
    assert np.array_equal(got, rest + offs[joints[:, 2]])


def test_identity_returns_the_rest_position_and_positive_zero(rtx):
    rest, joints, weights = random_skin(257, 3, seed=9)
    weights[:] = 0
    weights[np.arange(257), np.arange(257) % 4] = 1  # one joint of weight 1: nothing to round
    rest[::5, 0] = -0.0
    rest[1::7, 2] = 0.0
    got = rtx.skin_vertices(rest, joints, weights, identity(3))
    assert (got == rest).all()
    assert np.signbit(rest).any() and not np.signbit(got[rest == 0]).any()
    keep = rest != 0
    assert np.array_equal(bits(got)[keep], bits(rest)[keep])


def test_nan_matrix_reaches_only_the_vertices_that_weigh_it(rtx):
    rest, joints, weights = random_skin(300, 5, seed=11, last_joint=False)
    joints[joints == 4] = 0
    joints[weights == 0] = 4  # joint 4: named by zero-weight slots only
    assert (joints == 4).sum() > 100
    pose = random_pose(5, seed=3)
    clean = rtx.skin_vertices(rest, joints, weights, pose)
    bad = pose.copy()
    bad[4] = np.nan
    got = rtx.skin_vertices(rest, joints, weights, bad)
    assert np.isfinite(got).all() and np.array_equal(bits(got), bits(clean))
    v = 123
    k = int(np.nonzero(weights[v])[0][0])
    joints[v, k] = 4
    got = rtx.skin_vertices(rest, joints, weights, bad)
    assert np.isnan(got[v]).all()
    others = np.arange(300) != v
    assert np.array_equal(bits(got[others]), bits(clean[others]))


def _skin(rtx, rest, joints, weights, nj):
    return rtx.Skin(rest.ctypes.data, joints.ctypes.data, weights.ctypes.data, len(rest), nj)


def test_argument_checks_of_the_host_rule(rtx):
    L = rtx.load_library()
    rest, joints, weights = random_skin(8, 4, seed=1)
    pose = identity(4)
    out = np.full((8, 3), 7.0, F)
    ok = _skin(rtx, rest, joints, weights, 4)
    assert L.rt_skin_vertices(C.byref(ok), pose.ctypes.data, out.ctypes.data) == RT_OK
    assert np.array_equal(out, rule32(rest, joints, weights, pose))
    out[:] = 7.0
    cases = {"null skin": (None, pose.ctypes.data, out.ctypes.data),
             "null matrices": (C.byref(ok), None, out.ctypes.data),
             "null out": (C.byref(ok), pose.ctypes.data, None)}
    for field in ("rest_xyz", "joints", "weights"):
        s = _skin(rtx, rest, joints, weights, 4)
        setattr(s, field, None)
        cases["null " + field] = (C.byref(s), pose.ctypes.data, out.ctypes.data)
    big = np.zeros((4097, 12), F)
    for nj in (0, 4097):
        cases["joint_count %d" % nj] = (C.byref(_skin(rtx, rest, joints, weights, nj)), big.ctypes.data, out.ctypes.data)
    cases["no vertices"] = (C.byref(rtx.Skin(rest.ctypes.data, joints.ctypes.data, weights.ctypes.data, 0, 4)),
                            pose.ctypes.data, out.ctypes.data)
    keep = []
    j2 = joints.copy()
    j2[5, np.nonzero(weights[5] == 0)[0][0]] = 4  # equal to joint_count, in a slot of weight 0
    keep.append(j2)
    cases["joint index"] = (C.byref(_skin(rtx, rest, j2, weights, 4)), pose.ctypes.data, out.ctypes.data)
    for name, value in (("negative", -0.25), ("nan", np.nan), ("inf", np.inf)):
        w2 = weights.copy()
        w2[7, 3] = value
        keep.append(w2)
        cases[name + " weight"] = (C.byref(_skin(rtx, rest, joints, w2, 4)), pose.ctypes.data, out.ctypes.data)
    for name, args in cases.items():
        assert L.rt_skin_vertices(*args) == RT_ERR_ARG, name
        assert (out == 7.0).all(), name
    with pytest.raises(rtx.RtError, match="RT_ERR_ARG"):
        rtx.skin_vertices(rest, j2, weights, pose)


def test_calls_on_a_context_before_init(rtx, rt):
    L = rt.lib
    rest, joints, weights = random_skin(8, 2, seed=1)
    skin = _skin(rtx, rest, joints, weights, 2)
    m = identity(2)
    pose = rtx.Pose(m.ctypes.data, 2, None)
    nv, nj = C.c_uint32(7), C.c_uint32(7)
    ms = C.c_float(0)
    # NULL arguments are argument errors ahead of the state
    assert L.rt_set_skin(None, C.byref(skin)) == RT_ERR_ARG
    assert L.rt_set_skin(rt.h, None) == RT_ERR_ARG
    for field in ("rest_xyz", "joints", "weights"):
        s = _skin(rtx, rest, joints, weights, 2)
        setattr(s, field, None)
        assert L.rt_set_skin(rt.h, C.byref(s)) == RT_ERR_ARG, field
    assert L.rt_set_skin(rt.h, C.byref(_skin(rtx, rest, joints, weights, 0))) == RT_ERR_ARG
    assert L.rt_set_skin(rt.h, C.byref(_skin(rtx, rest, joints, weights, 4097))) == RT_ERR_ARG
    assert L.rt_set_skin(rt.h, C.byref(rtx.Skin(rest.ctypes.data, joints.ctypes.data, weights.ctypes.data, 0, 2))) == RT_ERR_ARG
    for fn in (L.rt_pose_skin, L.rt_pose_skin_device):
        assert fn(None, C.byref(pose)) == RT_ERR_ARG
        assert fn(rt.h, None) == RT_ERR_ARG
        assert fn(rt.h, C.byref(rtx.Pose(None, 2, None))) == RT_ERR_ARG
    assert L.rt_pose_skin_device(rt.h, C.byref(rtx.Pose(m.ctypes.data + 4, 2, None))) == RT_ERR_ARG  # misaligned
    assert L.rt_reset_skin(None) == RT_ERR_ARG
    assert L.rt_get_skin(None, C.byref(nv), C.byref(nj)) == RT_ERR_ARG
    assert L.rt_get_skin(rt.h, None, C.byref(nj)) == RT_ERR_ARG
    assert L.rt_get_skin(rt.h, C.byref(nv), None) == RT_ERR_ARG
    assert (nv.value, nj.value) == (7, 7)
    # ... and everything else is a state error that says so
    calls = {"rt_set_skin": lambda: L.rt_set_skin(rt.h, C.byref(skin)),
             "rt_pose_skin": lambda: L.rt_pose_skin(rt.h, C.byref(pose)),
             "rt_pose_skin_device": lambda: L.rt_pose_skin_device(rt.h, C.byref(pose)),
             "rt_reset_skin": lambda: L.rt_reset_skin(rt.h),
             "rt_time_stage": lambda: L.rt_time_stage(rt.h, 8, 1, C.byref(ms))}
    for name, call in calls.items():
        assert call() == RT_ERR_STATE, name
        err = L.rt_last_error(rt.h)
        assert b"before rt_init" in err and name.encode() in err, (name, err)
    assert L.rt_get_skin(rt.h, C.byref(nv), C.byref(nj)) == RT_OK and (nv.value, nj.value) == (0, 0)
    assert rt.skin == (0, 0)


class _NoLibrary:
    """Stands in for librtx: any call through it fails the test."""

    def __getattr__(self, name):
        raise AssertionError("the wrapper called %s for an array it must refuse" % name)


def _good():
    rest, joints, weights = random_skin(8, 2, seed=1)
    return dict(rest=rest, joints=joints, weights=weights)


BAD_SKINS = {
    "rest_float64": dict(rest=np.zeros((8, 3), np.float64)),
    "rest_n_by_4": dict(rest=np.zeros((8, 4), F)),
    "rest_strided": dict(rest=np.zeros((8, 6), F)[:, ::2]),
    "joints_int32": dict(joints=np.zeros((8, 4), np.int32)),
    "joints_int16": dict(joints=np.zeros((8, 4), np.int16)),
    "joints_n_by_3": dict(joints=np.zeros((8, 3), np.uint16)),
    "joints_fortran": dict(joints=np.zeros((4, 8), np.uint16).T),
    "weights_float64": dict(weights=np.zeros((8, 4), np.float64)),
    "weights_n_by_3": dict(weights=np.zeros((8, 3), F)),
    "weights_strided": dict(weights=np.zeros((8, 8), F)[:, ::2]),
    "weights_rows": dict(weights=np.zeros((7, 4), F)),
    "rest_list": dict(rest=[[0.0, 0.0, 0.0]] * 8),
}
BAD_POSES = {
    "float64": np.zeros((2, 3, 4), np.float64),
    "4_by_3": np.zeros((2, 4, 3), F),
    "n_by_16": np.zeros((2, 16), F),
    "flat": np.zeros(24, F),
    "strided": np.zeros((2, 24), F)[:, ::2],
    "fortran": np.zeros((4, 3, 2), F).T,
    "list": [[0.0] * 12] * 2,
}


@pytest.mark.parametrize("bad", list(BAD_SKINS), ids=list(BAD_SKINS))
def test_set_skin_refuses_bad_arrays_before_the_library(rtx, rt, bad, monkeypatch):
    a = dict(_good(), **BAD_SKINS[bad])
    lib = rt.lib
    rt.lib = _NoLibrary()
    monkeypatch.setattr(rtx, "load_library", lambda *args: _NoLibrary())
    try:
        with pytest.raises(ValueError):
            rt.set_skin(a["rest"], a["joints"], a["weights"], 2)
        with pytest.raises(ValueError):
            rtx.skin_vertices(a["rest"], a["joints"], a["weights"], identity(2))
    finally:
        rt.lib = lib


@pytest.mark.parametrize("bad", list(BAD_POSES), ids=list(BAD_POSES))
def test_pose_refuses_bad_arrays_before_the_library(rtx, rt, bad, monkeypatch):
    a = _good()
    lib = rt.lib
    rt.lib = _NoLibrary()
    monkeypatch.setattr(rtx, "load_library", lambda *args: _NoLibrary())
    try:
        with pytest.raises(ValueError):
            rt.pose_skin(BAD_POSES[bad])
        with pytest.raises(ValueError):
            rtx.skin_vertices(a["rest"], a["joints"], a["weights"], BAD_POSES[bad])
    finally:
        rt.lib = lib
