"""Closest-point queries without a GPU: the shared rule through rt_point_triangle, the definition of a
query's answer through rt_closest_points_host against float64 brute force, ties, and the argument and
state checks of the three entry points (include/rtx_amd.h) in their documented order.

Check order of rt_closest_points_device: NULL ctx / q; stride < 3; n > RT_QUERY_MAX_RAYS; a negative or
NaN max_distance; with n > 0 a NULL or misaligned points or out; then the init state."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import mesh_scenes
from closest_scenes import FOUND, FRONT, MISS, UNIT, bits, brute_distance64, mixed_points, triangles_of

RT_OK, RT_ERR_ARG, RT_ERR_IO, RT_ERR_STATE = 0, -1, -3, -4
HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "rtx_amd.h")
TRI = np.asarray([(0, 0, 0), (1, 0, 0), (0, 1, 0)], np.float32)
INF = float("inf")


def record(rtx, p, tri=TRI):
    r = rtx.point_triangle(np.asarray(p, np.float32), tri)
    w = r.view(np.uint32)
    return dict(c=r[0:3], d2=r[3], tri=int(r.view(np.int32)[4]), u=r[5], v=r[6], feature=int(w[7] & 7),
                front=bool(w[7] & FRONT), found=bool(w[7] & FOUND), word=int(w[7]), bits=w.copy())


def test_header_matches_the_mirror(rtx):
    text = open(HEADER).read()
    assert re.search(r"#define RT_CLOSEST_FLOATS\s+8u", text) and rtx.CLOSEST_FLOATS == 8
    assert "#define RT_CLOSEST_FRONT (1u << 16)" in text and rtx.CLOSEST_FRONT == FRONT
    assert "#define RT_CLOSEST_FOUND (1u << 17)" in text and rtx.CLOSEST_FOUND == FOUND
    m = re.search(r"typedef struct rt_closest_query \{(.*?)\} rt_closest_query;", text, re.S)
    fields = re.findall(r"([A-Za-z_0-9]+(?: [A-Za-z_0-9]+)?\*?)\s+(\w+);", m.group(1))
    assert [n for _, n in fields] == ["points", "stride", "n", "max_distance", "out", "ready_event", "done_event"]
    assert [n for n, _ in rtx.ClosestQuery._fields_] == [n for _, n in fields]
    # the C layout on LP64
    q = rtx.ClosestQuery
    assert (q.points.offset, q.stride.offset, q.n.offset, q.max_distance.offset, q.out.offset, q.ready_event.offset,
            q.done_event.offset, C.sizeof(q)) == (0, 8, 12, 16, 24, 32, 40, 48)
    for name in ("rt_closest_points_device", "rt_point_triangle", "rt_closest_points_host"):
        assert ("int %s(" % name) in text and name in rtx.SIGNATURES
    for word in ("signed distance", "per-point radii", "k nearest", "host-buffer variant"):
        assert word in text  # the "not provided" list


def test_vertices_edges_and_face_exactly(rtx):
    for k, (p, uv) in enumerate((((0, 0, 0), (1, 0)), ((1, 0, 0), (0, 1)), ((0, 1, 0), (0, 0)))):
        r = record(rtx, p)
        assert r["found"] and r["tri"] == 0 and r["d2"] == 0.0 and r["feature"] == k + 1
        assert (r["u"], r["v"]) == uv and r["c"].tolist() == list(p)
        r = record(rtx, np.asarray(p) * 3 - 1)  # beyond the vertex, away from the triangle
        assert r["feature"] == k + 1 and r["c"].tolist() == list(p)
    for p, code, c, d2, uv in (((0.5, -1, 0), 4, (0.5, 0, 0), 1.0, (0.5, 0.5)),   # beyond edge 12's midpoint
                               ((1.5, 1.5, 0), 5, (0.5, 0.5, 0), 2.0, (0.0, 0.5)),  # edge 23
                               ((-1, 0.5, 0), 6, (0, 0.5, 0), 1.0, (0.5, 0.0))):    # edge 31
        r = record(rtx, p)
        assert r["found"] and r["feature"] == code and r["c"].tolist() == list(c) and r["d2"] == d2, p
        assert (r["u"], r["v"]) == uv, p
        assert not r["front"]  # in the triangle's plane: the dot product is 0, not > 0
    for z, front in ((2.0, True), (-2.0, False)):
        r = record(rtx, (0.25, 0.25, z))
        assert r["found"] and r["feature"] == 0 and r["d2"] == 4.0 and r["front"] is front
        assert r["c"].tolist() == [0.25, 0.25, 0.0] and (r["u"], r["v"]) == (0.5, 0.25)
        assert r["word"] == (FOUND | (FRONT if front else 0))


def test_degenerate_triangles_and_points_that_are_not_finite(rtx):
    # a point with a coordinate that is not finite: the miss record, whatever the triangle
    for bad in (np.nan, np.inf, -np.inf):
        for k in range(3):
            p = np.asarray([0.25, 0.25, 1.0], np.float32)
            p[k] = bad
            assert np.array_equal(record(rtx, p)["bits"], MISS), (bad, k)
    # a triangle with a vertex that is not finite: d2 is a NaN, no candidate, whichever branch ends the walk
    for k in range(3):
        for bad in (np.nan, np.inf):
            t = TRI.copy()
            t[k, 1] = bad
            for p in ((0, 0, 0), (0.25, 0.25, 1), (5, 5, 5), (-1, -1, 0)):
                assert np.array_equal(record(rtx, p, t)["bits"], MISS), (k, bad, p)
    # zero area: three equal vertices end at vertex 1, collinear ones at a vertex or an edge, exactly
    r = record(rtx, (1, 2, 2), np.zeros((3, 3), np.float32))
    assert r["found"] and r["feature"] == 1 and r["d2"] == 9.0
    line = np.asarray([(0, 0, 0), (1, 0, 0), (2, 0, 0)], np.float32)
    r = record(rtx, (0.5, 1, 0), line)
    assert r["found"] and r["feature"] == 4 and r["d2"] == 1.0 and r["c"].tolist() == [0.5, 0, 0]
    r = record(rtx, (1.5, 1, 0), line)
    assert r["found"] and r["feature"] == 6 and r["d2"] == 1.0 and r["c"].tolist() == [1.5, 0, 0]
    # ... and the face's 1 / 0: va = vb = vc = 0 with no vertex or edge branch taken.  A NaN offset between
    # two vertices does it (every d is a NaN, every comparison false): d2 is a NaN, the miss record
    t = np.asarray([(0, 0, 0), (np.nan, 0, 0), (0, 1, 0)], np.float32)
    assert np.array_equal(record(rtx, (0.2, 0.2, 0.2), t)["bits"], MISS)
    # among others a triangle that is no candidate does not show
    out = rtx.closest_points_host(np.stack([t, TRI + np.float32(5.0), TRI]), np.asarray([(0.25, 0.25, 2)], np.float32))
    assert out.view(np.int32)[0, 4] == 2 and out[0, 3] == 4.0


def test_d2_is_the_stated_expression_bit_for_bit(rtx):
    """10,000 seeded cases, well-shaped and sliver triangles at offsets up to 1,000: d2 == |p - c|^2 in
    numpy float32 in the stated order, c is the stated combination of the vertices under (u, v, wc) for
    the vertex and edge features, and the front bit is the stated float32 expression."""
    rng = np.random.default_rng(2024)
    n = 10000
    tris = rng.uniform(-1.0, 1.0, (n, 3, 3))
    tris[::5, 2] = tris[::5, 0] + (tris[::5, 1] - tris[::5, 0]) * rng.uniform(-0.5, 1.5, (len(tris[::5]), 1)) \
        + rng.normal(size=(len(tris[::5]), 3)) * 1e-6  # slivers
    off = rng.uniform(-1.0, 1.0, (n, 1, 3)) * 10.0 ** rng.uniform(-1.0, 3.0, (n, 1, 1))
    tris = (tris + off).astype(np.float32)
    pts = (tris.mean(1) + rng.normal(size=(n, 3)) * 10.0 ** rng.uniform(-3.0, 1.0, (n, 1))).astype(np.float32)
    rec = np.stack([rtx.point_triangle(pts[k], tris[k]) for k in range(n)])
    w = rec.view(np.uint32)
    assert ((w[:, 7] & FOUND) != 0).all()
    c, d2 = rec[:, 0:3], rec[:, 3]
    d = pts - c
    want = (d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]
    assert want.dtype == np.float32 and np.array_equal(bits(want), bits(d2))
    feature = w[:, 7] & 7
    assert set(np.unique(feature)) == set(range(7))  # every branch is met
    u, v = rec[:, 5], rec[:, 6]
    one = np.float32(1.0)
    wc = np.select([feature == 1, feature == 2, feature == 3, feature == 4, feature == 5, feature == 6],
                   [0 * u, 0 * u, 0 * u + one, 0 * u, one - v, one - u], default=np.float32(np.nan))
    # edge 23 gives wb = 1 - t, edge 31 wa = 1 - t: t is not recoverable bit for bit from 1 - t in general,
    # so the combination is checked where wc is known exactly
    exact = np.isin(feature, (1, 2, 3, 4))
    comb = (tris[:, 0] * u[:, None] + tris[:, 1] * v[:, None]) + tris[:, 2] * wc[:, None]
    assert np.array_equal(bits(comb[exact]), bits(c[exact]))
    face = feature == 0
    assert ((u[face] >= 0) & (v[face] >= 0) & (u[face] + v[face] <= 1.0 + 2 ** -22)).all()
    ab, ac, ap = tris[:, 1] - tris[:, 0], tris[:, 2] - tris[:, 0], pts - tris[:, 0]
    nx = ab[:, 1] * ac[:, 2] - ab[:, 2] * ac[:, 1]
    ny = ab[:, 2] * ac[:, 0] - ab[:, 0] * ac[:, 2]
    nz = ab[:, 0] * ac[:, 1] - ab[:, 1] * ac[:, 0]
    front = ((nx * ap[:, 0] + ny * ap[:, 1]) + nz * ap[:, 2]) > 0
    assert np.array_equal(front, (w[:, 7] & FRONT) != 0)
    # the record's c lies within 8 * 2^-24 * M of the triangle's box: what the pruning bound builds on
    m = np.maximum(np.abs(tris).max(1), np.abs(pts))
    assert (c >= tris.min(1) - 8 * UNIT * m).all() and (c <= tris.max(1) + 8 * UNIT * m).all()


def test_host_answer_against_float64_brute_force(rtx):
    """grid(1023), 513 points on the surface, at vertices, inside the box and at 1,000 times the extent:
    |sqrt(d2) - dist64| <= 64 * 2^-24 * M, M the largest coordinate magnitude of the point and the mesh."""
    tris = triangles_of(*mesh_scenes.grid(1023))
    pts = mixed_points(tris, 513)
    out = rtx.closest_points_host(tris, pts)
    w = out.view(np.uint32)
    assert ((w[:, 7] & FOUND) != 0).all() and (out.view(np.int32)[:, 4] >= 0).all()
    want = brute_distance64(tris, pts)
    m = np.maximum(np.abs(pts.astype(np.float64)).max(1), float(np.abs(tris).max()))
    dev = np.abs(np.sqrt(out[:, 3].astype(np.float64)) - want) / (UNIT * m)
    print("worst |sqrt(d2) - dist64| = %.2f units of 2^-24 M (kinds: %s)" % (
        dev.max(), ", ".join("%.2f" % dev[k::4].max() for k in range(4))))
    assert dev.max() <= 64.0
    # the reported point is a point of the reported triangle at that distance
    t = tris[out.view(np.int32)[:, 4]].astype(np.float64)
    u, v = out[:, 5].astype(np.float64), out[:, 6].astype(np.float64)
    c = t[:, 0] * u[:, None] + t[:, 1] * v[:, None] + t[:, 2] * (1.0 - u - v)[:, None]
    assert (np.abs(c - out[:, 0:3]).max(1) <= 8 * UNIT * m).all()
    assert (np.abs(np.linalg.norm(pts - c, axis=1) - want) <= 64 * UNIT * m).all()
    on = np.arange(513) % 4 < 2  # on the surface and at vertices: the distance is rounding alone
    assert (np.sqrt(out[on, 3]) <= 64 * UNIT * m[on]).all()


def test_ties_ids_and_max_distance(rtx):
    far = TRI + np.asarray([0, 0, -3], np.float32)
    p = np.asarray([(0.25, 0.25, 2.0)], np.float32)  # 2 above TRI, 5 above far
    # coincident triangles: the lowest id, wherever it stands in the array
    tris = np.stack([far, TRI, TRI, TRI, far])
    assert rtx.closest_points_host(tris, p).view(np.int32)[0, 4] == 1
    for ids, want in (((9, 7, 5, 6, 1), 5), ((0, 40, 30, 20, 10), 20), ((4, 3, 2, 1, 0), 1), ((1, 2 ** 32 - 2, 8, 9, 0), 8)):
        out = rtx.closest_points_host(tris, p, ids=np.asarray(ids, np.uint32))
        assert out.view(np.uint32)[0, 4] == want and out[0, 3] == 4.0
    # permuting triangles and ids together changes nothing
    rng = np.random.default_rng(3)
    mesh = triangles_of(*mesh_scenes.grid(300))
    mesh = np.concatenate([mesh, mesh[:50]])  # with coincident copies under higher ids
    pts = mixed_points(mesh, 65)
    base = rtx.closest_points_host(mesh, pts)
    perm = rng.permutation(len(mesh))
    assert np.array_equal(bits(rtx.closest_points_host(mesh[perm], pts, ids=perm.astype(np.uint32))), bits(base))
    assert (base.view(np.int32)[:, 4] < 300).all()
    # max_distance: 0 finds only what touches; between the two nearest distances, the nearest; inf, the nearest
    two = np.stack([far, TRI])
    for md, tri in ((0.0, -1), (1.999, -1), (2.0, 1), (3.5, 1), (INF, 1)):
        out = rtx.closest_points_host(two, p, max_distance=md)
        assert out.view(np.int32)[0, 4] == tri, md
        assert np.array_equal(bits(out[0]), MISS) == (tri < 0)
    out = rtx.closest_points_host(two[:1], p, max_distance=4.999)
    assert np.array_equal(bits(out[0]), MISS)
    assert rtx.closest_points_host(two[:1], p, max_distance=5.0).view(np.int32)[0, 4] == 0
    touching = np.asarray([(0.25, 0.25, 0.0), (1, 0, 0), (0.3, 0.3, 1e-3)], np.float32)
    out = rtx.closest_points_host(two, touching, max_distance=0.0)
    assert out.view(np.int32)[:, 4].tolist() == [1, 1, -1] and out[:2, 3].tolist() == [0.0, 0.0]
    # no triangles, no points
    assert np.array_equal(bits(rtx.closest_points_host(np.zeros((0, 3, 3), np.float32), p)[0]), MISS)
    assert rtx.closest_points_host(two, np.zeros((0, 3), np.float32)).shape == (0, 8)


# ---- argument and state checks


@pytest.fixture()
def rt(rtx):
    r = rtx.RayTracer(64, 64, None)  # created, not inited: no device needed
    yield r
    r.cleanup()


@pytest.fixture()
def bufs():
    """Host memory standing in for device pointers: the checks never dereference them."""
    raw = np.zeros(64 * 8 + 8, np.float32)
    off = (-raw.ctypes.data % 16) // 4
    out = raw[off:off + 64 * 8]
    assert out.ctypes.data % 16 == 0
    return dict(points=np.zeros((64, 3), np.float32), out=out, keep=raw)


def query(rtx, b, **kw):
    f = dict(points=b["points"].ctypes.data, stride=3, n=64, max_distance=INF, out=b["out"].ctypes.data,
             ready_event=None, done_event=None)
    f.update(kw)
    return rtx.ClosestQuery(**f)


def test_device_query_refusals_in_the_documented_order(rt, rtx, bufs):
    L, b = rt.lib, bufs
    call = lambda q: L.rt_closest_points_device(rt.h, C.byref(q))  # noqa: E731
    bad_out = b["out"].ctypes.data + 4
    # 1. NULL ctx / q
    assert L.rt_closest_points_device(None, C.byref(query(rtx, b))) == RT_ERR_ARG
    assert L.rt_closest_points_device(rt.h, None) == RT_ERR_ARG
    # 2. each argument check, every later argument wrong as well, names itself
    steps = ((dict(stride=2), b"stride"), (dict(n=(1 << 30) + 1), b"RT_QUERY_MAX_RAYS"),
             (dict(max_distance=-1.0), b"max_distance"), (dict(points=None), b"must not be NULL"),
             (dict(points=b["points"].ctypes.data + 2), b"points must be 4-byte aligned"),
             (dict(out=bad_out), b"out must be 16-byte aligned"))
    for k, (kw, msg) in enumerate(steps):
        later = {}
        for kw2, _ in steps[k + 1:]:
            later.update(kw2)
        later.update(kw)
        assert call(query(rtx, b, **later)) == RT_ERR_ARG, kw
        err = L.rt_last_error(rt.h)
        assert msg in err and b"rt_closest_points_device" in err, (kw, err)
    for md in (float("nan"), -0.5, -INF):
        assert call(query(rtx, b, max_distance=md)) == RT_ERR_ARG
        assert b"max_distance" in L.rt_last_error(rt.h)
    assert call(query(rtx, b, out=None)) == RT_ERR_ARG
    assert call(query(rtx, b, stride=0)) == RT_ERR_ARG
    # 3. every well-formed query is a state error on this context
    for kw in (dict(), dict(max_distance=0.0), dict(max_distance=-0.0), dict(stride=8), dict(n=1 << 30), dict(n=1)):
        assert call(query(rtx, b, **kw)) == RT_ERR_STATE, kw
        assert b"rt_closest_points_device before rt_init" in L.rt_last_error(rt.h)
    # n == 0 needs no buffers, but its other arguments and the state are still checked
    assert call(query(rtx, b, n=0, points=None, out=None)) == RT_ERR_STATE
    assert call(query(rtx, b, n=0, points=None, out=bad_out)) == RT_ERR_STATE
    assert call(query(rtx, b, n=0, points=None, out=None, stride=1)) == RT_ERR_ARG
    assert call(query(rtx, b, n=0, points=None, out=None, max_distance=float("nan"))) == RT_ERR_ARG


def test_wrapper_packs_the_query(rt, rtx, bufs):
    b = bufs
    args = (b["points"].ctypes.data, 64, b["out"].ctypes.data)
    with pytest.raises(rtx.RtError, match="before rt_init"):
        rt.closest_points_device(*args)
    with pytest.raises(rtx.RtError, match="before rt_init"):
        rt.closest_points_device(*args, stride=8, max_distance=0.25)
    with pytest.raises(rtx.RtError, match="stride"):
        rt.closest_points_device(*args, stride=2)
    with pytest.raises(rtx.RtError, match="max_distance"):
        rt.closest_points_device(*args, max_distance=-1.0)
    with pytest.raises(rtx.RtError, match="out must be 16-byte aligned"):
        rt.closest_points_device(args[0], 64, args[2] + 8)
    with pytest.raises(ValueError):
        rt.closest_points_device(args[0], 1 << 32, args[2])


def test_host_entry_points_refuse_bad_arguments(rtx):
    L = rtx.load_library()
    p = np.zeros(3, np.float32)
    t = np.ascontiguousarray(TRI)
    out = np.zeros(8, np.float32)
    ids = np.zeros(1, np.uint32)
    P, T, O = p.ctypes.data, t.ctypes.data, out.ctypes.data
    assert L.rt_point_triangle(None, T, O) == RT_ERR_ARG
    assert L.rt_point_triangle(P, None, O) == RT_ERR_ARG
    assert L.rt_point_triangle(P, T, None) == RT_ERR_ARG
    assert L.rt_point_triangle(P, T, O) == RT_OK
    host = L.rt_closest_points_host
    assert host(T, None, 1, P, 1, INF, O) == RT_OK
    assert host(None, None, 1, P, 1, INF, O) == RT_ERR_ARG
    assert host(T, None, 1, None, 1, INF, O) == RT_ERR_ARG
    assert host(T, None, 1, P, 1, INF, None) == RT_ERR_ARG
    for md in (-1.0, float("nan"), -INF):
        assert host(T, None, 1, P, 1, md, O) == RT_ERR_ARG
    ids[0] = 0xFFFFFFFF  # the miss record's index
    assert host(T, ids.ctypes.data, 1, P, 1, INF, O) == RT_ERR_ARG
    assert host(None, None, 0, None, 0, INF, None) == RT_OK  # nothing to read or write
    assert host(None, None, 0, P, 1, 0.0, O) == RT_OK and np.array_equal(bits(out), MISS)
    with pytest.raises(ValueError):
        rtx.closest_points_host(TRI[None], np.zeros((2, 4), np.float32))
    with pytest.raises(ValueError):
        rtx.closest_points_host(TRI[None], np.zeros((2, 3), np.float32), ids=np.zeros(2, np.uint32))
    with pytest.raises(ValueError):
        rtx.point_triangle(np.zeros(4, np.float32), TRI)
    with pytest.raises(rtx.RtError):
        rtx.closest_points_host(TRI[None], np.zeros((2, 3), np.float32), max_distance=-2.0)


@pytest.mark.parametrize("value, rc", [("1", RT_ERR_ARG), ("33", RT_ERR_ARG), ("-4", RT_ERR_ARG), ("0", RT_ERR_ARG),
                                       ("two", RT_ERR_IO), ("2.5", RT_ERR_IO), ('"8"', RT_ERR_IO), ("[8]", RT_ERR_IO),
                                       ("2", RT_OK), ("32", RT_OK), ("17", RT_OK)])
def test_debug_closest_stack_key(rtx, tmp_path, value, rc):
    cfg = rtx.write_config(str(tmp_path / "c.toml"), 64, 36, extra="\n[debug]\nclosestStack = %s\n" % value, tuning={})
    L = rtx.load_library()
    h = C.c_void_p()
    got = L.rt_create(64, 36, cfg.encode(), C.byref(h))
    assert got == rc, (value, got)
    if got == RT_OK:
        L.rt_destroy(h)


class _NoLibrary:
    """Stands in for librtx: any call through it fails the test."""

    def __getattr__(self, name):
        raise AssertionError("the wrapper called %s for tensors it must refuse" % name)


def _torch():
    try:
        import torch

        torch.zeros((2, 3), dtype=torch.float32)
        return torch
    except Exception as e:  # no torch, or one that cannot make CPU tensors
        pytest.skip("torch CPU tensors unavailable: %s" % e)


def test_closest_refuses_bad_tensors_before_the_library(rt):
    torch = _torch()
    from rtx import query

    lib = rt.lib
    rt.lib = _NoLibrary()
    try:
        for pts, what in ((torch.zeros((4, 3), dtype=torch.float64), "float32"), (torch.zeros(12), "shape"),
                          (torch.zeros((4, 2)), "shape"), (torch.zeros((4, 9)), "shape"),
                          (torch.zeros((4, 6))[:, ::2], "inner stride"), (torch.zeros((1, 3)).expand(4, 3), "row stride"),
                          (np.zeros((4, 3), np.float32), "torch tensor"), (torch.zeros((4, 3)), "device"),
                          (torch.zeros((4, 8))[:, 0:3], "device")):
            with pytest.raises(ValueError, match=what):
                query.closest(rt, pts)
        ok = torch.zeros((4, 3))
        for out in (torch.zeros((4, 4)), torch.zeros((5, 8)), torch.zeros((4, 8), dtype=torch.int32), torch.zeros((8, 4)).T,
                    np.zeros((4, 8), np.float32)):
            with pytest.raises(ValueError, match="^out must be a contiguous \\(n, 8\\)"):
                query.closest(rt, ok, out=out)
        for md in (-1.0, float("nan")):
            with pytest.raises(ValueError, match="max_distance"):
                query.closest(rt, ok, max_distance=md)
    finally:
        rt.lib = lib


def test_views():
    torch = _torch()
    from rtx import query

    r = torch.arange(16, dtype=torch.float32).reshape(2, 8)
    r.view(torch.int32)[:, 4] = torch.tensor([77, -1], dtype=torch.int32)
    r.view(torch.int32)[:, 7] = torch.tensor([5 | FRONT | FOUND, 0], dtype=torch.int32)
    assert query.closest_position(r).tolist() == [[0, 1, 2], [8, 9, 10]] and query.distance2(r).tolist() == [3, 11]
    assert query.closest_tri(r).dtype == torch.int32 and query.closest_tri(r).tolist() == [77, -1]
    assert query.closest_uv(r).tolist() == [[5, 6], [13, 14]]
    assert query.closest_feature(r).tolist() == [5, 0]
    assert query.closest_front(r).dtype == torch.bool and query.closest_front(r).tolist() == [True, False]
    assert query.closest_found(r).tolist() == [True, False]
    assert query.closest_position(r).data_ptr() == r.data_ptr() and query.closest_uv(r).data_ptr() == r.data_ptr() + 20
