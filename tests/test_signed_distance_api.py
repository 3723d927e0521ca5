"""Signed distance queries without a GPU: the pseudo-normal rule through rt_pseudo_normals against its float64
restatement, the properties of the table (shared edges, boundary edges, an edge of three triangles,
degenerate triangles), the sign through rt_closest_points_host + rt_signed_distance_rule against the
generalised winding number, and the argument and state checks of the entry points (include/rtx_amd.h) in
their documented order.

Check order of rt_signed_distance_device: NULL ctx / q; the closest query's argument checks; unknown flags;
with n > 0 a NULL or misaligned signed_out; then the init state and the table."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import sdf_scenes as S
from closest_scenes import FOUND, FRONT, MISS, bits, triangles_of

RT_OK, RT_ERR_ARG, RT_ERR_IO, RT_ERR_STATE = 0, -1, -3, -4
HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "rtx_amd.h")
INF = float("inf")
MISS4 = np.asarray([0, 0, 0, 0x7F800000], np.uint32)


@pytest.fixture(scope="module")
def tables(rtx):
    """name -> (vertices, indices, the library's table (ntri, 6, 4)), once for the module."""
    out = {}
    for name, make in S.SCENES.items():
        v, idx = make()
        t = rtx.pseudo_normals(v, idx)
        for a in (v, idx, t):
            a.setflags(write=False)
        out[name] = (v, idx, t)
    return out


@pytest.fixture(scope="module")
def signs(rtx):
    """name -> (points, float64 winding numbers, host records, host sign quads) of the closed scenes."""
    out = {}
    for name, make in S.CLOSED.items():
        v, idx = make()
        pts = S.sign_points(v, idx)
        rec, sd = S.host_answers(rtx, v, idx, pts)
        out[name] = (v, idx, pts, S.winding64(v, idx, pts), rec, sd)
    return out


def test_header_matches_the_mirror(rtx):
    text = open(HEADER).read()
    assert re.search(r"#define RT_DISTANCE_FROM_RECORDS\s+1u", text) and rtx.DISTANCE_FROM_RECORDS == 1
    assert re.search(r"RT_ARR_PSEUDO_NORMALS = 51\b", text) and rtx.ARR["PSEUDO_NORMALS"] == 51
    m = re.search(r"typedef struct rt_distance_query \{(.*?)\} rt_distance_query;", text, re.S)
    fields = re.findall(r"([A-Za-z_0-9]+\*?)\s+(\w+);", re.sub(r"/\*.*?\*/", "", m.group(1), flags=re.S))
    assert [n for _, n in fields] == ["closest", "signed_out", "flags"]
    assert [n for n, _ in rtx.DistanceQuery._fields_] == [n for _, n in fields]
    q = rtx.DistanceQuery
    assert (q.closest.offset, q.signed_out.offset, q.flags.offset, C.sizeof(q)) == (0, 48, 56, 64)
    assert C.sizeof(rtx.ClosestQuery) == 48  # rt_closest_query did not grow
    lib = rtx.load_library()
    for name in ("rt_set_signed_distance", "rt_get_signed_distance", "rt_signed_distance_device", "rt_pseudo_normals",
                 "rt_signed_distance_rule"):
        assert ("int %s(" % name) in text and name in rtx.SIGNATURES and hasattr(lib, name), name
    for word in ("per-point radii", "k nearest", "host-buffer variant", "generalised winding number"):
        assert word in text  # the "not provided" list


def test_scenes_are_what_they_claim():
    for name, make in S.CLOSED.items():
        v, idx = make()
        assert S.signed_volume(v, idx) > 0, name  # wound outward
        if name != "cube":  # welded: every directed edge once, its reverse once
            e = S.directed_edges(idx)
            fwd = set(map(tuple, e.tolist()))
            assert len(fwd) == len(e) and all((b, a) in fwd for a, b in fwd), name
    v, idx = S.wedge()
    t = triangles_of(v, idx).astype(np.float64)
    n = np.cross(t[:, 1] - t[:, 0], t[:, 2] - t[:, 0])
    n /= np.linalg.norm(n, axis=1)[:, None]
    assert np.degrees(np.pi - np.arccos(n[0] @ n[1])) < 10.0  # the dihedral angle along v0 v1
    assert len(S.torus()[1]) == 192
    assert len(S.grid1100()[1]) == 1100 and len(S.grid1101()[1]) % 4 != 0


def test_table_matches_the_float64_rule(rtx, tables):
    """Every entry against rule64 within table_tolerance (derived there from the formats and the scene's
    conditioning, not from these results).  Measured on these scenes: at most 8.8e-7 (grid1100) against
    tolerances of 1.6e-5 .. 6.9e-5."""
    for name, (v, idx, got) in tables.items():
        want, cnt = S.rule64(v, idx)
        tol = S.table_tolerance(v, idx)
        dev = float(np.abs(got[:, :, :3].astype(np.float64) - want).max())
        print("%-12s %5d triangles: max |fp32 - float64| = %.3g, tolerance %.3g" % (name, len(idx), dev, tol))
        assert dev <= tol, (name, dev, tol)
        assert tol < 1e-4, (name, tol)  # the bound itself stays far below any entry that counts (>= 0.1)
        assert (got[:, :, 3].view(np.uint32) == 0).all(), name  # .w = +0
        assert ((cnt > 0) | (bits(got[:, :, :3]).reshape(len(idx), 6, 3) == 0).all(2)).all(), name


def test_shared_edges_hold_the_same_bits(tables):
    """Both (all) triangles of an undirected edge store bit-equal entries for it, and the corners of a vertex
    bit-equal vertex entries."""
    shared = 0
    for name, (v, idx, tab) in tables.items():
        b = bits(tab[:, :, :3]).reshape(len(idx), 6, 3)
        edges, verts = {}, {}
        for t in range(len(idx)):
            for k in range(3):
                a, c = int(idx[t, k]), int(idx[t, (k + 1) % 3])
                edges.setdefault((min(a, c), max(a, c)), []).append(b[t, 3 + k].tobytes())
                verts.setdefault(a, []).append(b[t, k].tobytes())
        for key, vals in edges.items():
            assert len(set(vals)) == 1, (name, key)
            shared += len(vals) > 1
        for key, vals in verts.items():
            assert len(set(vals)) == 1, (name, key)
    assert shared > 1000


def unit32(rtx, v, idx, t):
    """The library's own unit normal of triangle t: the face answer of the sign rule."""
    tri = np.ascontiguousarray(v[idx[t]], np.float32)
    p = (tri.mean(0) + np.float32(0.001) * np.cross(tri[1] - tri[0], tri[2] - tri[0])).astype(np.float32)
    rec = rtx.point_triangle(p, tri)
    assert rec.view(np.uint32)[7] & 7 == 0
    out = np.zeros(4, np.float32)
    lib = rtx.load_library()
    assert lib.rt_signed_distance_rule(p.ctypes.data, rec.ctypes.data, tri.reshape(9).ctypes.data,
                                       np.zeros(24, np.float32).ctypes.data, out.ctypes.data) == RT_OK
    return out[:3]


def test_boundary_edges_and_the_fin(rtx, tables):
    # a boundary edge holds its own triangle's unit normal, bit for bit
    v, idx, tab = tables["grid40"]
    e = S.directed_edges(idx)
    count = {}
    for a, b in e.tolist():
        count[(min(a, b), max(a, b))] = count.get((min(a, b), max(a, b)), 0) + 1
    seen = 0
    for t in range(len(idx)):
        for k in range(3):
            a, b = int(idx[t, k]), int(idx[t, (k + 1) % 3])
            if count[(min(a, b), max(a, b))] == 1:
                assert np.array_equal(bits(tab[t, 3 + k, :3]), bits(unit32(rtx, v, idx, t))), (t, k)
                seen += 1
    assert seen >= 20
    # the fin's edge v0 v1: the sum of the three unit normals in triangle order, in float32
    v, idx, tab = tables["fin"]
    n = [unit32(rtx, v, idx, t) for t in range(3)]
    want = (np.zeros(3, np.float32) + n[0]) + n[1]
    want = want + n[2]
    assert want.dtype == np.float32
    for t, k in ((0, 0), (1, 0), (2, 0)):  # edge 12 of each triangle is (0, 1) or (1, 0)
        assert np.array_equal(bits(tab[t, 3 + k, :3]), bits(want)), t
    assert np.abs(want).max() > 0.1
    # the wing edges belong to one triangle each
    assert np.array_equal(bits(tab[0, 4, :3]), bits(n[0])) and np.array_equal(bits(tab[2, 5, :3]), bits(n[2]))


def test_degenerate_and_nan_triangles_contribute_nothing(rtx, tables):
    v, idx, tab = tables["bad_fan"]
    b = bits(tab[:, :, :3]).reshape(len(idx), 6, 3)
    # their own edges that no counted triangle shares are zero: the zero-area triangle's rim edge (4, 5),
    # the NaN triangle's rim edge (9, 10) and its spoke (10, 0)
    assert (b[3, 4] == 0).all() and (b[8, 4] == 0).all() and (b[8, 5] == 0).all()
    assert (b[8, 2] == 0).all()  # vertex 10 is named by the NaN triangle alone
    assert not np.isnan(tab).any()
    # the table equals that of the fan without the two triangles, entry for entry
    keep = np.asarray([t for t in range(len(idx)) if t not in (3, 8)])
    clean = np.where(np.isnan(v), np.float32(0), v)
    sub = rtx.pseudo_normals(clean, np.ascontiguousarray(idx[keep]))
    assert np.array_equal(bits(tab[keep]), bits(sub))
    # the spokes the bad triangles share with good neighbours hold the neighbour's unit normal alone
    assert np.array_equal(b[3, 3], bits(sub[2, 5, :3]))  # (0, 4): triangle 2's edge 31
    assert np.array_equal(b[3, 5], bits(sub[3, 3, :3]))  # (5, 0): triangle 4's edge 12 (row 3 of the rest)
    # the face of a degenerate triangle: N = (0, 0, 0), which reads as outside
    tri = np.ascontiguousarray(v[idx[3]], np.float32)
    rec = np.zeros(8, np.float32)
    rec[0:3], rec[3] = tri[0], 4.0
    rec.view(np.uint32)[7] = FOUND
    out = np.ones(4, np.float32)
    p = (tri[0] + np.float32(2.0)).astype(np.float32)
    assert rtx.load_library().rt_signed_distance_rule(p.ctypes.data, rec.ctypes.data, tri.reshape(9).ctypes.data,
                                                      tab[3].reshape(24).ctypes.data, out.ctypes.data) == RT_OK
    assert out.tolist() == [0.0, 0.0, 0.0, 2.0]


def test_padding_triangles_drop_out(rtx, tables):
    """Index triples (0, 0, 0) behind the mesh, as the device's padded index array holds them, change no entry."""
    v, idx, tab = tables["grid1101"]
    padded = np.concatenate([idx, np.zeros((3, 3), np.uint32)])
    got = rtx.pseudo_normals(v, padded)
    assert np.array_equal(bits(got[:len(idx)]), bits(tab))
    # their own rows: vertex 0's pseudo-normal three times, and edges (0, 0) that no counted triangle carries
    assert int(idx[0, 0]) == 0
    assert np.array_equal(bits(got[len(idx):, 0:3]), np.tile(bits(tab[0, 0]), (3, 3, 1))) and (bits(got[len(idx):, 3:6]) == 0).all()


def test_pseudo_normals_argument_errors(rtx):
    lib = rtx.load_library()
    v, idx = S.fin()
    out = np.zeros((len(idx), 24), np.float32)
    ok = (v.ctypes.data, len(v), idx.ctypes.data, len(idx), out.ctypes.data)
    assert lib.rt_pseudo_normals(*ok) == RT_OK
    for k in (0, 2, 4):  # NULL pointers
        a = list(ok)
        a[k] = None
        assert lib.rt_pseudo_normals(*a) == RT_ERR_ARG, k
    for k in (1, 3):  # zero counts
        a = list(ok)
        a[k] = 0
        assert lib.rt_pseudo_normals(*a) == RT_ERR_ARG, k
    bad = idx.copy()
    bad[2, 1] = len(v)
    assert lib.rt_pseudo_normals(v.ctypes.data, len(v), bad.ctypes.data, len(bad), out.ctypes.data) == RT_ERR_ARG
    rec, f9, f24, o4 = np.zeros(8, np.float32), np.zeros(9, np.float32), np.zeros(24, np.float32), np.zeros(4, np.float32)
    ok = (np.zeros(3, np.float32).ctypes.data, rec.ctypes.data, f9.ctypes.data, f24.ctypes.data, o4.ctypes.data)
    assert lib.rt_signed_distance_rule(*ok) == RT_OK
    for k in range(5):
        a = list(ok)
        a[k] = None
        assert lib.rt_signed_distance_rule(*a) == RT_ERR_ARG, k


def test_float64_rule_agrees_with_the_winding_number(signs):
    """The premise of the sign test, independent of the library: the rule restated in float64 gives the
    winding number's answer at every point, and the winding numbers are integers to 1e-9."""
    for name, (v, idx, pts, w, rec, sd) in signs.items():
        assert np.abs(w - np.round(w)).max() < 1e-9 and set(np.round(w).astype(int)) == {0, 1}, name
        assert np.array_equal(S.sign64(v, idx, pts), w > 0.5), name


def test_sign_equals_the_winding_number(signs):
    """2,000 points per closed scene, nothing excluded: distance < 0 exactly where the winding number is 1."""
    for name, (v, idx, pts, w, rec, sd) in signs.items():
        assert len(pts) == 2000
        inside = w > 0.5
        assert 100 < inside.sum() < 1900, (name, int(inside.sum()))
        bad = np.flatnonzero((sd[:, 3] < 0) != inside)
        assert len(bad) == 0, (name, len(bad), pts[bad[:4]].tolist())
        features = set((rec.view(np.uint32)[:, 7] & 7).tolist())
        assert {0} < features and features & {1, 2, 3} and features & {4, 5, 6}, (name, features)


def test_wedge_front_bit_is_not_the_sign(signs):
    """The case the feature exists for: beside the 9-degree edge the record's front bit says "behind" (the
    lowest-index triangle of the tie) while the point is outside and the signed distance positive."""
    v, idx, pts, w, rec, sd = signs["wedge"]
    front = (rec.view(np.uint32)[:, 7] & FRONT) != 0
    count = int((~front & (sd[:, 3] > 0) & (w < 0.5)).sum())
    print("wedge: %d of 2000 points behind their record's triangle, outside and positive" % count)
    assert count > 0
    assert (rec.view(np.uint32)[~front & (sd[:, 3] > 0), 7] & 7 != 0).all()  # never on a face


def test_magnitude_normal_and_misses(rtx, signs, tables):
    v, idx, pts, w, rec, sd = signs["torus"]
    assert np.array_equal(bits(np.abs(sd[:, 3])), bits(np.sqrt(rec[:, 3])))  # |.w| = sqrtf(d2), bit for bit
    assert rec.dtype == np.float32 and np.sqrt(rec[:, 3]).dtype == np.float32
    tab = tables["torus"][2]
    words = rec.view(np.uint32)
    feat, tri = words[:, 7] & 7, words[:, 4]
    k = feat > 0
    assert np.array_equal(bits(sd[k, :3]), bits(tab[tri[k], feat[k] - 1, :3]))  # .xyz = the table entry
    n = sd[~k, :3].astype(np.float64)
    assert np.abs((n * n).sum(1) - 1.0).max() < 1e-6  # a face: the unit normal
    # s = (Nx dx + Ny dy) + Nz dz in float32, and its sign
    d = pts - rec[:, 0:3]
    s = (sd[:, 0] * d[:, 0] + sd[:, 1] * d[:, 1]) + sd[:, 2] * d[:, 2]
    assert s.dtype == np.float32 and np.array_equal(s < 0, sd[:, 3] < 0)
    # misses: a finite max_distance, the miss record itself, index -1 with the found bit, a feature past 6
    near, sd2 = S.host_answers(rtx, v, idx, pts, max_distance=0.05)
    miss = (near.view(np.uint32)[:, 7] & FOUND) == 0
    assert 100 < miss.sum() < 1900
    assert np.array_equal(bits(sd2[miss]), np.tile(MISS4, (int(miss.sum()), 1)))
    assert np.array_equal(bits(sd2[~miss]), bits(sd[~miss]))
    forged = np.tile(rec[:4], (1, 1)).copy()
    fw = forged.view(np.uint32)
    fw[0] = MISS
    fw[1, 4] = 0xFFFFFFFF
    fw[2, 7] = FOUND | 7
    fw[3, 4] = len(idx)  # at the triangle count: a miss for the table's owner
    out = rtx.signed_distance_rule(pts[:4], forged, v, idx, tab)
    assert np.array_equal(bits(out), np.tile(MISS4, (4, 1)))
    # a zero s reads as outside: a vertex itself (d = 0, s = +0, d2 = 0)
    r0, s0 = S.host_answers(rtx, v, idx, np.ascontiguousarray(v[7:8]))
    assert r0[0, 3] == 0.0 and bits(s0[0, 3:4])[0] == 0


def test_setter_getter_and_query_argument_order(rtx, tmp_path):
    """Without rt_init: NULL checks, the argument errors in their order ahead of the state, then RT_ERR_STATE."""
    lib = rtx.load_library()
    on = C.c_int(7)
    assert lib.rt_set_signed_distance(None, 1) == RT_ERR_ARG
    assert lib.rt_get_signed_distance(None, C.byref(on)) == RT_ERR_ARG
    rt = rtx.RayTracer(64, 36, rtx.write_config(str(tmp_path / "a.toml"), 64, 36))
    try:
        assert lib.rt_get_signed_distance(rt.h, None) == RT_ERR_ARG
        assert lib.rt_get_signed_distance(rt.h, C.byref(on)) == RT_OK and on.value == 0
        assert lib.rt_set_signed_distance(rt.h, 1) == RT_ERR_STATE  # before rt_init
        assert rt.signed_distance is False
        Q, D = rtx.ClosestQuery, rtx.DistanceQuery
        call = lambda q: lib.rt_signed_distance_device(rt.h, C.byref(q))  # noqa: E731
        assert lib.rt_signed_distance_device(None, C.byref(D())) == RT_ERR_ARG
        assert lib.rt_signed_distance_device(rt.h, None) == RT_ERR_ARG
        good = dict(points=256, stride=3, n=4, max_distance=INF, out=512)
        # every argument error of the closest query, although signed_out and the flags are wrong too
        for change in (dict(stride=2), dict(n=(1 << 30) + 1), dict(max_distance=-1.0), dict(max_distance=float("nan")),
                       dict(points=None), dict(out=None), dict(points=258), dict(out=520)):
            q = D(Q(**dict(good, **change)), 8, 6)
            assert call(q) == RT_ERR_ARG, change
        assert call(D(Q(**good), 1024, 2)) == RT_ERR_ARG      # unknown flag bits
        assert call(D(Q(**good), 1024, 0x80000001)) == RT_ERR_ARG
        assert call(D(Q(**good), None, 0)) == RT_ERR_ARG      # NULL signed_out with n > 0
        assert call(D(Q(**good), 1032, 1)) == RT_ERR_ARG      # not 16-byte aligned
        # valid arguments: the state
        assert call(D(Q(**good), 1024, 0)) == RT_ERR_STATE
        assert call(D(Q(**good), 1024, 1)) == RT_ERR_STATE
        assert call(D(Q(**dict(good, n=0, points=None, out=None)), None, 0)) == RT_ERR_STATE
    finally:
        rt.cleanup()


def test_config_key(rtx, tmp_path):
    lib = rtx.load_library()
    on = C.c_int(7)
    for value, want in (("true", 1), ("false", 0)):
        cfg = rtx.write_config(str(tmp_path / ("c_%s.toml" % value)), 64, 36, signed_distance=value == "true")
        assert ("signedDistance = %s" % value) in open(cfg).read()
        rt = rtx.RayTracer(64, 36, cfg)
        assert lib.rt_get_signed_distance(rt.h, C.byref(on)) == RT_OK and on.value == want
        rt.cleanup()
    for k, bad in enumerate(('"true"', "1", "[true]", "yes")):
        cfg = rtx.write_config(str(tmp_path / ("b%d.toml" % k)), 64, 36, extra="signedDistance = %s\n" % bad)
        h = C.c_void_p()
        assert lib.rt_create(64, 36, cfg.encode(), C.byref(h)) == RT_ERR_IO, bad
        assert not h.value


def test_query_refuses_host_tensors_before_any_device_work(rtx):
    torch = pytest.importorskip("torch")
    from rtx import query

    with pytest.raises(ValueError):
        query.signed_distance(None, torch.zeros((4, 3)), max_distance=-1.0)
    with pytest.raises(ValueError):
        query.signed_distance(None, torch.zeros((4, 3)), records=torch.zeros((4, 8)), out=torch.zeros((4, 8)))
    with pytest.raises(ValueError):
        query.signed_distance(None, torch.zeros((4, 3)), signed_out=torch.zeros((4, 3)))
    with pytest.raises(ValueError):
        query.signed_distance(None, torch.zeros((4, 3)))  # not on a device
    sd = torch.tensor([[0.0, 0.0, 1.0, -0.5], [0.0, 0.0, 0.0, float("inf")]])
    assert query.signed_distance_of(sd).tolist() == [-0.5, float("inf")]
    assert query.inside(sd).tolist() == [True, False]
    assert query.pseudo_normal(sd).tolist() == [[0.0, 0.0, 1.0], [0.0, 0.0, 0.0]]
