"""Meshes, points and expectations of the signed distance tests (rt_pseudo_normals, rt_signed_distance_rule,
rt_signed_distance_device).

All meshes are tiny, built in numpy, indexed and welded.  The expectations are numpy's alone: `rule64`
restates the pseudo-normal rule of include/rtx_amd.h in float64, `winding64` is the generalised winding
number (Jacobson et al. 2013, by van Oosterom and Strackee's solid angle), a reference that knows nothing
of pseudo-normals.  Neither calls the library."""
import numpy as np

import mesh_scenes
from closest_scenes import brute_distance64, triangles_of

F = np.float32
U = 2.0 ** -24


def _mesh(v, idx):
    return np.ascontiguousarray(v, F), np.ascontiguousarray(idx, np.uint32)


def wedge():
    """A tetrahedron whose faces along the edge v0 v1 meet at 2 atan(0.08) = 9.15 degrees: beside that edge
    a point outside the solid lies behind the plane of one of the two faces."""
    v = [(0, 0, 0), (1, 0, 0), (0.5, 1, 0.08), (0.5, 1, -0.08)]
    idx = [(0, 1, 2), (1, 0, 3), (0, 2, 3), (1, 3, 2)]
    return _mesh(v, idx)


def notch():
    """An L-shaped prism (the L in xy, z in [0, 1]): one concave edge, at (1, 1, z)."""
    poly = [(0, 0), (2, 0), (2, 1), (1, 1), (1, 2), (0, 2)]  # counter-clockwise
    caps = [(0, 1, 2), (0, 2, 3), (0, 3, 5), (3, 4, 5)]
    v = [(x, y, 0) for x, y in poly] + [(x, y, 1) for x, y in poly]
    idx = [(a, c, b) for a, b, c in caps] + [(a + 6, b + 6, c + 6) for a, b, c in caps]
    for i in range(6):
        j = (i + 1) % 6
        idx += [(i, j, j + 6), (i, j + 6, i + 6)]
    return _mesh(v, idx)


def torus(nu=12, nv=8, R=1.0, r=0.4):
    """nu x nv quads, 2 nu nv triangles (192), wound outward."""
    a = np.arange(nu) * (2.0 * np.pi / nu)
    b = np.arange(nv) * (2.0 * np.pi / nv)
    aa, bb = np.meshgrid(a, b, indexing="ij")
    v = np.stack([(R + r * np.cos(bb)) * np.cos(aa), (R + r * np.cos(bb)) * np.sin(aa), r * np.sin(bb)], -1).reshape(-1, 3)
    at = lambda i, j: (i % nu) * nv + (j % nv)  # noqa: E731
    idx = []
    for i in range(nu):
        for j in range(nv):
            p, q, s, t = at(i, j), at(i + 1, j), at(i + 1, j + 1), at(i, j + 1)
            idx += [(p, q, s), (p, s, t)]
    return _mesh(v, idx)


def welded_cube():
    """mesh_scenes.welded_cube as it is: each face welded, the faces not welded to each other (the cube's
    twelve edges are boundary edges of two faces each), and not all of them wound outward."""
    return mesh_scenes.welded_cube()


def cube():
    """welded_cube with every triangle wound outward: closed as a surface, convex, its edges and corners
    unwelded.  Around those the nearest feature is one face's boundary edge or corner, whose pseudo-normal is
    that face's normal: on a convex solid still the right sign."""
    v, idx = mesh_scenes.welded_cube()
    t = v.astype(np.float64)[idx.astype(np.int64)]
    inward = (np.cross(t[:, 1] - t[:, 0], t[:, 2] - t[:, 0]) * t.mean(1)).sum(1) < 0
    idx = idx.copy()
    idx[inward] = idx[inward][:, [0, 2, 1]]
    return _mesh(v, idx)


def fin():
    """Three triangles around the one edge v0 v1."""
    v = [(0, 0, 0), (0, 0, 1), (1, 0, 0.5), (-0.5, 0.8, 0.5), (-0.5, -0.8, 0.5)]
    return _mesh(v, [(0, 1, 2), (0, 1, 3), (1, 0, 4)])


def grid40():
    return mesh_scenes.grid(40)


def grid1100():
    """Triangle indices cross a 1,024 batch."""
    return mesh_scenes.grid(1100)


def grid1101():
    """... and a count that is no multiple of 4: three padding triangles at vertex 0."""
    return mesh_scenes.grid(1101)


def bad_fan():
    """An open fan of 9 triangles around vertex 0.  Triangle 3 has zero area: its rim vertices 4 and 5 share
    a position under two indices.  Triangle 8 has a NaN vertex, the last rim vertex, which no other names."""
    v, idx = mesh_scenes.fan(9)
    v = v.copy()
    v[5] = v[4]
    v[10] = np.nan
    return _mesh(v, idx)


CLOSED = {"wedge": wedge, "notch": notch, "torus": torus, "cube": cube}
OPEN = {"welded_cube": welded_cube, "fin": fin, "grid40": grid40, "grid1100": grid1100, "grid1101": grid1101, "bad_fan": bad_fan}
SCENES = dict(CLOSED, **OPEN)


def signed_volume(v, idx):
    t = np.asarray(v, np.float64)[np.asarray(idx, np.int64)]
    return float(np.einsum("ij,ij->i", t[:, 0], np.cross(t[:, 1], t[:, 2])).sum() / 6.0)


def directed_edges(idx):
    i = np.asarray(idx, np.int64)
    return np.concatenate([i[:, [0, 1]], i[:, [1, 2]], i[:, [2, 0]]])


# ---------------------------------------------------------------- the rule in float64


def unit_normals64(v, idx):
    """(unit normals (ntri, 3) with zeros for degenerate triangles, counted (ntri,) bool)."""
    t = np.asarray(v, np.float64)[np.asarray(idx, np.int64)]
    with np.errstate(all="ignore"):
        n = np.cross(t[:, 1] - t[:, 0], t[:, 2] - t[:, 0])
        l2 = (n * n).sum(1)
        ok = (l2 > 0) & np.isfinite(l2)
        unit = np.where(ok[:, None], n / np.sqrt(np.where(ok, l2, 1.0))[:, None], 0.0)
    return unit, ok


def corner_angles64(v, idx):
    """(ntri, 3) the angle at each corner; NaN where an edge has no length or is not finite."""
    t = np.asarray(v, np.float64)[np.asarray(idx, np.int64)]
    out = np.empty((len(t), 3))
    with np.errstate(all="ignore"):
        for k in range(3):
            ea, eb = t[:, (k + 1) % 3] - t[:, k], t[:, (k + 2) % 3] - t[:, k]
            q = (ea * eb).sum(1) / np.sqrt((ea * ea).sum(1) * (eb * eb).sum(1))
            out[:, k] = np.arccos(np.clip(q, -1.0, 1.0))
    return out


def rule64(v, idx):
    """The table (ntri, 6, 3) in float64 and each entry's number of counted terms (ntri, 6)."""
    idx = np.asarray(idx, np.int64)
    unit, ok = unit_normals64(v, idx)
    ang = corner_angles64(v, idx)
    nv = len(v)
    vsum, vcnt = np.zeros((nv, 3)), np.zeros(nv, np.int64)
    esum, ecnt = {}, {}
    for t in range(len(idx)):
        if not ok[t]:
            continue
        for k in range(3):
            a, b = int(idx[t, k]), int(idx[t, (k + 1) % 3])
            if not np.isnan(ang[t, k]):
                vsum[a] += ang[t, k] * unit[t]
                vcnt[a] += 1
            if a != b:
                key = (min(a, b), max(a, b))
                esum[key] = esum.get(key, np.zeros(3)) + unit[t]
                ecnt[key] = ecnt.get(key, 0) + 1
    out, cnt = np.zeros((len(idx), 6, 3)), np.zeros((len(idx), 6), np.int64)
    for t in range(len(idx)):
        for k in range(3):
            a, b = int(idx[t, k]), int(idx[t, (k + 1) % 3])
            out[t, k], cnt[t, k] = vsum[a], vcnt[a]
            key = (min(a, b), max(a, b))
            if key in esum:
                out[t, 3 + k], cnt[t, 3 + k] = esum[key], ecnt[key]
    return out, cnt


def min_corner_sine(v, idx):
    """The smallest sine of a corner angle among the counted triangles: the conditioning of the unit normal
    (|ab| |ac| / |ab x ac| = 1 / sin A) and of acos at every corner."""
    _, ok = unit_normals64(v, idx)
    a = corner_angles64(v, idx)[ok]
    return float(np.nanmin(np.sin(a)))


def table_tolerance(v, idx):
    """The bound on |fp32 table entry - float64 value| per component, u = 2^-24, s = min_corner_sine, k =
    the largest number of terms of an entry:
      - ab, ac round once (u each); a cross component's two products and difference then carry at most
        4 u |ab| |ac|, so |dn| <= 4 sqrt(3) u |ab| |ac| <= 7 u |n| / s; normalising doubles that and adds
        the roundings of l2, sqrtf and the quotient: |d unit| <= (14 / s + 3) u per component;
      - the quotient ahead of acos carries at most 6 u (two dots, a product, a sqrt, a division), acos
        multiplies by 1 / sin(angle) <= 1 / s and rounds once: |d angle| <= (6 / s + pi) u;
      - a vertex term angle * unit with angle <= pi: pi (14 / s + 3) u + (6 / s + pi) u + pi u (the product)
        <= (50 / s + 16) u; an edge term is smaller;
      - k terms, and k additions that each round a partial sum of at most k pi: k^2 pi u.
    A few ulp of the largest term (pi) times the valence, scaled by the scene's conditioning."""
    s = min_corner_sine(v, idx)
    k = int(rule64(v, idx)[1].max())
    return k * (50.0 / s + 16.0 + k * np.pi) * U


# ---------------------------------------------------------------- the winding number and the points


def winding64(v, idx, points):
    """The generalised winding number of every point in float64: sum of the triangles' signed solid angles
    over 4 pi (1 inside a closed outward-wound mesh, 0 outside)."""
    t = np.asarray(v, np.float64)[np.asarray(idx, np.int64)]
    p = np.asarray(points, np.float64)
    out = np.empty(len(p))
    for lo in range(0, len(p), 256):
        q = p[lo:lo + 256, None, :]
        a, b, c = t[None, :, 0] - q, t[None, :, 1] - q, t[None, :, 2] - q
        la, lb, lc = (np.linalg.norm(x, axis=-1) for x in (a, b, c))
        det = (a * np.cross(b, c)).sum(-1)
        den = la * lb * lc + (a * b).sum(-1) * lc + (b * c).sum(-1) * la + (c * a).sum(-1) * lb
        out[lo:lo + 256] = (2.0 * np.arctan2(det, den)).sum(1) / (4.0 * np.pi)
    return out


def sign_points(v, idx, n=2000, seed=5):
    """n seeded float32 points: half uniform in the mesh's box grown by half its extent, a quarter each
    within 5 % of the extent around vertices and around points of edges; rejection-sampled so that the
    float64 brute-force distance to the mesh is at least 1e-3 of the extent."""
    rng = np.random.default_rng(seed)
    vv = np.asarray(v, np.float64)
    lo, hi = vv.min(0), vv.max(0)
    ext = float(np.linalg.norm(hi - lo))
    e = directed_edges(idx)
    tris = triangles_of(v, idx)
    got = []
    have = 0
    while have < n:
        m = 2 * n
        kind = np.arange(m) % 4
        p = rng.uniform(lo - 0.5 * (hi - lo), hi + 0.5 * (hi - lo), (m, 3))
        d = rng.normal(size=(m, 3))
        d *= (0.05 * ext * rng.uniform(0.0, 1.0, m) ** (1.0 / 3.0) / np.linalg.norm(d, axis=1))[:, None]
        at_v = vv[rng.integers(0, len(vv), m)]
        pick = e[rng.integers(0, len(e), m)]
        w = rng.uniform(0.0, 1.0, (m, 1))
        at_e = vv[pick[:, 0]] * (1.0 - w) + vv[pick[:, 1]] * w
        p[kind == 2] = (at_v + d)[kind == 2]
        p[kind == 3] = (at_e + d)[kind == 3]
        p = np.ascontiguousarray(p, F)
        keep = brute_distance64(tris, p) >= 1e-3 * ext
        got.append(p[keep])
        have += int(keep.sum())
    return np.ascontiguousarray(np.concatenate(got)[:n], F)


def host_answers(rtx, v, idx, points, max_distance=float("inf")):
    """(records (n, 8) float32, signed (n, 4) float32) of the host rule over all triangles of the mesh."""
    table = rtx.pseudo_normals(v, idx)
    rec = rtx.closest_points_host(triangles_of(v, idx), points, max_distance=max_distance)
    return rec, rtx.signed_distance_rule(points, rec, v, idx, table)


def sign64(v, idx, points):
    """The rule restated in float64, end to end: Ericson's region walk for every (point, triangle) pair, the
    smallest (d2, index), the rule64 entry of the winning feature (the unit normal for a face), and whether
    dot(N, p - c) < 0.  Returns inside (n,) bool."""
    t = np.asarray(v, np.float64)[np.asarray(idx, np.int64)]
    p = np.asarray(points, np.float64)[:, None, :]
    table, _ = rule64(v, idx)
    unit, _ = unit_normals64(v, idx)
    a, b, c = t[None, :, 0], t[None, :, 1], t[None, :, 2]
    ab, ac = b - a, c - a
    dot = lambda x, y: (x * y).sum(-1)  # noqa: E731
    d1, d2 = dot(ab, p - a), dot(ac, p - a)
    d3, d4 = dot(ab, p - b), dot(ac, p - b)
    d5, d6 = dot(ab, p - c), dot(ac, p - c)
    vc, vb, va = d1 * d4 - d3 * d2, d5 * d2 - d1 * d6, d3 * d6 - d5 * d4
    with np.errstate(all="ignore"):
        conds = [(d1 <= 0) & (d2 <= 0), (d3 >= 0) & (d4 <= d3), (vc <= 0) & (d1 >= 0) & (d3 <= 0), (d6 >= 0) & (d5 <= d6),
                 (vb <= 0) & (d2 >= 0) & (d6 <= 0), (va <= 0) & (d4 - d3 >= 0) & (d5 - d6 >= 0)]
        feats = [1, 2, 4, 3, 6, 5]
        t12, t31, t23 = d1 / (d1 - d3), d2 / (d2 - d6), (d4 - d3) / ((d4 - d3) + (d5 - d6))
        r = 1.0 / (va + vb + vc)
        z, o = np.zeros_like(d1), np.ones_like(d1)
        weights = [(o, z, z), (z, o, z), (1 - t12, t12, z), (z, z, o), (1 - t31, z, t31), (z, 1 - t23, t23)]
        face = (1 - vb * r - vc * r, vb * r, vc * r)
    feature = np.zeros(d1.shape, np.int64)
    wa, wb, wc = face
    done = np.zeros(d1.shape, bool)
    for cond, f, (xa, xb, xc) in zip(conds, feats, weights):
        take = cond & ~done
        feature = np.where(take, f, feature)
        wa, wb, wc = np.where(take, xa, wa), np.where(take, xb, wb), np.where(take, xc, wc)
        done |= cond
    cp = a * wa[..., None] + b * wb[..., None] + c * wc[..., None]
    d = p - cp
    dd = dot(d, d)
    dd = np.where(np.isnan(dd), np.inf, dd)
    win = dd.argmin(1)  # the first of equal minima: the lowest index
    k = np.arange(len(win))
    f = feature[k, win]
    N = np.where((f == 0)[:, None], unit[win], table[win, np.maximum(f, 1) - 1])
    return (N * d[k, win]).sum(-1) < 0
