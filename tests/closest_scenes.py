"""Points and expectations of the closest-point tests (rt_closest_points_device, rt_closest_points_host).

Every expectation is the host's exhaustive evaluation of the shared rule (rtx.closest_points_host) or
float64 brute force in numpy; nothing here traverses a tree."""
import numpy as np

from bvh_check import tree_triangles

_RAYMAX = int(np.asarray([10e10], np.float32).view(np.uint32)[0])
MISS = np.asarray([_RAYMAX] * 3 + [0x7F800000, 0xFFFFFFFF, 0, 0, 0], np.uint32)  # RayMax x 3, +inf, -1, 0, 0, 0
FRONT, FOUND = 1 << 16, 1 << 17
UNIT = 2.0 ** -24


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def triangles_of(v, idx):
    """(ntri, 3, 3) float32 corners of an indexed mesh."""
    return np.ascontiguousarray(np.asarray(v, np.float32)[np.asarray(idx, np.int64)], np.float32)


def extent_of(tris):
    t = np.asarray(tris, np.float64).reshape(-1, 3)
    return float(np.linalg.norm(t.max(0) - t.min(0)))


def mixed_points(tris, n, seed=17, far=1000.0):
    """n seeded float32 points for a mesh, a quarter each: on the surface (a random point of a random
    triangle), at vertices, uniform in the mesh's box, and at `far` times the extent in random directions."""
    rng = np.random.default_rng(seed)
    t = np.asarray(tris, np.float64)
    lo, hi = t.reshape(-1, 3).min(0), t.reshape(-1, 3).max(0)
    ext = max(float(np.linalg.norm(hi - lo)), 1e-3)
    kind = np.arange(n) % 4
    pick = t[rng.integers(0, len(t), n)]
    w = rng.dirichlet((1.0, 1.0, 1.0), n)
    p = np.einsum("nk,nkc->nc", w, pick)
    p[kind == 1] = pick[kind == 1, rng.integers(0, 3)]
    p[kind == 2] = rng.uniform(lo, hi, (n, 3))[kind == 2]
    d = rng.normal(size=(n, 3))
    d /= np.linalg.norm(d, axis=1)[:, None]
    p[kind == 3] = (0.5 * (lo + hi) + far * ext * d)[kind == 3]
    return np.ascontiguousarray(p, np.float32)


def far_points(tris, n, seed=23):
    """n points at 1,000 to 100,000 times the extent, where many triangles share one fp32 d2."""
    rng = np.random.default_rng(seed)
    t = np.asarray(tris, np.float64).reshape(-1, 3)
    lo, hi = t.min(0), t.max(0)
    ext = max(float(np.linalg.norm(hi - lo)), 1e-3)
    d = rng.normal(size=(n, 3))
    d /= np.linalg.norm(d, axis=1)[:, None]
    d[::7] = np.eye(3)[rng.integers(0, 3, len(d[::7]))] * rng.choice([-1.0, 1.0], len(d[::7]))[:, None]  # along an axis
    r = ext * 10.0 ** rng.uniform(3.0, 5.0, n)
    return np.ascontiguousarray(0.5 * (lo + hi) + r[:, None] * d, np.float32)


def brute_distance64(tris, points):
    """float64 distance of every point to the nearest triangle: the minimum over the triangle's plane
    projection (where it falls inside) and its three edge segments, for all pairs at once."""
    t = np.asarray(tris, np.float64)
    p = np.asarray(points, np.float64)
    a, b, c = t[:, 0], t[:, 1], t[:, 2]
    best = np.full(len(p), np.inf)
    for lo in range(0, len(p), 64):
        q = p[lo:lo + 64, None, :]
        d2 = np.full((q.shape[0], len(t)), np.inf)
        for s, e in ((a, b), (b, c), (c, a)):
            se = (e - s)[None]
            ll = (se * se).sum(-1)
            with np.errstate(divide="ignore", invalid="ignore"):
                u = np.where(ll > 0.0, ((q - s[None]) * se).sum(-1) / ll, 0.0)
            u = np.clip(u, 0.0, 1.0)
            r = q - (s[None] + u[..., None] * se)
            d2 = np.minimum(d2, (r * r).sum(-1))
        n = np.cross(b - a, c - a)
        nn = (n * n).sum(-1)
        ok = nn > 0.0
        with np.errstate(divide="ignore", invalid="ignore"):
            h = ((q - a[None]) * n[None]).sum(-1) / np.sqrt(nn)[None]
            foot = q - h[..., None] * (n / np.sqrt(nn)[:, None])[None]
            inside = np.ones(h.shape, bool)
            for s, e in ((a, b), (b, c), (c, a)):
                inside &= (np.cross((e - s)[None], foot - s[None]) * n[None]).sum(-1) >= 0.0
        d2 = np.where(inside & ok[None], np.minimum(d2, h * h), d2)
        best[lo:lo + 64] = np.sqrt(d2.min(1))
    return best


def candidates(rt, *arrays):
    """(tris (k, 3, 3) float32, ids (k,) uint32) of a context's current build: the rows of RT_ARR_TRI_POS
    that are leaves of the tree (bvh_check.tree_triangles over RT_ARR_REORDER) and real triangles."""
    tri_count = rt.info().triCount
    pos = rt.download("TRI_POS", np.float32).reshape(-1, 3, 4)[:, :, :3]
    ids = tree_triangles(rt.download("REORDER", np.uint32), tri_count)
    ids = ids[ids < tri_count]
    return np.ascontiguousarray(pos[ids], np.float32), ids.astype(np.uint32)


def expected(rtx, rt, points, max_distance=float("inf")):
    """The records the device must give for these points on rt's current build, as (n, 8) uint32."""
    tris, ids = candidates(rt)
    return bits(rtx.closest_points_host(tris, points, ids=ids, max_distance=max_distance)).reshape(-1, 8)
