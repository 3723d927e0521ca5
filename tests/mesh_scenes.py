"""Meshes and expectations of the mesh-replacement tests (rt_set_mesh / rt_set_mesh_device).

Every expectation is numpy's or the oracle's: the adjacency is a stable argsort of the corners by
vertex id, its inverse, and the cumulated bincount."""
import numpy as np

from material_scenes import CUBE_QUADS


def pad_indices(idx):
    """(n, 3) -> ((n + 3) & ~3, 3), padded with index 0 as a meshFile's are (init.cu:104-115)."""
    idx = np.ascontiguousarray(idx, np.uint32).reshape(-1, 3)
    pad = (len(idx) + 3) // 4 * 4
    return np.concatenate([idx, np.zeros((pad - len(idx), 3), np.uint32)])


def numpy_adjacency(idx_padded, nv):
    """(adj_offsets[nv + 1], adj_corners[3 NP], corner_slots[3 NP]) by numpy alone."""
    keys = np.ascontiguousarray(idx_padded, np.uint32).reshape(-1)
    corners = np.argsort(keys, kind="stable").astype(np.uint32)
    slots = np.empty_like(corners)
    slots[corners] = np.arange(len(corners), dtype=np.uint32)
    off = np.zeros(nv + 1, np.uint32)
    off[1:] = np.cumsum(np.bincount(keys, minlength=nv)).astype(np.uint32)
    return off, corners, slots


def grid(ntri, nx=23, seed=3):
    """The first ntri triangles of a shared-vertex height field nx quads wide (valence up to 6)."""
    nz = (ntri + 2 * nx - 1) // (2 * nx)
    rng = np.random.default_rng(seed)
    h = rng.uniform(0.0, 1.0, size=(nz + 1, nx + 1)).astype(np.float32)
    zz, xx = np.meshgrid(np.arange(nz + 1, dtype=np.float32), np.arange(nx + 1, dtype=np.float32), indexing="ij")
    v = np.stack([xx * np.float32(0.5), h, zz * np.float32(0.5)], axis=-1).reshape(-1, 3)
    at = lambda z, x: z * (nx + 1) + x  # noqa: E731
    idx = []
    for z in range(nz):
        for x in range(nx):
            a, b, c, d = at(z, x), at(z, x + 1), at(z + 1, x + 1), at(z + 1, x)
            idx += [(a, c, b), (a, d, c)]
    return np.ascontiguousarray(v, np.float32), np.asarray(idx[:ntri], np.uint32)


def soup2():
    """2 soup triangles: 2 padding triangles follow, whose 6 corners end vertex 0's run."""
    v = np.asarray([(0, 0, 0), (1, 0, 0), (0, 1, 0), (0, 0, 1), (1, 0, 1), (0, 1, 1)], np.float32)
    return v, np.arange(6, dtype=np.uint32).reshape(2, 3)


def fan(ntri=5000):
    """ntri triangles around one hub (vertex 0): a run far longer than a sort tile and a workgroup."""
    ang = np.arange(ntri + 1, dtype=np.float32) * np.float32(2.0 * np.pi / ntri)
    rim = np.stack([np.cos(ang), np.float32(0.3) * np.sin(np.float32(5) * ang), np.sin(ang)], axis=-1)
    v = np.concatenate([np.asarray([(0, 0.5, 0)], np.float32), rim.astype(np.float32)])
    k = np.arange(ntri, dtype=np.uint32)
    return np.ascontiguousarray(v, np.float32), np.stack([np.zeros_like(k), k + 1, k + 2], axis=-1)


def gaps():
    """A grid whose vertices sit among unreferenced ones: 5 first, 300 in the middle, 7 last."""
    v, idx = grid(600)
    nv = len(v)
    half = nv // 2
    junk = lambda n: np.full((n, 3), 9.0, np.float32)  # noqa: E731
    v2 = np.concatenate([junk(5), v[:half], junk(300), v[half:], junk(7)])
    remap = np.where(np.arange(nv) < half, np.arange(nv) + 5, np.arange(nv) + 305).astype(np.uint32)
    return np.ascontiguousarray(v2, np.float32), remap[idx]


TOP_NV = (1 << 21) + 8


def top_digit():
    """64 triangles whose indices lie just below vertex_count = 2^21 + 8: the sort's top digit."""
    v, idx = grid(64, nx=8)
    nv = len(v)
    big = np.zeros((TOP_NV, 3), np.float32)
    big[TOP_NV - nv:] = v
    return big, (idx + np.uint32(TOP_NV - nv)).astype(np.uint32)


# the smallest shapes that reach each place the sort can go wrong: the padding corners, a batch
# boundary, a run longer than a tile and a workgroup, empty runs, the top digit
SHAPES = {
    "soup2": soup2,
    "grid1023": lambda: grid(1023),
    "grid1024": lambda: grid(1024),
    "grid1025": lambda: grid(1025),
    "fan5000": fan,
    "gaps": gaps,
    "top_digit": top_digit,
}
# an order that shrinks after growing, so that a stale tail of a larger mesh would show
ORDER = ("grid1025", "soup2", "fan5000", "grid1023", "top_digit", "gaps", "grid1024", "soup2")


def stack(layers, ntri):
    """layers coincident copies of grid(ntri), each with its own vertices, layer after layer: every
    Morton key of the batch occurs layers times."""
    v, idx = grid(ntri)
    vs = np.concatenate([v] * layers)
    ids = np.concatenate([idx + np.uint32(k * len(v)) for k in range(layers)])
    return np.ascontiguousarray(vs, np.float32), np.ascontiguousarray(ids, np.uint32)


# `runs`: copies of one small triangle at sites along x.  Only x differs between the sites, so the
# sorted order is the sites' order, and 601 sites on 1023 Morton cells have distinct keys.
RUN_TRI = np.asarray([(0.0, 0.0, 0.0), (0.3, 0.05, 0.0), (0.0, 0.1, 0.3)], np.float32)
RUN_SITES = 601
# site -> copies.  Sorted positions: the runs of 3, 4 and 7 lie inside one 64-lane wave (10..12,
# 102..105, 205..211), the run of 63 fills all but one lane of a wave (320..382), the run of 64
# straddles two (473..536), those of 65 and 200 exceed one (636..700, 750..949).
RUNS = {10: 3, 100: 4, 200: 7, 309: 63, 400: 64, 500: 65, 550: 200}
RUNS_ENDS = {0: 3, 100: 4, 200: 7, 309: 63, 400: 64, 500: 65, 550: 200, 600: 5}


def runs(lengths=None, drop=0, vertex0_at=None, seed=7):
    """One batch: lengths[s] copies of RUN_TRI at site s (one copy elsewhere), in a seeded shuffle,
    each triangle with its own vertices; the first `drop` single sites stay empty.  vertex0_at: an
    extra, unreferenced vertex 0 at that site's centroid, where the padding triangles of a count
    that is no multiple of 4 then lie: they sort into that site's run."""
    lengths = RUNS if lengths is None else lengths
    sites = []
    for s in range(RUN_SITES):
        if s not in lengths and drop > 0:
            drop -= 1
            continue
        sites += [s] * lengths.get(s, 1)
    sites = np.random.default_rng(seed).permutation(np.asarray(sites))
    off = np.zeros((len(sites), 1, 3), np.float32)
    off[:, 0, 0] = sites.astype(np.float32) * np.float32(0.5)
    v = (RUN_TRI[None] + off).reshape(-1, 3)
    idx = np.arange(3 * len(sites), dtype=np.uint32).reshape(-1, 3)
    if vertex0_at is not None:
        c = (RUN_TRI[0] + RUN_TRI[1] + RUN_TRI[2]) / np.float32(3.0)
        c[0] += np.float32(vertex0_at) * np.float32(0.5)
        v, idx = np.concatenate([c[None], v]), idx + np.uint32(1)
    return np.ascontiguousarray(v, np.float32), np.ascontiguousarray(idx, np.uint32)


def speck():
    """grid(1000) shrunk to a 0.0115 x 0.011 patch (heights kept) beside one 100-unit triangle: the
    patch lies in one Morton cell of x and of z, so about half of its keys repeat; 1,001 triangles,
    so three padding triangles at vertex 0 sort among them."""
    v, idx = grid(1000)
    v = v * np.asarray([0.001, 1.0, 0.001], np.float32)
    big = np.asarray([(-50.0, -1.0, -50.0), (50.0, -1.0, -50.0), (0.0, -1.0, 50.0)], np.float32)
    n = np.uint32(len(v))
    return (np.ascontiguousarray(np.concatenate([v, big]), np.float32),
            np.concatenate([idx, np.asarray([(n, n + 1, n + 2)], np.uint32)]))


def all_equal():
    """1,024 times the same triangle, in the plane y = 0: one key, and a batch box without height."""
    v = np.asarray([(0, 0, 0), (1, 0, 0), (0, 0, 1)], np.float32)
    return v, np.tile(np.asarray([(0, 1, 2)], np.uint32), (1024, 1))


def flat(y):
    """grid(1000) with every height y: no extent on one axis, so the Morton quotient there is 0 / 0."""
    v, idx = grid(1000)
    v = v.copy()
    v[:, 1] = np.float32(y)
    return v, idx


# meshes with Morton keys that occur three times and more (one batch, the last with padding
# triangles, a degenerate batch box, equal TLAS keys on the one-wave and the workgroup path), and two
# flat meshes without duplicates
DUPLICATE_SHAPES = {
    "stack3": lambda: stack(3, 340),
    "stack5": lambda: stack(5, 204),
    "runs": runs,
    "runs_ends": lambda: runs(RUNS_ENDS, drop=4),
    "runs_pad": lambda: runs(drop=3, vertex0_at=309),
    "speck": speck,
    "all_equal": all_equal,
    "tlas3": lambda: stack(3, 1024),
    "tlas66": lambda: stack(66, 1024),
    "flat0": lambda: flat(0.0),
    "flat_neg": lambda: flat(-3.0),
}
# shrinks after growing; tlas66 (67,584 triangles) has a context of its own
DUPLICATE_ORDER = ("stack3", "tlas3", "runs", "all_equal", "speck", "runs_pad", "stack5", "flat0", "runs_ends",
                   "flat_neg", "stack3")


def welded_cube():
    """[-1, 1]^3 as material_scenes.cube_triangles lays it out (6 faces of 8 x 8 quads, 768 triangles
    in the same order) with each face's 81 vertices shared: (6 * 81 vertices, 768 index triples)."""
    q = CUBE_QUADS
    step = np.float32(2.0 / q)
    verts, idx = [], []
    for axis in range(3):
        free = [k for k in range(3) if k != axis]
        for sign in (-1.0, 1.0):
            base = len(verts)
            for a in range(q + 1):
                for b in range(q + 1):
                    p = np.zeros(3, np.float32)
                    p[axis] = sign
                    p[free[0]] = np.float32(-1.0) + step * np.float32(a)
                    p[free[1]] = np.float32(-1.0) + step * np.float32(b)
                    verts.append(p)
            at = lambda a, b: base + a * (q + 1) + b  # noqa: E731
            for a in range(q):
                for b in range(q):
                    c = (at(a, b), at(a + 1, b), at(a + 1, b + 1), at(a, b + 1))
                    idx += [(c[0], c[1], c[2]), (c[0], c[2], c[3])]
    return np.asarray(verts, np.float32), np.asarray(idx, np.uint32)
