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
