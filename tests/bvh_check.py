"""Reference-free checks of a two-level LBVH and of ray hits.

assert_valid_bvh takes the arrays in the reference layout (what oracle.build_bvh returns and what
rt.download gives) and checks that they are a tree over the right leaves with the right boxes, from
the arrays alone.  brute_force_hits is float64 Moller-Trumbore over every triangle, in numpy.  rays_for
makes the seeded ray set that the CPU and the GPU tests share."""
import numpy as np

BATCH = 1024


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _merge(l, r):
    """AABBCompact::GetMerged on 6-float rows: the reference's ternary min / max (ocommon.h fmn / fmx)."""
    out = np.empty(6, np.float32)
    out[:3] = np.where(l[:3] < r[:3], l[:3], r[:3])
    out[3:] = np.where(l[3:] > r[3:], l[3:], r[3:])
    return out


def _check_tree(nodes, cnt, leaves_want, leaf_boxes, what):
    """One tree of cnt leaves in nodes[0 .. cnt - 1): topology, leaf multiset, boxes.  leaf_boxes[k]
    is the 6-float row of leaf reference k.  Returns the root's merged box."""
    if cnt == 1:  # DESIGN.md deviation 12: (leaf 0's box, zero box), leaf 0 twice
        nd = nodes[0]
        assert (int(nd["idxLeft"]), int(nd["idxRight"]), int(nd["isLeftLeaf"]), int(nd["isRightLeaf"])) == (0, 0, 1, 1), what
        left = np.concatenate([nd["lmin"], nd["lmax"]])
        right = np.concatenate([nd["rmin"], nd["rmax"]])
        assert np.array_equal(_bits(left), _bits(leaf_boxes[0])), what
        assert np.array_equal(_bits(right), np.zeros(6, np.uint32)), what
        return _merge(left, right)
    il, ir = nodes["idxLeft"].astype(np.int64), nodes["idxRight"].astype(np.int64)
    ll, rl = nodes["isLeftLeaf"], nodes["isRightLeaf"]
    assert np.isin(ll[:cnt - 1], (0, 1)).all() and np.isin(rl[:cnt - 1], (0, 1)).all(), what
    lbox = np.concatenate([nodes["lmin"], nodes["lmax"]], axis=1)
    rbox = np.concatenate([nodes["rmin"], nodes["rmax"]], axis=1)
    seen = np.zeros(cnt - 1, bool)
    merged = {}
    leaves = []
    stack = [(0, False)]
    seen[0] = True
    while stack:
        v, done = stack.pop()
        if not done:
            stack.append((v, True))
            for leaf, c in ((rl[v], ir[v]), (ll[v], il[v])):
                if leaf:
                    assert 0 <= c < len(leaf_boxes), "%s: node %d has leaf reference %d" % (what, v, c)
                    leaves.append(int(c))
                else:
                    assert 0 <= c < cnt - 1, "%s: node %d has child node %d of %d" % (what, v, c, cnt - 1)
                    assert not seen[c], "%s: node %d is reached twice (not a tree)" % (what, c)
                    seen[c] = True
                    stack.append((int(c), False))
            continue
        for side, leaf, c, box in (("left", ll[v], il[v], lbox[v]), ("right", rl[v], ir[v], rbox[v])):
            want = leaf_boxes[c] if leaf else merged.pop(int(c))
            assert np.array_equal(_bits(box), _bits(want)), "%s: node %d %s box %s, beneath it %s" % (what, v, side, box, want)
        merged[v] = _merge(lbox[v], rbox[v])
    assert seen.all(), "%s: %d of %d nodes are not reached from the root" % (what, int((~seen).sum()), cnt - 1)
    assert sorted(leaves) == sorted(int(x) for x in leaves_want), "%s: the leaves are not the sorted order's first %d" % (what, cnt)
    return merged[0]


def assert_valid_bvh(nodes, reorder, aabbs, tlas_nodes, tlas_reorder, tlas_aabbs, tri_count):
    """Every BLAS batch and the TLAS are trees: from node 0 each of the cnt - 1 nodes is met once, the
    leaf references are the multiset reorder[:cnt], every child box is, bit for bit, the leaf's AABBS
    row or the min / max merge of everything beneath the child, each TLAS leaf box is its batch root's
    merged box, and a one-leaf tree has the form of deviation 12."""
    B = (tri_count + BATCH - 1) // BATCH
    aabbs = np.ascontiguousarray(aabbs, np.float32).reshape(-1, 6)
    tlas_aabbs = np.ascontiguousarray(tlas_aabbs, np.float32).reshape(-1, 6)
    assert len(tlas_nodes) >= max(B - 1, 1) and len(tlas_aabbs) >= B
    for b in range(B):
        start = b * BATCH
        cnt = BATCH if b < B - 1 else tri_count - (B - 1) * BATCH
        root = _check_tree(nodes[start:start + BATCH], cnt, reorder[start:start + cnt], aabbs[start:start + BATCH],
                           "BLAS %d" % b)
        assert np.array_equal(_bits(tlas_aabbs[b]), _bits(root)), "TLAS leaf box %d is not its batch root's" % b
    _check_tree(tlas_nodes, B, tlas_reorder[:B], tlas_aabbs[:B], "TLAS")


def tree_triangles(reorder, tri_count):
    """Global indices of the triangles that are leaves: reorder[:cnt] of every batch (padding
    triangles that sort among the real ones take the places of the last real ones)."""
    B = (tri_count + BATCH - 1) // BATCH
    out = []
    for b in range(B):
        cnt = BATCH if b < B - 1 else tri_count - (B - 1) * BATCH
        out.append(b * BATCH + np.asarray(reorder[b * BATCH:b * BATCH + cnt], np.int64))
    return np.unique(np.concatenate(out))


def brute_force_hits(tris, org, dir, rtol=0.0):
    """float64 Moller-Trumbore of every ray against every triangle (tris: (n, 3, 3)), two-sided, t >= 0.
    Returns (t, tie, gap): per ray the smallest t (inf: no hit), a boolean (rays, n) matrix of the
    triangles whose t is within rtol * t of it, and the relative distance from it to the nearest t
    outside that set (inf: none)."""
    tris = np.asarray(tris, np.float64)
    org, dir = np.asarray(org, np.float64), np.asarray(dir, np.float64)
    v0, e1, e2 = tris[:, 0], tris[:, 1] - tris[:, 0], tris[:, 2] - tris[:, 0]
    R, n = len(org), len(tris)
    tt = np.full((R, n), np.inf)
    for lo in range(0, R, 64):  # blocks of rays keep the (rays, n, 3) temporaries small
        o, d = org[lo:lo + 64, None, :], dir[lo:lo + 64, None, :]
        p = np.cross(d, e2[None])
        det = np.einsum("rnk,nk->rn", p, e1)
        with np.errstate(divide="ignore", invalid="ignore"):
            inv = 1.0 / det
            s = o - v0[None]
            u = np.einsum("rnk,rnk->rn", s, p) * inv
            q = np.cross(s, e1[None])
            v = np.einsum("rnk,rnk->rn", np.broadcast_to(d, q.shape), q) * inv
            t = np.einsum("rnk,nk->rn", q, e2) * inv
            ok = (det != 0.0) & (u >= 0.0) & (v >= 0.0) & (u + v <= 1.0) & (t >= 0.0)
        tt[lo:lo + 64] = np.where(ok, t, np.inf)
    tmin = tt.min(axis=1)
    with np.errstate(invalid="ignore"):
        tie = np.isfinite(tt) & (tt <= (tmin * (1.0 + rtol))[:, None])
        rest = np.where(tie, np.inf, tt).min(axis=1)
        gap = np.where(np.isfinite(rest), (rest - tmin) / tmin, np.inf)
    return tmin, tie, gap


def rays_for(v, idx, n=600, seed=5):
    """n seeded rays for a mesh, (n, 6) float32 origin + unit direction: about two thirds aimed at the
    centroid of a random triangle from origins scattered around and above the mesh, a sixth of them
    from origins that share one or two coordinates with their target (direction components of exactly
    zero), and a sixth that cannot hit: they start above the mesh's box and point away from it."""
    rng = np.random.default_rng(seed)
    tri = np.asarray(v, np.float64)[np.asarray(idx, np.int64)]
    # the extent of where the triangles are (1st to 99th percentile of the corners), not of the box: the
    # fp32 triangle test resolves a triangle of width w from a distance d to about 1e-7 d / w of its
    # barycentrics, so rays started a lone large triangle's length away from a patch of small ones
    # would land on a neighbour of the triangle that float64 finds
    lo, hi = np.percentile(tri.reshape(-1, 3), 1.0, axis=0), np.percentile(tri.reshape(-1, 3), 99.0, axis=0)
    size = float(np.linalg.norm(hi - lo))
    mid = 0.5 * (lo + hi)
    target = tri[rng.integers(0, len(tri), n)].mean(axis=1)
    org = mid + rng.uniform(-1.0, 1.0, (n, 3)) * size * np.asarray([0.8, 0.0, 0.8])
    org[:, 1] = hi[1] + rng.uniform(0.2, 1.5, n) * size
    kind = rng.integers(0, 6, n)
    ax = kind == 0
    two = ax & (rng.integers(0, 2, n) == 0)
    org[ax, 0] = target[ax, 0]  # dir.x == 0
    org[two, 2] = target[two, 2]  # ... and dir.z == 0: straight down
    d = target - org
    away = kind == 1
    d[away] = org[away] - mid
    d[away, 1] = np.abs(d[away, 1]) + 0.1 * size
    org32, tgt32 = org.astype(np.float32), (org + d).astype(np.float32)
    d32 = tgt32 - org32
    d32[ax, 0] = 0.0
    d32[two, 2] = 0.0
    d32 /= np.linalg.norm(d32.astype(np.float64), axis=1)[:, None].astype(np.float32)
    return np.ascontiguousarray(np.concatenate([org32, d32], axis=1), np.float32)
