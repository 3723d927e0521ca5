"""The inputs of tests/test_gpu_traversal_limits.py reach the traversal's limits, on the CPU oracle:
which share of limit_scenes' rays fills the 16-entry stack, drops a push and ends at the 1,024-
iteration cap (the maxDepth, droppedPushes and iterations fields of oracle.intersect).  The bounds are
conditions on the inputs, about half of the measured shares, so that the GPU tests cannot quietly
stop reaching the limits.

Measured (hit, >= 11 entries, 16 entries, dropped > 0, 1024 iterations):
  chain31,   chain_rays(4096, 3)   1.00  1.00  0.51   0.32 (at most 6 a ray)   0
  chain1201, the same rays         1.00  1.00  0.35   0.28 (at most 97)        1.00
  chain31,   camera, fov 20        1.00  1.00  0.78   0.62                     0
  chain31,   camera, fov 90        0.72  0.44  0.068  0.036                    0
  chain1201, camera, fov 20 / 90   1.00 / 0.72  1.00 / 0.45  0.60 / 0.064  0.52 / 0.048  1.00 / 0.74
  chain1201, corner camera         1.00  0.40  0.208  0.207 (at most 7)       0.20
  ... its rays reflected           0     0.80  0.80   0.80                    1.00

The rays that end at no limit equal float64 brute force (bvh_check.brute_force_hits) within
test_bvh_duplicates.T_RTOL; of those that end at one, some report a hit farther than the closest:
the limits are visible in the answer, so the kernels must reproduce them exactly."""
import numpy as np
import pytest

from bvh_check import brute_force_hits, tree_triangles
from limit_scenes import (FOV_NARROW, FOV_WIDE, H, W, chain1201, chain31, chain_rays, limit_camera, limits, mirror_rays,
                          share_text, shares)
from mesh_scenes import pad_indices
from test_bvh_duplicates import T_RTOL, build


@pytest.fixture(scope="module")
def built(oracle):
    cache = {}

    def get(name):
        if name not in cache:
            v, idx = {"chain31": chain31, "chain1201": chain1201}[name]()
            cache[name] = (v, idx, build(oracle, v, idx))
        return cache[name]
    return get


@pytest.fixture(scope="module")
def rays():
    r = chain_rays(4096, 3)
    r.setflags(write=False)
    return r


def test_the_meshes_are_what_they_are_named_for(built):
    v, idx, ob = built("chain31")
    assert len(idx) == 31 and len(v) == 93 and ob["batch_count"] == 1
    v, idx, ob = built("chain1201")
    assert len(idx) == 1201 and ob["batch_count"] == 2 and len(pad_indices(idx)) == 1204


def test_chain_rays_reach_the_stack_limits(oracle, built, rays):
    """chain31: half of the rays fill the stack, a third drops a push, none reaches the cap, and a
    third ends at no limit at all."""
    o = oracle.intersect(built("chain31")[2], rays)
    s = shares(o)
    print(share_text("chain31, chain_rays(4096, 3)", s))
    full, drop, cap = limits(o)
    assert s["full"] >= 0.25 and s["drop"] >= 0.15
    assert (~(drop | cap)).mean() >= 0.3


def test_chain_rays_reach_the_iteration_cap(oracle, built, rays):
    """chain1201: every ray ends at the 1,024-iteration cap, a quarter of them with dropped pushes."""
    o = oracle.intersect(built("chain1201")[2], rays)
    s = shares(o)
    print(share_text("chain1201, chain_rays(4096, 3)", s))
    assert s["cap"] >= 0.9 and s["drop"] >= 0.14


def test_camera_rays_reach_the_limits(oracle, built):
    """The camera of the GPU frames: at 20 degrees most rays fill the stack and drop pushes; at 90
    degrees limits, plain hits and misses lie side by side."""
    ob = built("chain31")[2]
    cam, _ = limit_camera(None, oracle, FOV_NARROW)
    prim, _ = oracle.primary_rays(W, H, 1, cam=cam)
    o = oracle.intersect(ob, prim)
    s = shares(o)
    print(share_text("chain31, camera fov 20", s))
    assert s["full"] >= 0.4 and s["drop"] >= 0.3
    cam, _ = limit_camera(None, oracle, FOV_WIDE)
    prim, _ = oracle.primary_rays(W, H, 1, cam=cam)
    o = oracle.intersect(ob, prim)
    s = shares(o)
    print(share_text("chain31, camera fov 90", s))
    full, drop, cap = limits(o)
    assert s["drop"] > 0 and 1.0 - s["hit"] >= 0.1
    assert (~(drop | cap)).mean() >= 0.3
    ob = built("chain1201")[2]
    for fov, name in ((FOV_NARROW, "20"), (FOV_WIDE, "90")):
        cam, _ = limit_camera(None, oracle, fov)
        prim, _ = oracle.primary_rays(W, H, 1, cam=cam)
        print(share_text("chain1201, camera fov " + name, shares(oracle.intersect(ob, prim))))


def test_hit_barycentrics_are_the_closest_hits_own(oracle, built, rays):
    """oracle.intersect_uv's (hitU, hitV), which the GPU tests compare the hit records with: with them
    every record is a point of its triangle on the ray, |org + t dir - P(tri, hitU, hitV)| within 16 x 2^-23 x
    the largest |org| + t (rounding of a point computed from coordinates of that size).  The u / v fields
    (HitInfo's, overwritten by every triangle test that passes) are another triangle's for some rays: the
    three triangles of a group are coplanar and tie in t, and their points lie 2 sqrt(2) and more apart."""
    from test_gpu_ray_query import residual

    for name in ("chain31", "chain1201"):
        ob = built(name)[2]
        o, uv = oracle.intersect_uv(ob, rays)
        assert o.tobytes() == oracle.intersect(ob, rays).tobytes()  # the same hits either way
        hit_u, hit_v = np.ascontiguousarray(uv[:, 0]), np.ascontiguousarray(uv[:, 1])
        assert (o["hit"] == 1).all()
        corners = ob["triangles"].reshape(-1, 6, 3)[:, :3].astype(np.float64)
        org, d = rays[:, :3], rays[:, 3:]
        bound = 16.0 * 2.0 ** -23 * float((np.linalg.norm(org.astype(np.float64), axis=1) + o["t"]).max())

        def res(u, v):
            rec = np.stack([o["t"].view(np.uint32), o["objectIdx"].view(np.uint32), u.view(np.uint32), v.view(np.uint32)], axis=1)
            return residual(org, d, rec, corners)
        own, last = res(hit_u, hit_v), res(o["u"], o["v"])
        print("%s: largest residual with hitU / hitV %.3g (bound %.3g); with u / v %d rays over 1, largest %.3g"
              % (name, own.max(), bound, (last > 1.0).sum(), last.max()))
        assert own.max() <= bound
        assert (last > 1.0).any()
        same = last <= bound  # where u / v are the hit's own, the two pairs are the same bits
        assert np.array_equal(o["u"][same].view(np.uint32), hit_u[same].view(np.uint32))
        assert np.array_equal(o["v"][same].view(np.uint32), hit_v[same].view(np.uint32))


def test_corner_camera_sends_bounce_rays_to_the_limits(oracle, built):
    """The second camera of the GPU frames (limit_camera's "corner" view) on chain1201: a fifth of its
    own rays fills the stack and drops pushes, and so do four fifths of their mirror reflections, which
    stand for the rays the shading kernels trace themselves (measured: 0.208 / 0.207 and 0.800; the
    bounds are half of that).  From the front camera no reflection holds more than ten entries."""
    ob = built("chain1201")[2]
    cam, _ = limit_camera(None, oracle, FOV_NARROW, "corner")
    prim, _ = oracle.primary_rays(W, H, 1, cam=cam)
    o = oracle.intersect(ob, prim)
    s = shares(o)
    print(share_text("chain1201, corner camera", s))
    assert s["hit"] >= 0.99 and s["full"] >= 0.1 and s["drop"] >= 0.1
    b = oracle.intersect(ob, mirror_rays(prim, o))
    full, drop, cap = limits(b)
    print(share_text("chain1201, corner camera, reflected", shares(b)))
    assert (full & drop).mean() >= 0.4
    cam, _ = limit_camera(None, oracle, FOV_NARROW)
    prim, _ = oracle.primary_rays(W, H, 1, cam=cam)
    b = oracle.intersect(ob, mirror_rays(prim, oracle.intersect(ob, prim)))
    assert shares(b)["deep"] == 0.0


def test_the_limits_change_answers_and_nothing_else_does(oracle, built, rays):
    """chain31 against float64 brute force.  The rays that end at no limit: hit or miss agrees and t
    agrees within T_RTOL (measured: 2.9e-7 relative); the rays left out are exactly those at a limit,
    at most 0.75 of the set (twice the measured 0.32).  Of the rays at a limit at least one reports a t
    more than T_RTOL beyond brute force's (measured: 53 % of them, by up to 1.9e-3 relative)."""
    v, idx, ob = built("chain31")
    o = oracle.intersect(ob, rays)
    leaves = tree_triangles(ob["reorder"], len(idx))
    t, _, _ = brute_force_hits(v[pad_indices(idx)[leaves]], rays[:, :3], rays[:, 3:], T_RTOL)
    full, drop, cap = limits(o)
    skip = drop | cap
    assert skip.mean() <= 0.75
    keep = ~skip
    hit = np.isfinite(t)
    assert np.array_equal(o["hit"][keep] == 1, hit[keep])
    rel = (o["t"].astype(np.float64) - t) / np.where(hit, t, 1.0)
    both = hit & (o["hit"] == 1)
    far = skip & both & (rel > T_RTOL)
    print("chain31: %d of %d rays at no limit, largest relative t difference %.3g; of the %d at a limit %d report a "
          "farther hit, by up to %.3g" % (keep.sum(), len(rays), np.abs(rel[keep & both]).max(), skip.sum(), far.sum(),
                                          rel[skip & both].max()))
    assert (keep & both).sum() >= 0.25 * len(rays)
    assert (np.abs(rel[keep & both]) <= T_RTOL).all(), np.abs(rel[keep & both]).max()
    assert far.any()
