"""Meshes, rays and cameras that drive the traversal to the reference's three limits (TraverseBvh,
csrc/traverse.h trav_step): the 16-entry stack, the push onto a full stack that is dropped, and the
1,024-iteration cap.

chain(S, c, reps) is a mesh whose LBVH is a chain about 30 levels deep with every box around the
middle of the stack: a ray through the middle finds both children hit at every level, so its stack
fills.  tests/test_traversal_limits.py pins, on the CPU oracle, which share of chain_rays and of the
camera's rays reaches which limit; tests/test_gpu_traversal_limits.py runs the same inputs through
every traversal kernel."""
import math

import numpy as np

W, H = 96, 54
DEG = np.float32(0.01745329251)
FOV_NARROW = np.float32(20.0) * DEG  # every camera ray meets the stack of triangles
FOV_WIDE = np.float32(90.0) * DEG    # the default: hits, misses and rays at no limit side by side
D = np.full(3, 1.0 / math.sqrt(3.0))  # the triangles' normal, and the way the rays travel
# the way a mirror sends the corner camera's line of sight on: the normal leant by 1.5 towards (-2,1,1)
CORNER_OUT = D + 1.5 * np.asarray([-2.0, 1.0, 1.0]) / math.sqrt(6.0)
CORNER_OUT /= np.linalg.norm(CORNER_OUT)


def chain(S, c, reps):
    """1 + 30 reps triangles, each with its own vertices.  The base triangle (S,0,0), (0,S,0), (0,0,S)
    less S/3 per component has the normal (1,1,1) and its centroid at 0; after it, for i = 0..9 and
    axis a = 0..2, reps coincident copies of it moved by c 2^i along a.  The centroids differ in one
    Morton bit each, so every split of the LBVH takes one group off: a chain.  float64, rounded once."""
    base = np.asarray([(S, 0.0, 0.0), (0.0, S, 0.0), (0.0, 0.0, S)], np.float64) - S / 3.0
    tris = [base]
    for i in range(10):
        for a in range(3):
            off = np.zeros(3)
            off[a] = c * 2.0 ** i
            tris += [base + off] * reps
    v = np.concatenate(tris).astype(np.float32)
    idx = np.arange(len(v), dtype=np.uint32).reshape(-1, 3)
    return np.ascontiguousarray(v), idx


def chain31():
    """31 triangles, one batch."""
    return chain(4096.0, 2.0, 1)


def chain1201():
    """1,201 triangles: two batches, so the stack holds TLAS and BLAS words together, and three
    padding triangles; the forty coincident copies per group keep every ray going to the 1,024 cap."""
    return chain(4096.0, 1.0, 40)


def chain_rays(n, seed, spread=100.0):
    """(n, 6) float32 origin + unit direction: rays along (1,1,1) from 3,000 units in front of the
    stack, aimed at points scattered around its middle and up to 300 along the diagonal, the origins
    jittered by 50 so that no two are parallel.  Normalised as test_gpu_ray_query.make_rays does."""
    rng = np.random.default_rng(seed)
    target = rng.uniform(-spread, spread, (n, 3)) + rng.uniform(0.0, 300.0, (n, 1))
    origin = target - 3000.0 * D + rng.uniform(-50.0, 50.0, (n, 3))
    org = origin.astype(np.float32)
    d = target.astype(np.float32) - org
    d /= np.linalg.norm(d, axis=1, keepdims=True).astype(np.float32)
    assert org.dtype == np.float32 and d.dtype == np.float32
    return np.ascontiguousarray(np.concatenate([org, d], axis=1), np.float32)


def limit_camera(rtx, oracle, fov=FOV_NARROW, view="front", w=W, h=H):
    """(oracle CameraIn, rtx.Camera).  rtx None: the oracle's camera only (the CPU test).

    view "front": 3,000 units in front of the stack, looking along (1,1,1) at the point (150, 150, 150).
    Its camera rays reach the limits; the rays that leave the surfaces do not: they start in the middle
    of every box, where all box distances tie at zero, and travel away from the stack.

    view "corner": 1,500 units behind the stack, looking back at a point 15 % inside the triangles' +x
    corner, from the side: the mirror image of its line of sight in the triangles' plane, CORNER_OUT,
    leans from the normal towards (-2,1,1).  A surface there lies outside the boxes of the groups moved
    along y and z, and a ray that leaves it along CORNER_OUT crosses those boxes one after the other, so
    the rays leaving the surfaces fill the stack too (mirror_rays; chain1201 only: chain31's groups of
    one triangle never do)."""
    if view == "front":
        pos = tuple(float(np.float32(150.0 - 3000.0 * k)) for k in D)
        yaw, pitch = float(np.float32(math.pi / 4.0)), 0.6155
    else:
        s = 4096.0
        target = 0.85 * np.asarray([2.0 * s / 3.0, -s / 3.0, -s / 3.0])
        look = CORNER_OUT - 2.0 * np.dot(CORNER_OUT, D) * D  # from the camera to the surface
        pos = tuple(float(np.float32(k)) for k in target - 1500.0 * look)
        yaw, pitch = float(np.float32(math.atan2(look[0], look[2]))), float(np.float32(math.asin(look[1])))
    c = oracle.default_camera(w, h)
    c.pos[:] = pos
    c.yaw, c.pitch, c.fovX = yaw, pitch, fov
    if rtx is None:
        return c, None
    r = rtx.Camera()
    r.pos[:] = pos
    r.yaw, r.pitch, r.focal, r.aperture, r.fovX = yaw, pitch, c.focal, c.aperture, fov
    return c, r


def mirror_rays(prim, o):
    """The camera rays `prim` that hit (o: their oracle.intersect result), reflected at the hit about
    the oracle's normal and started one hundredth off the surface: a mirror's first bounce up to where
    exactly the renderer starts it.  The renderer traces those inside its shading kernel and the oracle
    keeps no statistics of them; this stands in for them where a test shows what such rays reach."""
    hit = o["hit"] == 1
    n = o["normal"][hit].astype(np.float64)
    d = prim[hit, 3:6].astype(np.float64)
    out = d - 2.0 * (d * n).sum(axis=1, keepdims=True) * n
    org = o["pos"][hit].astype(np.float64) + 0.01 * n
    return np.ascontiguousarray(np.concatenate([org, out], axis=1), np.float32)


def limits(o):
    """Per ray of an oracle.intersect result: stack full (16 entries), a push dropped, the iteration cap."""
    return o["maxDepth"] >= 16, o["droppedPushes"] > 0, o["iterations"] >= 1024


def shares(o):
    """hit, >= 11 entries (past the camera kernels' LDS part), 16 entries, dropped > 0, at the cap."""
    full, drop, cap = limits(o)
    return dict(hit=float((o["hit"] == 1).mean()), deep=float((o["maxDepth"] >= 11).mean()), full=float(full.mean()),
                drop=float(drop.mean()), cap=float(cap.mean()), max_drop=int(o["droppedPushes"].max()))


def share_text(name, s):
    return "%s: hit %.3f, >= 11 entries %.3f, 16 entries %.3f, dropped %.3f (at most %d a ray), 1024 iterations %.3f" % (
        name, s["hit"], s["deep"], s["full"], s["drop"], s["max_drop"], s["cap"])
