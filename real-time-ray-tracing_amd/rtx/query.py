"""Device ray queries on torch tensors (rt_trace_rays_device, rt_trace_surfaces_device, include/rtx_amd.h).

``trace(rt, origins, directions)`` traces n rays that live in device tensors against the BVH of the
last ``build_bvh`` / draw and returns their hit records as a device tensor, without a host
synchronisation and without a copy of the inputs: visibility, line of sight, picking, collision and
ray-cast sensors against geometry the host animates on the device (``update_vertices_device``).

``trace(..., surface=True)`` also returns what the hits hit, one surface record per ray: the
re-projected hit point and the reference's ray offset, the geometric and the shading normal, the
material id, front face and hit flags, and with ``motion=True`` the hit point's displacement since the
build before (views: ``position`` .. ``is_hit``).  ``surfaces(rt, origins, directions, hits)`` computes
the same records from the hit records of an earlier query, without a traversal.  ``spawn_origins``
gives the origins of secondary rays, so that query -> surfaces -> second query runs on the device.

``closest(rt, points)`` answers the proximity question no ray does: per point the nearest triangle of
the current build and the nearest point on it (rt_closest_points_device), one (n, 8) record per point
(views: ``closest_position`` .. ``closest_found``), for colliders, penetration depth, distance-field
sampling and placement on skinned meshes.

``signed_distance(rt, points)`` adds "inside or outside" (rt_signed_distance_device): the closest records
and one (n, 4) quad per point, the nearest feature's angle-weighted pseudo-normal and the distance,
negative inside a closed mesh (views: ``signed_distance_of``, ``pseudo_normal``, ``inside``).  It needs
``rt.signed_distance = True`` since before the current build.

The query runs on the renderer's stream (``set_stream``).  ``trace`` may be called from any torch
stream: it hands the renderer an event recorded on ``torch.cuda.current_stream()`` to wait for, and
makes that stream wait for the query's end, so tensors filled just before the call are read after
the fill and the result is ready for whatever the caller enqueues next.
"""
from __future__ import annotations


def _rays(name, x, torch):
    """Refuse what the kernel cannot read in place; returns (n, row stride in floats)."""
    if not isinstance(x, torch.Tensor):
        raise ValueError("%s must be a torch tensor" % name)
    if x.dtype != torch.float32:
        raise ValueError("%s must be float32, not %s" % (name, x.dtype))
    if x.dim() != 2 or not 3 <= x.shape[1] <= 8:
        raise ValueError("%s must have shape (n, 3..8), not %s" % (name, tuple(x.shape)))
    if x.stride(1) != 1:
        raise ValueError("%s must have a unit inner stride (xyz adjacent in memory)" % name)
    n = x.shape[0]
    stride = x.stride(0) if n > 1 else max(int(x.stride(0)), 3)
    if not 3 <= stride <= 0xFFFFFFFF:
        raise ValueError("%s: the row stride must be at least 3 floats (no broadcast or reversed rows)" % name)
    return n, int(stride)


def _dense(name, x, shape, torch):
    """An optional result tensor, or the hit records `surfaces` reads: contiguous float32 of this shape."""
    if x is not None and (not isinstance(x, torch.Tensor) or x.dtype != torch.float32 or tuple(x.shape) != shape
                          or not x.is_contiguous()):
        raise ValueError("%s must be a contiguous (n, %d) float32 tensor" % (name, shape[1]))


def _check(rt, origins, directions, dense, torch):
    """The host-checkable refusals of a query, then the device checks; returns (n, strides, device).
    dense: (name, tensor or None, columns) of the (n, columns) tensors beside the rays."""
    n, org_stride = _rays("origins", origins, torch)
    nd, dir_stride = _rays("directions", directions, torch)
    if nd != n:
        raise ValueError("origins and directions must hold the same number of rays (%d, %d)" % (n, nd))
    if n > (1 << 30):
        raise ValueError("at most 2^30 rays per query")
    for name, x, cols in dense:
        _dense(name, x, (n, cols), torch)
    for name, x in (("origins", origins), ("directions", directions)):  # the device checks come last
        if not x.is_cuda:
            raise ValueError("%s must be on the renderer's device, not on %s" % (name, x.device))
    if directions.device != origins.device or any(x is not None and x.device != origins.device for _, x, _ in dense):
        raise ValueError("origins, directions%s must be on one device" % "".join(", " + name for name, _, _ in dense))
    dev = origins.device
    dev_id = rt.info().deviceId
    if dev_id >= 0 and dev.index is not None and dev.index != dev_id:
        raise ValueError("the rays are on %s, the renderer on device %d" % (dev, dev_id))
    return n, org_stride, dir_stride, dev


def trace(rt, origins, directions, *, any_hit: bool = False, want_iters: bool = False, out=None,
          surface: bool = False, motion: bool = False, surface_out=None):
    """Hit records of the rays (origins[i, :3], directions[i, :3]).

    origins, directions: float32 device tensors of shape (n, 3..8) with a unit inner stride; the row
    stride (the leading dimension of the storage, e.g. 8 for the two halves ``rays[:, 0:3]`` and
    ``rays[:, 4:7]`` of one interleaved (n, 8) tensor) is passed on, nothing is copied.  Directions
    need not be normalised.  any_hit: each ray stops at the first hit the traversal records (same
    hit / miss answer, t >= the closest t).  out: an (n, 4) contiguous float32 tensor for the records.
    surface: also the surface records (rt_trace_surfaces_device), an (n, 12) float32 tensor, (n, 16)
    with motion (which needs surface); surface_out: a contiguous tensor of that shape for them.

    Returns hits (n, 4) float32: t (1e11 on a miss), the triangle index as int32 bits (-1), u, v (see
    ``split``); with surface (hits, surf); with want_iters also the traversal iterations per ray as an
    (n,) int32 tensor, last."""
    import torch

    if (motion or surface_out is not None) and not surface:
        raise ValueError("motion and surface_out belong to surface=True")
    cols = 16 if motion else 12
    dense = (("out", out, 4),) + ((("surface_out", surface_out, cols),) if surface else ())
    n, org_stride, dir_stride, dev = _check(rt, origins, directions, dense, torch)
    cur = torch.cuda.current_stream(dev)
    with torch.cuda.device(dev):
        hits = out if out is not None else torch.empty((n, 4), dtype=torch.float32, device=dev)
        iters = torch.empty(n, dtype=torch.int32, device=dev) if want_iters else None
        surf = None
        if surface:
            surf = surface_out if surface_out is not None else torch.empty((n, cols), dtype=torch.float32, device=dev)
        ready, done = torch.cuda.Event(), torch.cuda.Event()
        ready.record(cur)
        done.record(cur)  # creates the handle; the renderer records it again behind the kernel
        kw = dict(org_stride=org_stride, dir_stride=dir_stride, iters_ptr=iters.data_ptr() if want_iters else None,
                  any_hit=any_hit, ready_event=ready.cuda_event, done_event=done.cuda_event)
        if surface:
            rt.trace_surfaces_device(origins.data_ptr(), directions.data_ptr(), n, hits.data_ptr(), surf.data_ptr(),
                                     motion=motion, **kw)
        else:
            rt.trace_rays_device(origins.data_ptr(), directions.data_ptr(), n, hits.data_ptr(), **kw)
        cur.wait_event(done)
    res = (hits,) + ((surf,) if surface else ()) + ((iters,) if want_iters else ())
    return res if len(res) > 1 else hits


def surfaces(rt, origins, directions, hits, *, motion: bool = False, out=None):
    """Surface records of rays whose hit records exist (RT_SURFACE_FROM_HITS): no traversal.

    hits: the contiguous (n, 4) float32 records of an earlier query of the same rays on the build that is
    current now (that it is the same build is the caller's responsibility); the rays as in ``trace``.
    out: a contiguous (n, 12) float32 tensor, (n, 16) with motion.  Returns the records."""
    import torch

    cols = 16 if motion else 12
    if hits is None:
        raise ValueError("hits must be a contiguous (n, 4) float32 tensor")
    n, org_stride, dir_stride, dev = _check(rt, origins, directions, (("hits", hits, 4), ("out", out, cols)), torch)
    cur = torch.cuda.current_stream(dev)
    with torch.cuda.device(dev):
        surf = out if out is not None else torch.empty((n, cols), dtype=torch.float32, device=dev)
        ready, done = torch.cuda.Event(), torch.cuda.Event()
        ready.record(cur)
        done.record(cur)  # creates the handle; the renderer records it again behind the kernel
        rt.trace_surfaces_device(origins.data_ptr(), directions.data_ptr(), n, hits.data_ptr(), surf.data_ptr(),
                                 org_stride=org_stride, dir_stride=dir_stride, from_hits=True, motion=motion,
                                 ready_event=ready.cuda_event, done_event=done.cuda_event)
        cur.wait_event(done)
    return surf


def closest(rt, points, *, max_distance: float = float("inf"), out=None):
    """Closest-point records of the points (points[i, :3]) against the build that is current now.

    points: a float32 device tensor of shape (n, 3..8) with a unit inner stride, read in place as the
    rays of ``trace`` are.  max_distance: >= 0 or inf; a point with nothing within it gets the miss
    record.  out: a contiguous (n, 8) float32 tensor for the records.

    Returns (n, 8) float32: the closest point (1e11 x 3 on a miss), the squared distance (inf), the
    triangle index as int32 bits (-1), u, v (the weights of the triangle's first two vertices) and the
    feature / front / found word (see the ``closest_*`` views).  Same event protocol as ``trace``."""
    import torch

    n, stride = _rays("points", points, torch)
    if n > (1 << 30):
        raise ValueError("at most 2^30 points per query")
    if not max_distance >= 0.0:
        raise ValueError("max_distance must be >= 0 or inf")
    _dense("out", out, (n, 8), torch)
    if not points.is_cuda:
        raise ValueError("points must be on the renderer's device, not on %s" % points.device)
    dev = points.device
    if out is not None and out.device != dev:
        raise ValueError("points, out must be on one device")
    dev_id = rt.info().deviceId
    if dev_id >= 0 and dev.index is not None and dev.index != dev_id:
        raise ValueError("the points are on %s, the renderer on device %d" % (dev, dev_id))
    cur = torch.cuda.current_stream(dev)
    with torch.cuda.device(dev):
        rec = out if out is not None else torch.empty((n, 8), dtype=torch.float32, device=dev)
        ready, done = torch.cuda.Event(), torch.cuda.Event()
        ready.record(cur)
        done.record(cur)  # creates the handle; the renderer records it again behind the kernel
        rt.closest_points_device(points.data_ptr(), n, rec.data_ptr(), stride=stride, max_distance=max_distance,
                                 ready_event=ready.cuda_event, done_event=done.cuda_event)
        cur.wait_event(done)
    return rec


def signed_distance(rt, points, *, max_distance: float = float("inf"), out=None, signed_out=None, records=None):
    """Closest-point records and signed distances of the points against the build that is current now.

    points, max_distance, out: as ``closest``.  signed_out: a contiguous (n, 4) float32 tensor for the
    quads.  records: the contiguous (n, 8) records of an earlier query of the same points on the build
    that is current now (that it is the same build is the caller's responsibility): nothing descends,
    only the sign pass runs (RT_DISTANCE_FROM_RECORDS), and they are returned as they are; out must then
    be None.  The renderer's ``signed_distance`` must have been on since before the current build.

    Returns (records (n, 8), signed (n, 4)): the nearest feature's pseudo-normal, not normalised, and the
    distance, negative where the point lies behind it; (0, 0, 0, inf) on a miss.  Same event protocol
    as ``trace``."""
    import torch

    n, stride = _rays("points", points, torch)
    if n > (1 << 30):
        raise ValueError("at most 2^30 points per query")
    if not max_distance >= 0.0:
        raise ValueError("max_distance must be >= 0 or inf")
    if records is not None and out is not None:
        raise ValueError("records are read in place: out must be None")
    _dense("out", out, (n, 8), torch)
    _dense("records", records, (n, 8), torch)
    _dense("signed_out", signed_out, (n, 4), torch)
    if not points.is_cuda:
        raise ValueError("points must be on the renderer's device, not on %s" % points.device)
    dev = points.device
    if any(x is not None and x.device != dev for x in (out, records, signed_out)):
        raise ValueError("points, out, records, signed_out must be on one device")
    dev_id = rt.info().deviceId
    if dev_id >= 0 and dev.index is not None and dev.index != dev_id:
        raise ValueError("the points are on %s, the renderer on device %d" % (dev, dev_id))
    cur = torch.cuda.current_stream(dev)
    with torch.cuda.device(dev):
        rec = records if records is not None else out
        if rec is None:
            rec = torch.empty((n, 8), dtype=torch.float32, device=dev)
        sd = signed_out if signed_out is not None else torch.empty((n, 4), dtype=torch.float32, device=dev)
        ready, done = torch.cuda.Event(), torch.cuda.Event()
        ready.record(cur)
        done.record(cur)  # creates the handle; the renderer records it again behind the kernels
        rt.signed_distance_device(points.data_ptr(), n, rec.data_ptr(), sd.data_ptr(), stride=stride,
                                  max_distance=max_distance, from_records=records is not None,
                                  ready_event=ready.cuda_event, done_event=done.cuda_event)
        cur.wait_event(done)
    return rec, sd


def split(hits):
    """(t, tri, u, v) views of an (n, 4) hit tensor; tri is int32, -1 on a miss."""
    return t_of(hits), tri_of(hits), u_of(hits), v_of(hits)


def t_of(hits):
    return hits[:, 0]


def tri_of(hits):
    import torch

    return hits.view(torch.int32)[:, 1]


def u_of(hits):
    return hits[:, 2]


def v_of(hits):
    return hits[:, 3]


# ---- views of an (n, 12) or (n, 16) surface tensor


def position(surf):
    """The hit point re-projected onto its triangle, (n, 3); 1e11 on a miss."""
    return surf[:, 0:3]


def offset(surf):
    """The reference's ray offset at the hit, (n,); 1e-7 on a miss."""
    return surf[:, 3]


def normal(surf):
    """The geometric normal facing the ray, (n, 3); (0, -1, 0) on a miss."""
    return surf[:, 4:7]


def normal_dot_dir(surf):
    """dot(normal, direction), <= 0, (n,)."""
    return surf[:, 7]


def shading_normal(surf):
    """The interpolated vertex normal on the geometric normal's side, (n, 3); (0, -1, 0) on a miss."""
    return surf[:, 8:11]


def word(surf):
    """The material / front-face / hit word as int32, (n,)."""
    import torch

    return surf.view(torch.int32)[:, 11]


def material(surf):
    """The material id the path tracer reads for the hit triangle, int32 (n,); 0 on a miss."""
    return word(surf) & 0xFFFF


def front_face(surf):
    """Whether the ray met the front of the triangle, bool (n,); False on a miss."""
    return (word(surf) & (1 << 16)) != 0


def is_hit(surf):
    return (word(surf) & (1 << 17)) != 0


def displacement(surf):
    """How the hit point moved since the build before, (n, 3): only of (n, 16) records (motion=True)."""
    if surf.shape[1] != 16:
        raise ValueError("displacement needs the (n, 16) records of motion=True")
    return surf[:, 12:15]


def spawn_origins(surf, directions):
    """Origins of secondary rays leaving the hits along `directions` (n, 3): pos + offset * normal, and
    pos - offset * normal where the direction points through the surface (dot(direction, normal) < 0),
    as the reference's reflection and refraction do.  A plain torch expression in float32: its roundings
    are torch's, so unlike the records it makes no claim of bit parity with the reference."""
    nrm = normal(surf)
    side = ((directions[:, 0:3] * nrm).sum(1) < 0).to(surf.dtype) * -2.0 + 1.0
    return position(surf) + (offset(surf) * side)[:, None] * nrm


# ---- views of an (n, 8) closest-point tensor


def closest_position(rec):
    """The nearest point of the nearest triangle, (n, 3); 1e11 on a miss."""
    return rec[:, 0:3]


def distance2(rec):
    """The squared distance to it, (n,); inf on a miss."""
    return rec[:, 3]


def closest_tri(rec):
    """The triangle index as int32, (n,); -1 on a miss."""
    import torch

    return rec.view(torch.int32)[:, 4]


def closest_uv(rec):
    """(u, v), (n, 2): the weights of the triangle's first and second vertex, the third's is 1 - u - v."""
    return rec[:, 5:7]


def closest_word(rec):
    """The feature / front / found word as int32, (n,)."""
    import torch

    return rec.view(torch.int32)[:, 7]


def closest_feature(rec):
    """0 face, 1 2 3 vertex 1 2 3, 4 edge 12, 5 edge 23, 6 edge 31; int32 (n,), 0 on a miss."""
    return closest_word(rec) & 7


def closest_front(rec):
    """Whether the point lies on the side the triangle's normal (v2 - v1) x (v3 - v1) points to, bool (n,)."""
    return (closest_word(rec) & (1 << 16)) != 0


def closest_found(rec):
    return (closest_word(rec) & (1 << 17)) != 0


# ---- views of an (n, 4) signed distance tensor


def signed_distance_of(signed):
    """The distance to the nearest point of the mesh, negative inside, (n,); inf on a miss."""
    return signed[:, 3]


def pseudo_normal(signed):
    """The nearest feature's pseudo-normal, (n, 3): a face's unit normal, the sum of an edge's unit normals,
    a vertex's angle-weighted sum.  Not normalised; all zero on a miss or where no incident triangle counted."""
    return signed[:, 0:3]


def inside(signed):
    """Whether the point lies inside the closed mesh, bool (n,); False on a miss."""
    return signed[:, 3] < 0
