"""Device ray queries on torch tensors (rt_trace_rays_device, include/rtx_amd.h).

``trace(rt, origins, directions)`` traces n rays that live in device tensors against the BVH of the
last ``build_bvh`` / draw and returns their hit records as a device tensor, without a host
synchronisation and without a copy of the inputs: visibility, line of sight, picking, collision and
ray-cast sensors against geometry the host animates on the device (``update_vertices_device``).

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


def trace(rt, origins, directions, *, any_hit: bool = False, want_iters: bool = False, out=None):
    """Hit records of the rays (origins[i, :3], directions[i, :3]).

    origins, directions: float32 device tensors of shape (n, 3..8) with a unit inner stride; the row
    stride (the leading dimension of the storage, e.g. 8 for the two halves ``rays[:, 0:3]`` and
    ``rays[:, 4:7]`` of one interleaved (n, 8) tensor) is passed on, nothing is copied.  Directions
    need not be normalised.  any_hit: each ray stops at the first hit the traversal records (same
    hit / miss answer, t >= the closest t).  out: an (n, 4) contiguous float32 tensor for the records.

    Returns hits (n, 4) float32: t (1e11 on a miss), the triangle index as int32 bits (-1), u, v (see
    ``split``), and with want_iters also the traversal iterations per ray as an (n,) int32 tensor."""
    import torch

    n, org_stride = _rays("origins", origins, torch)
    nd, dir_stride = _rays("directions", directions, torch)
    if nd != n:
        raise ValueError("origins and directions must hold the same number of rays (%d, %d)" % (n, nd))
    if n > (1 << 30):
        raise ValueError("at most 2^30 rays per query")
    if out is not None and (not isinstance(out, torch.Tensor) or out.dtype != torch.float32
                            or tuple(out.shape) != (n, 4) or not out.is_contiguous()):
        raise ValueError("out must be a contiguous (n, 4) float32 tensor")
    for name, x in (("origins", origins), ("directions", directions)):  # the device checks come last
        if not x.is_cuda:
            raise ValueError("%s must be on the renderer's device, not on %s" % (name, x.device))
    if directions.device != origins.device or (out is not None and out.device != origins.device):
        raise ValueError("origins, directions and out must be on one device")
    dev = origins.device
    dev_id = rt.info().deviceId
    if dev_id >= 0 and dev.index is not None and dev.index != dev_id:
        raise ValueError("the rays are on %s, the renderer on device %d" % (dev, dev_id))
    cur = torch.cuda.current_stream(dev)
    with torch.cuda.device(dev):
        hits = out if out is not None else torch.empty((n, 4), dtype=torch.float32, device=dev)
        iters = torch.empty(n, dtype=torch.int32, device=dev) if want_iters else None
        ready, done = torch.cuda.Event(), torch.cuda.Event()
        ready.record(cur)
        done.record(cur)  # creates the handle; the renderer records it again behind the kernel
        rt.trace_rays_device(origins.data_ptr(), directions.data_ptr(), n, hits.data_ptr(), org_stride=org_stride,
                             dir_stride=dir_stride, iters_ptr=iters.data_ptr() if want_iters else None,
                             any_hit=any_hit, ready_event=ready.cuda_event, done_event=done.cuda_event)
        cur.wait_event(done)
    return (hits, iters) if want_iters else hits


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
