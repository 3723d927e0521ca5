"""GPU LBVH build and traversal on meshes with repeated Morton keys (mesh_scenes.DUPLICATE_SHAPES):
runs of three and more equal keys inside a batch and among the TLAS leaves, in both workgroup shapes
of the build kernel and on both TLAS paths.  The arrays equal the oracle's bit for bit, pass the
reference-free tree check on their own and are the same on a second build; the traversal equals the
oracle's, whose hits tests/test_bvh_duplicates.py checks against float64 brute force.

Without the tie-break in bvh_build.hip lcp these inputs have no valid tree (DESIGN.md deviation 15)."""
import numpy as np
import pytest

from bvh_check import assert_valid_bvh, rays_for
from mesh_scenes import DUPLICATE_ORDER, DUPLICATE_SHAPES
from test_gpu_mesh import assert_bvh, bits, oracle_mesh, patch_rt

pytestmark = pytest.mark.gpu

W, H = 96, 54
MAX_TRIANGLES = 68608  # tlas66: 66 batches + 1
MAX_VERTICES = 66 * 576
# tlas66 between smaller meshes; the rest of DUPLICATE_ORDER around it
ORDER = DUPLICATE_ORDER[:4] + ("tlas66",) + DUPLICATE_ORDER[4:]
DEVICE_SET = "stack5"  # this one arrives through set_mesh_device


@pytest.fixture(scope="module")
def meshes(oracle):
    """name -> the mesh and the oracle's build of it, computed once for both workgroup shapes."""
    cache = {}

    def get(name):
        if name not in cache:
            cache[name] = oracle_mesh(oracle, *DUPLICATE_SHAPES[name]())
        return cache[name]
    return get


def downloaded(rt):
    return {k: rt.download(k).copy() for k in ("NODES", "MORTON", "REORDER", "AABBS", "TRI_POS", "TLAS_NODES", "TLAS_AABBS",
                                            "TLAS_MORTON", "TLAS_REORDER", "TLAS_SCENE_AABB", "BATCH_SCENE_AABBS")}


def assert_tlas(rt, ob):
    assert np.array_equal(bits(rt.download("TLAS_AABBS", np.float32).reshape(-1, 6)), bits(ob["tlas_aabbs"]))
    assert np.array_equal(bits(rt.download("TLAS_SCENE_AABB", np.float32)), bits(ob["tlas_scene_aabb"]))
    assert np.array_equal(rt.download("TLAS_MORTON", np.uint32), ob["tlas_morton"])
    assert np.array_equal(rt.download("TLAS_REORDER", np.uint32), ob["tlas_reorder"])
    assert np.array_equal(bits(rt.download("BATCH_SCENE_AABBS", np.float32).reshape(-1, 6)), bits(ob["batch_scene_aabbs"]))


@pytest.mark.parametrize("threads", [1024, 512])
def test_builds_with_equal_keys(rtx, oracle, tmp_path, meshes, threads):
    """Every duplicate mesh in turn on one context, in an order that shrinks after growing: the BVH
    arrays equal the oracle's, are a valid tree on their own, and a second build gives the same bytes."""
    import torch

    rt = patch_rt(rtx, tmp_path, max_triangles=MAX_TRIANGLES, max_vertices=MAX_VERTICES,
                  extra="bvhThreads = %d\n" % threads)
    for name in ORDER:
        m = meshes(name)
        n = len(m["idx"])
        if name == DEVICE_SET:
            dv, di = torch.from_numpy(m["v"]).cuda(), torch.from_numpy(m["idx"].astype(np.int32)).cuda()
            torch.cuda.synchronize()
            rt.set_mesh_device(dv.data_ptr(), len(m["v"]), di.data_ptr(), n)
        else:
            rt.set_mesh(m["v"], m["idx"])
        rt.build_bvh()
        rt.sync()
        first = downloaded(rt)
        assert_bvh(rt, rtx, m["bvh"], n)
        assert_tlas(rt, m["bvh"])
        assert_valid_bvh(first["NODES"].view(rtx.NODE_DTYPE), first["REORDER"].view(np.uint32),
                         first["AABBS"].view(np.float32).reshape(-1, 6), first["TLAS_NODES"].view(rtx.NODE_DTYPE),
                         first["TLAS_REORDER"].view(np.uint32), first["TLAS_AABBS"].view(np.float32).reshape(-1, 6), n)
        rt.build_bvh()
        rt.sync()
        second = downloaded(rt)
        for k in first:
            assert np.array_equal(first[k], second[k]), (name, k)
    rt.cleanup()


# (position, yaw, pitch) with the mesh in view
CAMERAS = {
    "stack3": ((5.5, 3.0, -1.5), 0.0, -0.8),
    "runs": ((5.15, 0.3, 0.0), 0.0, -1.2),
    "speck": ((0.00575, 1.3, -0.25), 0.0, -0.9),
    "tlas3": ((5.5, 4.0, -3.0), 0.0, -0.55),
}


def cameras(rtx, oracle, name):
    pos, yaw, pitch = CAMERAS[name]
    oc = oracle.default_camera(W, H)
    oc.pos[:] = pos
    oc.yaw, oc.pitch = yaw, pitch
    rc = rtx.Camera()
    rc.pos[:] = pos
    rc.yaw, rc.pitch, rc.focal, rc.aperture, rc.fovX = yaw, pitch, oc.focal, oc.aperture, oc.fovX
    return rc, oc


@pytest.mark.parametrize("name", sorted(CAMERAS))
def test_traversal_with_equal_keys(rtx, oracle, tmp_path, meshes, name):
    """rt_trace_rays over the CPU test's 600 rays and the camera rays of a 96 x 54 frame: t, triangle,
    barycentrics and the counters equal the oracle's bit for bit."""
    m = meshes(name)
    ob = m["bvh"]
    rt = patch_rt(rtx, tmp_path, max_triangles=4096, max_vertices=4096)
    rt.set_mesh(m["v"], m["idx"])
    rc, oc = cameras(rtx, oracle, name)
    rt.camera = rc
    rt.build_bvh()
    rays = rays_for(m["v"], m["idx"])
    t, tri, u, v, iters, _ = rt.trace_rays(rays[:, :3], rays[:, 3:], want_iters=True)
    oh = oracle.intersect(ob, rays)
    assert (oh["hit"] == 1).mean() > 0.5
    assert np.array_equal(tri, oh["objectIdx"]) and np.array_equal(bits(t), bits(oh["t"]))
    assert np.array_equal(bits(u), bits(oh["u"])) and np.array_equal(bits(v), bits(oh["v"]))
    assert np.array_equal(iters, oh["iterations"])
    rt.trace_primary(1, detail=True)
    rt.sync()
    hits = rt.download("HITS", np.float32).reshape(-1, 4)
    stats = rt.download("HIT_STATS", np.uint32).reshape(-1, 4)
    rt.cleanup()
    prim, _ = oracle.primary_rays(W, H, 1, cam=oc)
    o = oracle.intersect(ob, prim)
    assert o["hit"].mean() > 0.2, name  # the mesh is in view
    assert np.array_equal(bits(hits[:, 0]), bits(o["t"])) and np.array_equal(hits[:, 1].view(np.int32), o["objectIdx"])
    assert np.array_equal(bits(hits[:, 2]), bits(o["u"])) and np.array_equal(bits(hits[:, 3]), bits(o["v"]))
    for k, f in enumerate(("nodeVisits", "triTests", "droppedPushes", "iterations")):
        assert np.array_equal(stats[:, k], o[f]), (name, f)
