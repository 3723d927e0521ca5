"""The traversal's limits on the GPU: the 16-entry stack, the push onto a full stack that is dropped
and the 1,024-iteration cap (csrc/traverse.h trav_step, trav_done), in every kernel that traverses,
bit for bit against the CPU oracle.

The limits have their own code per instantiation: with the whole stack in LDS (k_trace_queue,
k_trace_rays, k_pt_shade0<glossy>, k_pt_chain) the would-be push is stored unconditionally, on a full
stack into the 17th, dead slot of the column; with ten entries in LDS (k_pt_camera, k_trace_primary)
entries 10..15 live in the DeepStack select chains; the queue tracers and the ray queries apply the cap
through trav_done, two steps per trip.  A dropped push changes which triangle a ray reports
(tests/test_traversal_limits.py), so none of this may differ from the reference.

The inputs are limit_scenes': every test first asserts, from the oracle's maxDepth, droppedPushes and
iterations, that its own rays reach the limit it is for, with the lower bounds test_traversal_limits.py
pins on the CPU.

Hit records: a record's (u, v) are the closest hit's own, oracle.intersect_uv's.  The oracle's u / v
(HitInfo's, overwritten at every triangle test that passes) belong to another triangle wherever a
coplanar triangle of the same group ties the closest t, which these meshes are full of; the primary-ray
kernel reports those, and is compared with them."""
import numpy as np
import pytest

from bvh_check import rays_for
from limit_scenes import (FOV_NARROW, FOV_WIDE, H, W, chain1201, chain31, chain_rays, limit_camera, limits, mirror_rays,
                          share_text, shares)
from mesh_scenes import DUPLICATE_SHAPES
from test_gpu_mesh import assert_gbuffers_equal, bits, gpu_gbuffers, oracle_mesh, patch_rt
from test_gpu_ray_query import assert_records, rec_of, residual, to_dev
from test_gpu_trace import assert_same

pytestmark = pytest.mark.gpu

FRAME = 1
SPP = 2
MESHES = {"chain31": chain31, "chain1201": chain1201, "all_equal": DUPLICATE_SHAPES["all_equal"]}
# the lower bounds of test_traversal_limits.py: what a ray set has to reach on the named mesh
REACH = {"chain31": dict(full=0.25, drop=0.15), "chain1201": dict(cap=0.9, drop=0.14), "all_equal": dict(cap=0.5)}
REACH_CAMERA = {("chain31", "narrow"): dict(full=0.4, drop=0.3), ("chain1201", "narrow"): dict(cap=0.9, drop=0.14),
                ("chain1201", "corner"): dict(full=0.1, drop=0.1)}
# view -> limit_camera's (fov, view): the front camera at 20 and 90 degrees, and the one behind the +x corner
VIEWS = {"narrow": (FOV_NARROW, "front"), "wide": (FOV_WIDE, "front"), "corner": (FOV_NARROW, "corner")}


@pytest.fixture(scope="module")
def meshes(oracle):
    """name -> the mesh and the oracle's build of it, computed once."""
    cache = {}

    def get(name):
        if name not in cache:
            cache[name] = oracle_mesh(oracle, *MESHES[name]())
        return cache[name]
    return get


@pytest.fixture(scope="module")
def sky_tex(oracle):
    return oracle.sky(), oracle.textures()


def assert_reaches(s, want, what):
    for k, lo in want.items():
        assert s[k] >= lo, (what, k, s[k], lo)


@pytest.fixture(scope="module")
def ray_cases(oracle, meshes):
    """(mesh, n) -> the rays and the oracle's records of them (test_gpu_ray_query.assert_records' form),
    computed once and read-only.  The records hold oracle.intersect_uv's pair, so no ray is `foreign`:
    the residual |org + t dir - P(tri, u, v)| of every record is of rounding size, which is asserted here with the
    bound 16 x 2^-23 x the largest |org| + t (the largest coordinate the point is computed from, and
    above the edge length the barycentrics scale; the nearest other triangle's point is 1.4 away)."""
    cache = {}

    def get(name, n):
        if (name, n) not in cache:
            m = meshes(name)
            rays = rays_for(m["v"], m["idx"]) if name == "all_equal" else chain_rays(n, 3)
            org, d = np.ascontiguousarray(rays[:, :3]), np.ascontiguousarray(rays[:, 3:])
            o, uv = oracle.intersect_uv(m["bvh"], rays)
            s = shares(o)
            print(share_text("%s, %d rays" % (name, len(rays)), s))
            assert_reaches(s, REACH[name], name)
            rec = np.empty((len(rays), 4), np.uint32)
            rec[:, 0], rec[:, 1] = bits(o["t"]), o["objectIdx"].view(np.uint32)
            rec[:, 2], rec[:, 3] = bits(uv[:, 0]), bits(uv[:, 1])
            corners = m["bvh"]["triangles"].reshape(-1, 6, 3)[:, :3].astype(np.float64)
            res = residual(org, d, rec, corners)
            reach = float((np.linalg.norm(org.astype(np.float64), axis=1) + np.where(o["hit"] == 1, o["t"], 0.0)).max())
            foreign = res > 16.0 * 2.0 ** -23 * reach
            assert foreign.sum() == 0, (name, int(foreign.sum()), float(res.max()))
            ties = int(((bits(o["u"]) != rec[:, 2]) | (bits(o["v"]) != rec[:, 3])).sum())
            print("%s: largest record residual %.3g; %d rays whose HitInfo (u, v) are a tying triangle's" % (
                name, res.max(), ties))
            c = dict(org=org, dir=d, rec=rec, iters=o["iterations"].astype(np.uint32), foreign=foreign,
                     res_max=float(res.max()), o=o)
            for a in (org, d, rec, c["iters"], foreign):
                a.setflags(write=False)
            cache[(name, n)] = c
        return cache[(name, n)]
    return get


def limit_rt(rtx, tmp_path, m, name="l.toml", **kw):
    """A 96 x 54 context holding mesh m, its LBVH built."""
    rt = patch_rt(rtx, tmp_path, name, max_triangles=2048, max_vertices=4096, **kw)
    rt.set_mesh(m["v"], m["idx"])
    rt.build_bvh()
    return rt


@pytest.mark.parametrize("name", ["chain31", "chain1201"])
def test_queue_tracer_at_the_limits(rtx, tmp_path, meshes, ray_cases, name):
    """k_trace_queue (rt_trace_rays), the whole stack in LDS: t, triangle, u, v and iterations of
    2,048 chain rays.  chain31: half of them fill the stack, a third drops pushes (the dead slot);
    chain1201: every ray ends at the cap, inside trav_done's two steps per trip."""
    c = ray_cases(name, 2048)
    rt = limit_rt(rtx, tmp_path, meshes(name))
    t, tri, u, v, iters, _ = rt.trace_rays(c["org"], c["dir"], want_iters=True)
    rt.cleanup()
    assert np.array_equal(bits(t), c["rec"][:, 0]) and np.array_equal(tri.view(np.uint32), c["rec"][:, 1])
    assert np.array_equal(bits(u), c["rec"][:, 2]) and np.array_equal(bits(v), c["rec"][:, 3])
    assert np.array_equal(iters, c["iters"])


@pytest.mark.parametrize("name", ["chain31", "chain1201", "all_equal"])
def test_device_query_at_the_limits(rtx, tmp_path, meshes, ray_cases, name):
    """k_trace_rays (rtx.query.trace) on one workgroup per CU: records and iterations of 4,096 chain
    rays, and of bvh_check.rays_for on all_equal, 1,024 coincident triangles under one key, where the
    rays that hit run to the cap without ever holding more than a few entries."""
    from rtx import query

    c = ray_cases(name, 4096)
    rt = limit_rt(rtx, tmp_path, meshes(name), tuning=dict(tracePerCu=1))
    org, d = to_dev(c["org"], c["dir"])
    hits, iters = query.trace(rt, org, d, want_iters=True)
    assert_records(hits, iters, c, what=name)
    rt.cleanup()


def test_any_hit_at_the_limits(rtx, tmp_path, meshes, ray_cases):
    """RT_QUERY_ANY_HIT on chain31's 4,096 rays, test_gpu_ray_query.test_any_hit's properties: the
    closest-hit answer to hit or miss, no more iterations (fewer for some ray), the same record where
    the counts are equal, t no nearer (the closest-hit traversal passes through the any-hit ray's state
    and only lowers t afterwards, limits or not), barycentrics inside the triangle and a residual within
    4 x the largest of the oracle's closest-hit records of these rays."""
    from rtx import query

    c = ray_cases("chain31", 4096)
    rt = limit_rt(rtx, tmp_path, meshes("chain31"))
    org, d = to_dev(c["org"], c["dir"])
    hits, iters = query.trace(rt, org, d, any_hit=True, want_iters=True)
    tris = rt.download("TRI_POS", np.float32).reshape(-1, 3, 4)[:, :, :3].astype(np.float64)
    tri_count = rt.info().triCount
    rt.cleanup()
    a, ai = rec_of(hits), iters.cpu().numpy().view(np.uint32)
    cr, ci = c["rec"], c["iters"]
    a_tri, c_tri = a[:, 1].view(np.int32), cr[:, 1].view(np.int32)
    assert np.array_equal(a_tri >= 0, c_tri >= 0)
    assert (ai <= ci).all() and (ai < ci).any()
    same = ai == ci
    assert np.array_equal(a[same], cr[same])
    hit = a_tri >= 0
    assert (a[hit, 0].view(np.float32) >= cr[hit, 0].view(np.float32)).all()
    assert np.array_equal(a[~hit], cr[~hit])
    au, av = a[hit, 2].view(np.float32), a[hit, 3].view(np.float32)
    assert (a_tri[hit] < tri_count).all()
    assert (au >= 0).all() and (av >= 0).all() and (au.astype(np.float64) + av.astype(np.float64) <= 1.0).all()
    bound = 4.0 * c["res_max"]
    worst = residual(c["org"], c["dir"], a, tris).max()
    print("any-hit: %d of %d rays end earlier, mean iterations %.1f vs %.1f; residual bound 4 x %.3e = %.3e, worst %.3e"
          % ((ai < ci).sum(), len(ai), ai.mean(), ci.mean(), bound / 4.0, bound, worst))
    assert worst <= bound


CAMERA_CASES = [("chain31", "narrow"), ("chain31", "wide"), ("chain1201", "narrow"), ("chain1201", "corner")]


@pytest.fixture(scope="module")
def camera_rays(oracle, meshes):
    """(mesh, fov) -> the oracle's hits of frame FRAME's camera rays, with the case's precondition."""
    cache = {}

    def get(name, fov):
        if (name, fov) not in cache:
            oc, _ = limit_camera(None, oracle, *VIEWS[fov])
            prim, _ = oracle.primary_rays(W, H, FRAME, cam=oc)
            o = oracle.intersect(meshes(name)["bvh"], prim)
            s = shares(o)
            print(share_text("%s, camera rays, %s" % (name, fov), s))
            if fov == "wide":  # limits, plain hits and misses side by side
                full, drop, cap = limits(o)
                assert s["drop"] > 0 and 1.0 - s["hit"] >= 0.1 and (~(drop | cap)).mean() >= 0.3
            else:
                assert_reaches(s, REACH_CAMERA[(name, fov)], (name, fov))
            assert s["deep"] >= 0.2  # past the ten entries in LDS (measured: 0.44 wide, 0.40 corner, 1.00 narrow)
            if fov == "corner":  # what a mirror sends on from here fills the stack (measured: 0.80)
                b = oracle.intersect(meshes(name)["bvh"], mirror_rays(prim, o))
                full, drop, cap = limits(b)
                print(share_text("%s, camera rays reflected, %s" % (name, fov), shares(b)))
                assert (full & drop).mean() >= 0.4
            cache[(name, fov)] = o
        return cache[(name, fov)]
    return get


@pytest.mark.parametrize("name,fov", CAMERA_CASES)
def test_primary_rays_at_the_limits(rtx, oracle, tmp_path, meshes, camera_rays, name, fov):
    """k_trace_primary, ten entries in LDS and six in the DeepStack registers up to e5: hits, normals,
    offsets and the four counters of a 96 x 54 frame.  The dropped-push column is non-zero."""
    o = camera_rays(name, fov)
    _, rc = limit_camera(rtx, oracle, *VIEWS[fov])
    rt = limit_rt(rtx, tmp_path, meshes(name))
    rt.camera = rc
    rt.trace_primary(FRAME, detail=True)
    rt.sync()
    g = dict(hits=rt.download("HITS", np.float32).reshape(-1, 4), nrm=rt.download("HIT_NORMALS", np.float32).reshape(-1, 4),
             fake=rt.download("HIT_FAKE_NORMALS", np.float32).reshape(-1, 4),
             stats=rt.download("HIT_STATS", np.uint32).reshape(-1, 4))
    rt.cleanup()
    assert (o["droppedPushes"] > 0).any() and (g["stats"][:, 2] > 0).any()
    assert_same(g, o)


@pytest.fixture(scope="module")
def oracle_frames(oracle, meshes, sky_tex):
    cache = {}

    def get(name, fov, override):
        key = (name, fov, override)
        if key not in cache:
            oc, _ = limit_camera(None, oracle, *VIEWS[fov])
            s, tex = sky_tex
            cache[key] = oracle.pathtrace(meshes(name)["bvh"], W, H, frame_num=FRAME, spp=SPP, cam=oc, hist_cam=oc,
                                          sky_out=s, tex=tex, material_override=override)
        return cache[key]
    return get


def frame(rtx, oracle, tmp_path, m, fov, override, tuning=None):
    """One detail launch of frame FRAME under [render] materialOverride: G-buffers with RAYS, the
    counters, lastChain and the rays the frame put into queue 3."""
    _, rc = limit_camera(rtx, oracle, *VIEWS[fov])
    rt = limit_rt(rtx, tmp_path, m, spp=SPP, extra="materialOverride = %d\n" % override, tuning=tuning)
    rt.camera = rc
    rt.path_trace(FRAME, detail=True)
    rt.sync()
    g = gpu_gbuffers(rt, W, H)
    q = rt.download("PT_QUEUE", np.uint32).copy()
    chain = rt.info().lastChain
    n3 = int(q[0])
    q3 = np.concatenate([rt.download("PT_Q3_ORIGINS", np.float32).reshape(-1, 4)[:n3, :3],
                         rt.download("PT_Q3_DIRS", np.float32).reshape(-1, 4)[:n3, :3]], axis=1)
    rt.cleanup()
    return g, q, chain, q3


# override -> ([tuning], lastChain, the bounce plan behind the shade kernel (frame_kernels.h pt_bounce_plan)).
# Overrides 5 and 1 are of the glossy class, whose plan is unsplit whatever resumeSplit says; 3 and 4 keep a
# shading list by default, so resumeSplit = 0 selects other kernels there: k_trace_queue<3> without the list
# and the unsplit k_pt_resume<3>.
PLANS = {3: [(None, 1, "chain"), (dict(chain="off"), 0, "split"), (dict(chain="off", resumeSplit=0), 0, "unsplit")],
         4: [(None, 0, "split"), (dict(resumeSplit=0), 0, "unsplit")],
         5: [(None, 0, "unsplit")],
         1: [(None, 0, "unsplit")]}


@pytest.mark.parametrize("name,fov", CAMERA_CASES)
def test_path_trace_at_the_limits(rtx, oracle, tmp_path, meshes, camera_rays, oracle_frames, name, fov):
    """k_pt_camera (ten entries in LDS), k_pt_shade0<glossy>'s inline bounces, the fused chain, and
    k_trace_queue<3> / <4> with the resume kernels: a 96 x 54, 2-spp frame under materialOverride 3, 5, 4
    and 1 equals the oracle's in every G-buffer and in RAYS, in every bounce plan the override can run as
    (PLANS): override 3 as the fused chain, with [tuning] chain = "off" as the split bounce kernels and with
    resumeSplit = 0 on top as the unsplit ones; override 4 split and unsplit; 5 and 1 unsplit.  The shading
    list (PT_QUEUE[23]) is empty in the unsplit plans and, for override 3, as long as the count of
    resume<3>'s diffuse events in the split one.

    The oracle keeps no per-bounce statistics, so the rays each frame queued are downloaded and traced
    by oracle.intersect, and their shares printed.  Overrides 3 and 4 queue rays in every case (asserted).
    From the front camera no queued ray fills the stack (printed only, a note on coverage: at most one ray
    in a thousand holds more than ten entries; limit_scenes.limit_camera says why).  From the corner camera
    queued rays of overrides 3 and 4 fill the stack and drop a push, in every plan of theirs (asserted).
    The rays a mirror or glass sends on are traced inside k_pt_shade0<glossy> and never queued (override 5
    queues nothing at all here), so that kernel's coverage is shown by proxy only: camera_rays shows on
    the oracle that the camera rays' reflections fill the stack.  These are conditions on the coverage;
    the frame's correctness is the G-buffer equality."""
    camera_rays(name, fov)  # the camera rays reach their limits
    m = meshes(name)
    reached = {}
    for override in (3, 5, 4, 1):
        want = oracle_frames(name, fov, override)
        assert (want["color"][:, 3] == override).mean() >= (0.5 if fov == "wide" else 0.99)  # surface pixels
        for tuning, want_chain, plan in PLANS[override]:
            g, q, chain, q3 = frame(rtx, oracle, tmp_path, m, fov, override, tuning)
            assert_gbuffers_equal(g, want)
            assert q[10] == 0, (override, plan)  # kCntError
            assert chain == want_chain, (override, plan)
            if plan == "unsplit":
                assert q[23] == 0, (override, plan)  # no shading list
            elif plan == "split":
                assert q[23] <= q[0], (override, plan)
                if override == 3:  # a listed entry is a D1 event and the reverse (test_gpu_resume_split.py)
                    assert q[23] == q[21], (override, plan, q[23], q[21])
            what = "%s %s, override %d %s, %d queued rays, %d listed" % (name, fov, override, plan, len(q3), q[23])
            if override in (3, 4):
                assert len(q3) > 0, what
            if len(q3) == 0:  # every path ended inside the shading kernel
                print(what)
                continue
            o = oracle.intersect(m["bvh"], q3)
            full, drop, cap = limits(o)
            reached[(override, plan)] = bool((full & drop).any())
            print(share_text(what, shares(o)) + ", 16 entries and dropped %.4f" % (full & drop).mean())
    if fov == "corner":
        for override in (3, 4):
            for _, _, plan in PLANS[override]:
                assert reached[(override, plan)], (override, plan, reached)
