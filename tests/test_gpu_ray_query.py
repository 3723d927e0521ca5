"""Device ray queries (rt_trace_rays_device, csrc/trace_rays.hip, rtx.query) vs the CPU oracle, bit
for bit, and their ordering against builds, vertex updates and frames without a host sync.

Every case runs on the default 60,800-triangle scene with a 64x36 context, whose queue capacity
(rt_trace_rays' limit) is 2,304 rays: every batch below except the edge counts is over it.

The rays: origins uniform in [-40, 100]^3 aimed at points uniform in the vertex AABB (random
directions hit 0.4 % of the time), the first eighth with one direction component zeroed (the
traversal's safe-divide path).  The oracle's hit share of the set is asserted to lie in (0.5, 0.95),
so neither the hits nor the misses go untested."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

N = 100037
W, H = 64, 36
DT = 16.667
QN = 4096
PICK = np.arange(QN) * (N // QN)  # 4,096 rays across the set: the zeroed-component eighth and the others


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def make_rays(vertices, n=N, seed=11):
    rng = np.random.default_rng(seed)
    org = rng.uniform(-40.0, 100.0, (n, 3)).astype(np.float32)
    lo, hi = vertices.min(0), vertices.max(0)
    tgt = rng.uniform(lo, hi, (n, 3)).astype(np.float32)
    d = tgt - org
    k = n // 8
    d[np.arange(k), rng.integers(0, 3, k)] = 0.0  # axis-parallel components (safe_divide path)
    d /= np.linalg.norm(d, axis=1, keepdims=True).astype(np.float32)
    assert org.dtype == np.float32 and d.dtype == np.float32
    return org, d


def residual(org, d, rec, corners):
    """|org + t dir - P(tri, u, v)| of the hit records (float64), P = u v1 + v v2 + (1 - u - v) v3 as
    the traversal weights the corners; 0 for misses.  corners: float64 [triangles][3][3]."""
    hit = rec[:, 1].view(np.int32) >= 0
    t = rec[hit, 0].view(np.float32).astype(np.float64)
    k = rec[hit, 1].view(np.int32)
    u = rec[hit, 2].view(np.float32).astype(np.float64)
    v = rec[hit, 3].view(np.float32).astype(np.float64)
    p = corners[k, 0] * u[:, None] + corners[k, 1] * v[:, None] + corners[k, 2] * (1.0 - u - v)[:, None]
    q = org[hit].astype(np.float64) + t[:, None] * d[hit].astype(np.float64)
    out = np.zeros(len(rec))
    out[hit] = np.linalg.norm(q - p, axis=1)
    return out


# A record whose (u, v) are its own triangle's has a residual of rounding size: a few units of
# 2^-23 (|org| + t) <= 2^-23 * 500 = 6e-5 for these rays (measured on the oracle: at most 3.2e-5 over
# 69,689 hits).  Foreign barycentrics put P elsewhere on the triangle, an edge length (0.1 .. 0.3) off.
FOREIGN_RESIDUAL = 1e-3


def oracle_records(oracle, bvh, org, d):
    """The oracle's records of the rays as bit patterns, its iteration counts, and `foreign`.

    oracle.intersect reports the reference's HitInfo.u / .v, which TraverseBvh overwrites at every
    triangle test that passes, also one that ties the closest t without replacing it (a ray through an
    edge shared by two triangles): there (u, v) belong to the other triangle, not to objectIdx.  The
    renderer's hit records (k_trace_queue's hitRec, rt_trace_rays, rt_trace_rays_device) keep the
    closest hit's own (u, v), the pair the reference shades with.  `foreign` marks the rays whose
    oracle (u, v) are demonstrably not a point of their triangle on the ray (FOREIGN_RESIDUAL): one
    ray of the 100,037 (index 75038, residual 1.4e-2).  Their t, triangle and iterations are compared
    with the oracle like every other ray's; their (u, v) with rt_trace_rays' (test 1)."""
    o = oracle.intersect(bvh, np.concatenate([org, d], axis=1))
    rec = np.empty((len(org), 4), np.uint32)
    rec[:, 0] = bits(o["t"])
    rec[:, 1] = o["objectIdx"].view(np.uint32)
    rec[:, 2] = bits(o["u"])
    rec[:, 3] = bits(o["v"])
    corners = bvh["triangles"].reshape(-1, 6, 3)[:, :3].astype(np.float64)
    res = residual(org, d, rec, corners)
    foreign = res > FOREIGN_RESIDUAL
    assert foreign.sum() <= max(1, len(org) // 10000), foreign.sum()  # an exception, never a way out
    return dict(rec=rec, iters=o["iterations"].astype(np.uint32), foreign=foreign, res_max=float(res[~foreign].max()),
                share=float((o["objectIdx"] >= 0).mean()))


@pytest.fixture(scope="module")
def rays(oracle, default_scene):
    """The ray set and the oracle's records for it on the default scene, computed once."""
    org, d = make_rays(default_scene["vertices"])
    r = oracle_records(oracle, default_scene["bvh"], org, d)
    assert 0.5 < r["share"] < 0.95, r["share"]
    r.update(org=org, dir=d)
    for a in (org, d, r["rec"], r["iters"], r["foreign"]):
        a.setflags(write=False)
    return r


def make_rt(rtx, tmp_path, w=W, h=H, spp=1, tuning=None, name="q.toml"):
    rt = rtx.RayTracer(w, h, rtx.write_config(str(tmp_path / name), w, h, spp=spp, tuning=tuning)).init()
    rt.set_delta_time(DT)
    return rt


def to_dev(*arrays):
    import torch

    out = [torch.from_numpy(np.array(a)).cuda() for a in arrays]  # a copy: the fixture arrays are read-only
    torch.cuda.synchronize()
    return out


def rec_of(hits):
    """(n, 4) uint32 bit patterns of a device hit tensor."""
    return hits.cpu().numpy().view(np.uint32)


def assert_records(hits, iters, ref, n=None, what=""):
    """The device records against the oracle's (oracle_records), bit for bit.  n: the first n rays of the
    set (None: all), or an index array (PICK).  (u, v) of the oracle's `foreign` rays are not compared."""
    sel = slice(0, n) if n is None or isinstance(n, int) else n
    got = rec_of(hits)
    own = ~ref["foreign"][sel]
    for c, name in enumerate(("t", "tri")):
        assert np.array_equal(got[:, c], ref["rec"][sel, c]), (what, name)
    for c, name in ((2, "u"), (3, "v")):
        assert np.array_equal(got[own, c], ref["rec"][sel, c][own]), (what, name)
    if iters is not None:
        assert np.array_equal(iters.cpu().numpy().view(np.uint32), ref["iters"][sel]), (what, "iters")


def test_closest_hit_bit_exact_with_fetch_coverage(rtx, tmp_path, rays):
    """100,037 rays on one workgroup per CU ([tuning] tracePerCu = 1): more rays than the static first
    batches (cus x 256) plus one 64-ray reserve per fetch part, so the dynamic parts and their ragged
    ends run.  t, tri, u, v and iters equal oracle.intersect; the same from one interleaved (n, 8)
    tensor at strides 8, whose first 2,304 records equal rt_trace_rays'.  The (u, v) of the one ray
    whose oracle barycentrics are another triangle's (oracle_records) equal rt_trace_rays' instead."""
    import torch

    from rtx import query

    cus = torch.cuda.get_device_properties(0).multi_processor_count
    assert N > cus * 256 + 8 * 64, cus
    rt = make_rt(rtx, tmp_path, tuning=dict(tracePerCu=1))
    rt.build_bvh()
    org, d = to_dev(rays["org"], rays["dir"])
    hits, iters = query.trace(rt, org, d, want_iters=True)
    assert_records(hits, iters, rays, what="packed")
    t, tri, u, v = (x.cpu().numpy() for x in query.split(hits))
    assert tri.dtype == np.int32 and float((tri >= 0).mean()) == rays["share"]
    assert np.array_equal(bits(t[tri < 0]), bits(np.full((tri < 0).sum(), 10e10, np.float32)))
    r8 = torch.full((N, 8), float("nan"), device="cuda")
    r8[:, 0:3] = org
    r8[:, 4:7] = d
    hits8, iters8 = query.trace(rt, r8[:, 0:3], r8[:, 4:7], want_iters=True)
    assert_records(hits8, iters8, rays, what="stride 8")
    cap = W * H
    qt, qtri, qu, qv, qit, _ = rt.trace_rays(rays["org"][:cap], rays["dir"][:cap], want_iters=True)
    got = rec_of(hits8)[:cap]
    assert np.array_equal(got[:, 0], bits(qt)) and np.array_equal(got[:, 1], qtri.view(np.uint32))
    assert np.array_equal(got[:, 2], bits(qu)) and np.array_equal(got[:, 3], bits(qv))
    assert np.array_equal(iters8.cpu().numpy()[:cap].view(np.uint32), qit)
    # the rays whose oracle (u, v) are another triangle's (oracle_records): rt_trace_rays' record, bit for
    # bit, and a point of its own triangle on the ray
    f = np.nonzero(rays["foreign"])[0]
    assert len(f) <= cap
    if len(f):
        ft, ftri, fu, fv, fit, _ = rt.trace_rays(rays["org"][f], rays["dir"][f], want_iters=True)
        for got in (rec_of(hits)[f], rec_of(hits8)[f]):
            assert np.array_equal(got[:, 0], bits(ft)) and np.array_equal(got[:, 1], ftri.view(np.uint32))
            assert np.array_equal(got[:, 2], bits(fu)) and np.array_equal(got[:, 3], bits(fv))
            corners = rt.download("TRI_POS", np.float32).reshape(-1, 3, 4)[:, :, :3].astype(np.float64)
            assert residual(rays["org"][f], rays["dir"][f], got, corners).max() <= FOREIGN_RESIDUAL
    rt.cleanup()


def test_edge_counts(rtx, tmp_path, rays):
    """n in {1, 63, 64, 65, 257} on the default grid: bit-exact prefixes of the oracle's records, and
    the elements past n of an over-allocated hit tensor keep their sentinel.  n = 0 is RT_OK and
    records the done event."""
    import torch

    from rtx import query

    rt = make_rt(rtx, tmp_path)
    rt.build_bvh()
    org, d = to_dev(rays["org"][:300], rays["dir"][:300])
    sentinel = np.float32(-12345.5)
    for n in (1, 63, 64, 65, 257):
        big = torch.full((n + 70, 4), float(sentinel), device="cuda")
        bigi = torch.full((n + 70,), -7, dtype=torch.int32, device="cuda")
        hits = query.trace(rt, org[:n], d[:n], out=big[:n])
        assert hits.data_ptr() == big.data_ptr()
        assert_records(hits, None, rays, n, what=n)
        assert (big[n:] == float(sentinel)).all().item(), n
        rt.trace_rays_device(org.data_ptr(), d.data_ptr(), n, big.data_ptr(), iters_ptr=bigi.data_ptr())
        rt.sync()
        assert_records(big[:n], bigi[:n], rays, n, what=(n, "iters"))
        assert (big[n:] == float(sentinel)).all().item() and (bigi[n:] == -7).all().item(), n
    ev = torch.cuda.Event()
    ev.record()  # creates the handle
    torch.cuda.synchronize()
    rt.trace_rays_device(None, None, 0, None, done_event=ev.cuda_event)
    ev.synchronize()
    empty = query.trace(rt, org[:0], d[:0])
    assert tuple(empty.shape) == (0, 4)
    rt.cleanup()


def test_any_hit(rtx, tmp_path, rays):
    """RT_QUERY_ANY_HIT on the same rays: the closest-hit query's hit / miss answer, no more
    iterations (fewer for some ray), the same record where the counts are equal, t no nearer, and every
    record a point of its triangle on the ray: barycentrics inside the triangle and a residual
    |org + t dir - P(tri, u, v)| within 4x the largest residual of the oracle's closest-hit records of
    these rays (the factor allows for grazing hits farther along a ray).

    Measured on gfx950: 59,978 of the 100,037 rays end earlier, mean 27.1 against 34.6
    iterations; the oracle's largest closest-hit residual is 3.18e-5 (the ray with another triangle's
    barycentrics aside, oracle_records), so the bound is 1.27e-4; the largest any-hit residual is 3.18e-5."""
    from rtx import query

    rt = make_rt(rtx, tmp_path)
    rt.build_bvh()
    org, d = to_dev(rays["org"], rays["dir"])
    hits, iters = query.trace(rt, org, d, any_hit=True, want_iters=True)
    tris = rt.download("TRI_POS", np.float32).reshape(-1, 3, 4)[:, :, :3].astype(np.float64)
    tri_count = rt.info().triCount
    rt.cleanup()
    a = rec_of(hits)
    ai = iters.cpu().numpy().view(np.uint32)
    c, ci = rays["rec"], rays["iters"]
    a_tri, c_tri = a[:, 1].view(np.int32), c[:, 1].view(np.int32)
    assert np.array_equal(a_tri >= 0, c_tri >= 0)
    assert (ai <= ci).all() and (ai < ci).any()
    same = ai == ci
    own = same & ~rays["foreign"]  # (the oracle's (u, v) of a foreign ray are not its hit's: oracle_records)
    assert np.array_equal(a[own], c[own]) and np.array_equal(a[same, :2], c[same, :2])
    hit = a_tri >= 0
    a_t, c_t = a[:, 0].view(np.float32), c[:, 0].view(np.float32)
    assert (a_t[hit] >= c_t[hit]).all()
    assert np.array_equal(a[~hit], c[~hit])

    au, av = a[hit, 2].view(np.float32), a[hit, 3].view(np.float32)
    assert (a_tri[hit] < tri_count).all()
    assert (au >= 0).all() and (av >= 0).all() and (au.astype(np.float64) + av.astype(np.float64) <= 1.0).all()
    # the oracle's closest-hit records of these rays, less the one whose (u, v) are another triangle's
    # (oracle_records; with it the bound would be 4 x 1.4e-2, which bounds nothing)
    bound = 4.0 * rays["res_max"]
    worst = residual(rays["org"], rays["dir"], a, tris).max()
    print("any-hit: %d of %d rays end earlier, mean iterations %.1f vs %.1f; residual bound 4 x %.3e = %.3e, worst %.3e"
          % ((ai < ci).sum(), len(ai), ai.mean(), ci.mean(), bound / 4.0, bound, worst))
    assert worst <= bound, "any-hit residual %.3e over the bound %.3e (4 x the oracle's closest-hit %.3e)" % (
        worst, bound, bound / 4.0)


def displaced(v, sign):
    v2 = v.copy()
    v2[:, 1] += np.float32(sign) * np.float32(0.2) * np.sin(v[:, 0])
    assert v2.dtype == np.float32
    return v2


def test_ordering_against_builds_without_host_sync(rtx, oracle, tmp_path, default_scene, rays):
    """A pipelined context on a torch stream: update(A), build, query, update(B), build, query,
    update(A), build, query, all enqueued without a host sync (the updates on ready events, so that
    nothing but the renderer's own ordering holds the third build, into the set the first query reads,
    behind that query).  Each query equals the oracle on the geometry built just before it."""
    import torch

    from rtx import query

    v, i, n = default_scene["vertices"], default_scene["indices"], default_scene["tri_count"]
    org, d = rays["org"][PICK], rays["dir"][PICK]
    want = {}
    for sign in (1, -1):
        v2 = displaced(v, sign)
        b = oracle.build_bvh(v2, i, n, oracle.smooth_normals(v2, i))
        want[sign] = oracle_records(oracle, b, org, d)
        want[sign]["v"] = v2
    assert not np.array_equal(want[1]["rec"], want[-1]["rec"])
    assert (want[1]["rec"] != want[-1]["rec"]).any(1).mean() > 0.5  # most hits move with the surface
    dorg, ddir, da, db = to_dev(org, d, want[1]["v"], want[-1]["v"])
    rt = make_rt(rtx, tmp_path)
    prev = torch.cuda.current_stream(0)
    main, post = torch.cuda.Stream(device=0), torch.cuda.Stream(device=0)
    try:
        torch.cuda.set_stream(main)
        rt.set_stream(main.cuda_stream)
        rt.set_post_stream(post.cuda_stream)
        ready = torch.cuda.Event()
        ready.record(prev)  # the positions exist (to_dev synchronised)
        got = []
        for dv in (da, db, da):
            rt.update_vertices_device(dv.data_ptr(), len(v), 0, ready.cuda_event)
            rt.build_bvh()
            got.append(query.trace(rt, dorg, ddir, want_iters=True))
        torch.cuda.synchronize()
        for k, sign in enumerate((1, -1, 1)):
            assert_records(got[k][0], got[k][1], want[sign], what=("query", k))
    finally:
        rt.cleanup()
        torch.cuda.set_stream(prev)


FW, FH, FSPP, FRAMES = 128, 72, 4, 6


def _pipeline(rtx, tmp_path, rays, queries, read_each):
    """FramePipeline frames 1..6 at 128x72, 4 spp, a 4,096-ray query behind every frame() when asked.
    read_each: RGBA8 and HDR of every frame (each read drains the streams); otherwise only the last
    frame's, with frames and queries enqueued back to back.  Then the last frame's PT_QUEUE counters."""
    import torch

    from rtx import query
    from rtx.frames import FramePipeline

    dorg, ddir = to_dev(rays["org"][PICK], rays["dir"][PICK])
    rt = make_rt(rtx, tmp_path, FW, FH, spp=FSPP)
    prev = torch.cuda.current_stream(0)
    out, hits = [], []

    def read():
        return rt.download("RGBA8", np.uint8).copy(), rt.download("HDR", np.uint32).copy()

    try:
        fp = FramePipeline(rt, torch.device("cuda", 0), pipelined=True)
        for f in range(1, FRAMES + 1):
            fp.frame(f, hdr=True)
            if queries:
                hits.append(query.trace(rt, dorg, ddir, want_iters=True))
            if read_each:
                out.append(read())
        fp.finish()
        if not read_each:
            out.append(read())
        counters = rt.download("PT_QUEUE", np.uint32).copy()
        rays_counted = rt.ray_count()
    finally:
        rt.cleanup()
        torch.cuda.set_stream(prev)
    return out, counters, rays_counted, hits


def test_queries_do_not_disturb_pipelined_frames(rtx, tmp_path, rays):
    """Pipelined frames 1..6 with a query after every frame equal the frames without queries: every
    frame's RGBA8 and HDR read frame by frame, the last frame's when nothing is read in between, the
    last frame's PT_QUEUE counters and the ray count; every query equals the oracle."""
    for read_each in (True, False):
        plain, pc, pr, _ = _pipeline(rtx, tmp_path, rays, False, read_each)
        with_q, qc, qr, hits = _pipeline(rtx, tmp_path, rays, True, read_each)
        assert len(plain) == len(with_q) == (FRAMES if read_each else 1)
        for f, (a, b) in enumerate(zip(plain, with_q)):
            assert np.array_equal(a[0], b[0]), (read_each, f + 1, "RGBA8")
            assert np.array_equal(a[1], b[1]), (read_each, f + 1, "HDR")
        assert np.array_equal(pc, qc), read_each
        assert pr == qr and pr > 0, read_each
        assert len(hits) == FRAMES
        for k, (h, it) in enumerate(hits):
            assert_records(h, it, rays, PICK, what=(read_each, "query", k + 1))


def _sync_draws(rtx, tmp_path, rays, queries):
    """Synchronous rt.draw() frames 1..6 (the default [tuning] syncSpec: the next frame's LBVH and
    camera rays are prepared ahead), one query between consecutive draws when asked."""
    from rtx import query

    dorg, ddir = to_dev(rays["org"][PICK], rays["dir"][PICK])
    rt = make_rt(rtx, tmp_path, FW, FH, spp=FSPP)
    frames, hits = [], []
    for f in range(1, FRAMES + 1):
        rgba, hdr = np.zeros((FH, FW, 4), np.uint8), np.zeros((FH, FW, 4), np.float32)
        rt.draw(rgba, hdr)
        frames.append((rgba, hdr.view(np.uint32)))
        if queries and f < FRAMES:
            hits.append(query.trace(rt, dorg, ddir, want_iters=True))
    counters = rt.download("PT_QUEUE", np.uint32).copy()
    rt.cleanup()
    return frames, counters, hits


def test_queries_do_not_disturb_synchronous_draws(rtx, tmp_path, rays):
    """Synchronous draws with a query between consecutive draws equal the draws without: the query
    drains nothing, so what each draw prepared ahead for the next is still used, and it leaves the
    counter blocks alone.  Then a query followed by two more draws before anything waits for it (the
    second of them prebuilds into the LBVH set the query reads) still equals the oracle."""
    from rtx import query

    plain, pc, _ = _sync_draws(rtx, tmp_path, rays, False)
    with_q, qc, hits = _sync_draws(rtx, tmp_path, rays, True)
    for f, (a, b) in enumerate(zip(plain, with_q)):
        assert np.array_equal(a[0], b[0]), (f + 1, "RGBA8")
        assert np.array_equal(a[1], b[1]), (f + 1, "HDR")
    assert np.array_equal(pc, qc)
    assert len(hits) == FRAMES - 1
    for k, (h, it) in enumerate(hits):
        assert_records(h, it, rays, PICK, what=("between draws", k + 1))
    for tuning in (None, dict(syncSpec=False)):  # with and without the camera rays traced ahead
        dorg, ddir = to_dev(rays["org"][PICK], rays["dir"][PICK])
        rt = make_rt(rtx, tmp_path, FW, FH, spp=FSPP, tuning=tuning)
        rgba = np.zeros((FH, FW, 4), np.uint8)
        rt.draw(rgba)
        h, it = query.trace(rt, dorg, ddir, want_iters=True)
        rt.draw(rgba)
        rt.draw(rgba)
        assert_records(h, it, rays, PICK, what=("two draws later", tuning))
        assert np.array_equal(rgba, plain[2][0]), tuning
        rt.cleanup()


def test_query_from_another_torch_stream(rtx, tmp_path, rays):
    """rtx.query.trace from a torch stream that is not the renderer's: the origins are written on that
    stream right before the call (over a tensor of other values) and nothing synchronises the host
    in between; the records are the oracle's, and a copy enqueued on that stream right after reads them."""
    import torch

    from rtx import query

    m = 20011
    src_o, src_d = to_dev(rays["org"][:m], rays["dir"][:m])
    rt = make_rt(rtx, tmp_path)  # on its own stream
    rt.build_bvh()
    other = torch.cuda.Stream(device=0)
    with torch.cuda.stream(other):
        org = torch.full((m, 3), 1.0e6, device="cuda")  # from out there every ray misses
        big = torch.empty((64, m, 3), device="cuda")
        for k in range(64):  # work ahead of the fill, so the fill is late on this stream
            big[k].copy_(src_o)
        org.copy_(big[63])
        hits, iters = query.trace(rt, org, src_d, want_iters=True)
        snapshot = hits.clone()
    torch.cuda.synchronize()
    assert_records(snapshot, iters, rays, m, what="other stream")
    assert_records(hits, None, rays, m, what="other stream, in place")
    rt.cleanup()
