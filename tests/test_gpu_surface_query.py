"""Surface queries (rt_trace_surfaces_device, csrc/surface_rays.hip, rtx.query) vs the CPU oracle, bit
for bit: hit position and ray offset, geometric and shading normal, material / front-face / hit word,
the hit point's displacement, and their ordering against builds, vertex updates, material sets and
frames without a host sync.

Every case runs on the default 60,800-triangle scene with a 64x36 context and the 4,097 rays of
surface_scenes.ray_set (not a multiple of 64 or 256; hit share 0.699, both facings, shading normals
that differ from the geometric ones)."""
import numpy as np
import pytest

from surface_scenes import FRONT_BIT, HIT_BIT, MISS, bits, oracle_hits, pack_surfaces, ray_set
from test_gpu_ray_query import DT, H, W, make_rt, to_dev

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def rays(oracle, default_scene):
    return ray_set(oracle, default_scene)


def u32(t):
    """uint32 bit patterns of a device float tensor."""
    return t.cpu().numpy().view(np.uint32)


def assert_surfaces(surf, want, what=""):
    got = u32(surf)
    assert got.shape == want.shape, (what, got.shape)
    for c, name in ((slice(0, 3), "pos"), (3, "offset"), (slice(4, 7), "normal"), (7, "ndr"),
                    (slice(8, 11), "fakeNormal"), (11, "word")):
        assert np.array_equal(got[:, c], want[:, c]), (what, name)


def test_closest_hit_parity(rtx, tmp_path, rays):
    """The fused call: hit records equal to rt_trace_rays_device's and to the oracle's, surfaces equal to
    the oracle's with material 3, from packed stride-3 arrays and from one interleaved (n, 8) tensor; the
    iteration counts are the oracle's."""
    import torch

    from rtx import query

    rt = make_rt(rtx, tmp_path)
    rt.build_bvh()
    org, d = to_dev(rays["org"], rays["dir"])
    plain = query.trace(rt, org, d)
    hits, surf, iters = query.trace(rt, org, d, surface=True, want_iters=True)
    assert tuple(surf.shape) == (len(org), 12) and surf.dtype == torch.float32
    assert np.array_equal(u32(hits), u32(plain)) and np.array_equal(u32(hits), rays["rec"])
    assert np.array_equal(iters.cpu().numpy().view(np.uint32), rays["o"]["iterations"])
    assert_surfaces(surf, rays["surf"], "packed")
    r8 = torch.full((len(org), 8), float("nan"), device="cuda")
    r8[:, 0:3] = org
    r8[:, 4:7] = d
    hits8, surf8 = query.trace(rt, r8[:, 0:3], r8[:, 4:7], surface=True)
    assert np.array_equal(u32(hits8), rays["rec"])
    assert_surfaces(surf8, rays["surf"], "stride 8")
    # the views on the device's records
    hit = rays["hit"]
    assert np.array_equal(query.is_hit(surf).cpu().numpy(), hit)
    assert np.array_equal(query.front_face(surf).cpu().numpy(), rays["o"]["intoSurface"] != 0)
    assert np.array_equal(query.material(surf).cpu().numpy(), np.where(hit, 3, 0))
    assert np.array_equal(bits(query.position(surf).cpu().numpy()), bits(rays["o"]["pos"]))
    assert np.array_equal(bits(query.shading_normal(surf).cpu().numpy()), bits(rays["o"]["fakeNormal"]))
    rt.cleanup()


def test_the_pass_alone_on_the_oracles_records(rtx, tmp_path, rays):
    """RT_SURFACE_FROM_HITS fed the oracle's own records, uploaded from the host: the same surfaces,
    whatever the tracer does; through rtx.query.surfaces with and without `out`."""
    import torch

    from rtx import query

    rt = make_rt(rtx, tmp_path)
    rt.build_bvh()
    org, d = to_dev(rays["org"], rays["dir"])
    rec = to_dev(rays["rec"].view(np.float32))[0]
    surf = query.surfaces(rt, org, d, rec)
    assert_surfaces(surf, rays["surf"], "from hits")
    assert np.array_equal(u32(rec), rays["rec"])  # the records are input only
    out = torch.full((len(org), 12), -1.0, device="cuda")
    got = query.surfaces(rt, org, d, rec, out=out)
    assert got.data_ptr() == out.data_ptr()
    assert_surfaces(out, rays["surf"], "from hits, out")
    rt.cleanup()


def test_edge_counts(rtx, tmp_path, rays):
    """n in {1, 63, 64, 65, 255, 256, 257}: bit-exact prefixes of the oracle's surfaces, fused and from the
    records, and the elements past n of over-allocated tensors keep their sentinel.  n = 0 is RT_OK, writes
    nothing and records the done event."""
    import torch

    from rtx import query

    rt = make_rt(rtx, tmp_path)
    rt.build_bvh()
    org, d = to_dev(rays["org"][:300], rays["dir"][:300])
    rec = to_dev(rays["rec"][:300].view(np.float32))[0]
    sentinel = -12345.5
    for n in (1, 63, 64, 65, 255, 256, 257):
        for motion, cols in ((False, 12), (True, 16)):
            big = torch.full((n + 70, cols), sentinel, device="cuda")
            bigh = torch.full((n + 70, 4), sentinel, device="cuda")
            hits, surf = query.trace(rt, org[:n], d[:n], surface=True, motion=motion, out=bigh[:n], surface_out=big[:n])
            assert surf.data_ptr() == big.data_ptr() and hits.data_ptr() == bigh.data_ptr()
            assert np.array_equal(u32(hits), rays["rec"][:n]), n
            assert_surfaces(surf[:, :12], rays["surf"][:n], (n, motion))
            assert (big[n:] == sentinel).all().item() and (bigh[n:] == sentinel).all().item(), (n, motion)
            big2 = torch.full((n + 70, cols), sentinel, device="cuda")
            query.surfaces(rt, org[:n], d[:n], rec[:n], motion=motion, out=big2[:n])
            assert torch.equal(big2.view(torch.int32), big.view(torch.int32)), (n, motion)
    ev = torch.cuda.Event()
    ev.record()  # creates the handle
    torch.cuda.synchronize()
    big = torch.full((8, 12), sentinel, device="cuda")
    rt.trace_surfaces_device(None, None, 0, None, None, done_event=ev.cuda_event)
    rt.trace_surfaces_device(org.data_ptr(), d.data_ptr(), 0, rec.data_ptr(), big.data_ptr(), from_hits=True,
                             done_event=ev.cuda_event)
    ev.synchronize()
    rt.sync()
    assert (big == sentinel).all().item()
    hits, surf = query.trace(rt, org[:0], d[:0], surface=True, motion=True)
    assert tuple(hits.shape) == (0, 4) and tuple(surf.shape) == (0, 16)
    assert tuple(query.surfaces(rt, org[:0], d[:0], rec[:0]).shape) == (0, 12)
    rt.cleanup()


def test_any_hit(rtx, tmp_path, rays):
    """RT_QUERY_ANY_HIT in the fused call: the records are rt_trace_rays_device's any-hit records, the
    surfaces those of the pass alone over these records, and where the any-hit record is the closest-hit
    one (at least a quarter of the hits; measured on gfx950: 2,719 of 2,865) the surface is the oracle's."""
    from rtx import query

    rt = make_rt(rtx, tmp_path)
    rt.build_bvh()
    org, d = to_dev(rays["org"], rays["dir"])
    plain = query.trace(rt, org, d, any_hit=True)
    hits, surf = query.trace(rt, org, d, any_hit=True, surface=True)
    again = query.surfaces(rt, org, d, plain)
    a = u32(hits)
    assert np.array_equal(a, u32(plain))
    assert np.array_equal(u32(surf), u32(again))
    same = (a == rays["rec"]).all(1)
    hit = rays["hit"]
    print("any-hit: %d of %d hits have the closest-hit record" % ((same & hit).sum(), hit.sum()))
    assert (same & hit).sum() * 4 >= hit.sum(), ((same & hit).sum(), hit.sum())
    assert same[~hit].all()
    assert np.array_equal(u32(surf)[same], rays["surf"][same])
    got = u32(surf)
    assert np.array_equal((got[:, 11] & HIT_BIT) != 0, hit)  # the same hit / miss answer
    rt.cleanup()


def test_guarded_records(rtx, tmp_path, rays):
    """Records whose index is -1, -2 or triCountPadded are finished as misses: nothing is read through
    them, the surface is the miss surface whatever t, u and v say, and the context stays healthy."""
    from rtx import query

    rt = make_rt(rtx, tmp_path)
    rt.build_bvh()
    np_ = rt.info().triCountPadded
    n = 300
    rec = np.array(rays["rec"][:n])
    idx = np.array([-1, -2, np_], np.int64)[np.arange(n) % 3]
    rec[:, 1] = (idx & 0xFFFFFFFF).astype(np.uint32)
    rec[::2, 0] = bits(np.float32(1.5))[0]  # a finite t does not make them hits
    org, d = to_dev(rays["org"][:n], rays["dir"][:n])
    drec = to_dev(rec.view(np.float32))[0]
    for motion, cols in ((False, 12), (True, 16)):
        surf = query.surfaces(rt, org, d, drec, motion=motion)
        rt.sync()  # RT_OK: raises otherwise
        got = u32(surf)
        assert np.array_equal(got[:, :12], np.broadcast_to(MISS, (n, 12))), motion
        assert not got[:, 12:].any()
    # the context still answers
    assert_surfaces(query.trace(rt, org, d, surface=True)[1], rays["surf"][:n], "after the guarded records")
    rt.cleanup()


def material_ids(n):
    return ((7 * np.arange(n, dtype=np.int64) + 1) % 10).astype(np.uint8)


def test_materials(rtx, tmp_path, rays):
    """The id of a hit is the one the path tracer reads: 3 by default, ids[tri] after a host set and after
    a device set; with query A, a device set of other ids and query B enqueued without a host wait, A
    shows the old ids and B the new; the front-face and hit bits are the oracle's throughout."""
    import torch

    from rtx import query

    rt = make_rt(rtx, tmp_path)
    rt.build_bvh()
    org, d = to_dev(rays["org"], rays["dir"])
    o = rays["o"]
    n = rt.info().triCount
    assert o["objectIdx"].max() < n
    assert_surfaces(query.trace(rt, org, d, surface=True)[1], rays["surf"], "default")
    ids = material_ids(n)
    rt.set_triangle_materials(ids)
    assert_surfaces(query.trace(rt, org, d, surface=True)[1], pack_surfaces(o, ids), "host set")
    ids2 = ((ids.astype(np.int64) + 3) % 10).astype(np.uint8)
    ids3 = ((ids.astype(np.int64) + 5) % 10).astype(np.uint8)
    d2, d3 = to_dev(ids2, ids3)
    rt.set_triangle_materials_device(d2.data_ptr(), n)
    a = query.trace(rt, org, d, surface=True)[1]
    rt.set_triangle_materials_device(d3.data_ptr(), n)
    b = query.trace(rt, org, d, surface=True)[1]
    c = query.surfaces(rt, org, d, to_dev(rays["rec"].view(np.float32))[0])
    torch.cuda.synchronize()
    assert_surfaces(a, pack_surfaces(o, ids2), "device set, query A")
    assert_surfaces(b, pack_surfaces(o, ids3), "device set, query B")
    assert_surfaces(c, pack_surfaces(o, ids3), "device set, from hits")
    hit = rays["hit"]
    assert len(np.unique(query.material(b).cpu().numpy()[hit])) == 10
    rt.cleanup()


def test_material_override(rtx, tmp_path, rays):
    from rtx import query

    cfg = rtx.write_config(str(tmp_path / "ov.toml"), W, H, extra="materialOverride = 5\n")
    rt = rtx.RayTracer(W, H, cfg).init()
    rt.set_delta_time(DT)
    rt.build_bvh()
    rt.set_triangle_materials(material_ids(rt.info().triCount))  # the override wins over the table
    org, d = to_dev(rays["org"], rays["dir"])
    surf = query.trace(rt, org, d, surface=True)[1]
    assert_surfaces(surf, pack_surfaces(rays["o"], 5), "override")
    assert (query.material(surf).cpu().numpy()[rays["hit"]] == 5).all()
    rt.cleanup()


def moved(v):
    """A smooth, non-constant per-vertex offset."""
    v2 = v.copy()
    v2[:, 1] += np.float32(0.05) * np.sin(np.float32(3) * v[:, 0] + np.float32(2) * v[:, 2])
    v2[:, 0] += np.float32(0.02) * np.cos(v[:, 2])
    assert v2.dtype == np.float32
    return v2


def test_motion(rtx, tmp_path, default_scene, rays):
    """RT_SURFACE_MOTION with geometry motion on: zeros on the first build; after rt_update_vertices and a
    build, quad 3 is ((d3 w + d1 u) + d2 v) in float32 with w = (1 - u) - v and d_k = new - old position of
    corner k of the hit triangle, on the device's own records; quads 0..2 are those of the query without
    the flag.  A context that never enabled motion gives zeros."""
    from rtx import query

    v, ind = default_scene["vertices"], default_scene["indices"]
    v2 = moved(v)
    org, d = to_dev(rays["org"], rays["dir"])
    cfg = rtx.write_config(str(tmp_path / "m.toml"), W, H, geometry_motion=True)
    rt = rtx.RayTracer(W, H, cfg).init()
    rt.set_delta_time(DT)
    rt.build_bvh()
    hits, surf = query.trace(rt, org, d, surface=True, motion=True)
    assert tuple(surf.shape) == (len(org), 16)
    assert_surfaces(surf[:, :12], rays["surf"], "first build")
    assert not u32(surf)[:, 12:].any()
    rt.update_vertices(v2)
    rt.build_bvh()
    hits, surf = query.trace(rt, org, d, surface=True, motion=True)
    hits12, surf12 = query.trace(rt, org, d, surface=True)
    rec, s = u32(hits), u32(surf)
    assert np.array_equal(rec, u32(hits12)) and np.array_equal(s[:, :12], u32(surf12))
    tri = rec[:, 1].view(np.int32)
    hit = tri >= 0
    assert 0.5 < hit.mean() < 0.95
    u, w_ = rec[hit, 2].view(np.float32), rec[hit, 3].view(np.float32)
    corners = ind.reshape(-1, 3)[tri[hit]]
    dk = [v2[corners[:, k]] - v[corners[:, k]] for k in range(3)]  # d1, d2, d3
    w = (np.float32(1.0) - u) - w_
    want = (dk[2] * w[:, None] + dk[0] * u[:, None]) + dk[1] * w_[:, None]
    assert want.dtype == np.float32
    assert np.array_equal(s[hit, 12:15], bits(want))
    assert (np.abs(want).max(1) > 1e-3).mean() > 0.9  # the hits did move
    assert not s[hit, 15].any() and not s[~hit, 12:].any()
    assert np.array_equal(query.displacement(surf).cpu().numpy()[hit].view(np.uint32), bits(want))
    rt.cleanup()
    rt = make_rt(rtx, tmp_path, name="nm.toml")  # geometry motion never enabled
    rt.build_bvh()
    rt.update_vertices(v2)
    rt.build_bvh()
    s = u32(query.trace(rt, org, d, surface=True, motion=True)[1])
    assert np.array_equal(s[:, :12], u32(surf12)) and not s[:, 12:].any()
    rt.cleanup()


@pytest.mark.parametrize("pipelined", [False, True], ids=["serial", "pipelined"])
def test_ordering_against_builds_without_host_sync(rtx, oracle, tmp_path, default_scene, rays, pipelined):
    """Surface query A, update_vertices_device, build_bvh, surface query B (with motion), one sync at the
    end: A equals the oracle on the old vertices, B on the new; the build that follows B's, into the set A
    read, is held behind A by the renderer alone."""
    import torch

    from rtx import query

    v, i, n = default_scene["vertices"], default_scene["indices"], default_scene["tri_count"]
    v2 = moved(v)
    b2 = oracle.build_bvh(v2, i, n, oracle.smooth_normals(v2, i))
    o2, rec2 = oracle_hits(oracle, b2, rays["org"], rays["dir"])
    want2 = pack_surfaces(o2)
    assert (want2 != rays["surf"]).any(1).mean() > 0.5
    org, d, dv, dv2 = to_dev(rays["org"], rays["dir"], v, v2)
    cfg = rtx.write_config(str(tmp_path / "o.toml"), W, H, geometry_motion=True)
    rt = rtx.RayTracer(W, H, cfg).init()
    rt.set_delta_time(DT)
    prev = torch.cuda.current_stream(0)
    main, post = torch.cuda.Stream(device=0), torch.cuda.Stream(device=0)
    try:
        torch.cuda.set_stream(main)
        rt.set_stream(main.cuda_stream)
        if pipelined:
            rt.set_post_stream(post.cuda_stream)
        ready = torch.cuda.Event()
        ready.record(prev)  # the positions exist (to_dev synchronised)
        got = []
        for pos in (dv, dv2, dv, dv2):
            rt.update_vertices_device(pos.data_ptr(), len(v), 0, ready.cuda_event)
            rt.build_bvh()
            got.append(query.trace(rt, org, d, surface=True, motion=True))
        rt.sync()
        torch.cuda.synchronize()
        for k, (hits, surf) in enumerate(got):
            rec, want = (rays["rec"], rays["surf"]) if k % 2 == 0 else (rec2, want2)
            assert np.array_equal(u32(hits), rec), k
            assert_surfaces(surf[:, :12], want, ("query", k))
        assert not u32(got[0][1])[:, 12:].any()
        for k in (1, 2, 3):  # each later build moved the vertices
            assert u32(got[k][1])[rays["hit"], 12:15].any()
    finally:
        rt.cleanup()
        torch.cuda.set_stream(prev)


FRAMES = 4


def _pipelined_frames(rtx, tmp_path, seq, rays, queries):
    import torch

    from rtx import query
    from rtx.frames import FramePipeline

    dev = torch.device("cuda", 0)
    base = [torch.from_numpy(a).to(dev) for a in seq]
    org, d = to_dev(rays["org"], rays["dir"])
    cfg = rtx.write_config(str(tmp_path / ("pf%d.toml" % queries)), W, H, spp=2, geometry_motion=True)
    rt = rtx.RayTracer(W, H, cfg).init()
    rt.set_delta_time(DT)
    prev = torch.cuda.current_stream(0)
    out, surfs = [], []
    try:
        fp = FramePipeline(rt, dev, pipelined=True)
        for f, t in enumerate(base, 1):
            fp.frame(f, vertices=t)
            if queries:
                surfs.append(query.trace(rt, org, d, surface=True, motion=True))
            out.append((rt.download("RGBA8", np.uint8).copy(), rt.get_buffer("MOTION", (W * H, 2), np.uint16).copy()))
        fp.finish()
        counters = rt.download("PT_QUEUE", np.uint32).copy()
    finally:
        rt.cleanup()
        torch.cuda.set_stream(prev)
    return out, counters, surfs


def _sync_draws(rtx, tmp_path, seq, rays, queries, read_each):
    """Synchronous draws with a vertex update before every frame of seq, then two draws without one, whose
    launches ahead are reused; a surface query with motion behind every draw when asked.  read_each: the
    RGBA8 image and the motion buffer of every frame (each read waits for the streams, which drops what
    was launched ahead); otherwise every frame's HDR image through rt.draw(None, hdr), which reads nothing
    of the context, and the last frame's RGBA8 and motion buffer."""
    from rtx import query

    org, d = to_dev(rays["org"], rays["dir"])
    cfg = rtx.write_config(str(tmp_path / ("sd%d%d.toml" % (queries, read_each))), W, H, spp=2, geometry_motion=True)
    rt = rtx.RayTracer(W, H, cfg).init()
    rt.set_delta_time(DT)
    out, surfs = [], []
    steps = list(seq) + [None, None]
    for k, t in enumerate(steps):
        if t is not None:
            rt.update_vertices(t)
        if read_each:
            img = np.zeros((H, W, 4), np.uint8)
            rt.draw(img)
        else:
            img = np.zeros((H, W, 4), np.float32)
            rt.draw(None, img)
            img = img.view(np.uint32)
        if queries:
            surfs.append(query.trace(rt, org, d, surface=True, motion=True))
        out.append((img, rt.get_buffer("MOTION", (W * H, 2), np.uint16).copy() if read_each else None))
    stats = rt.download("SPEC_STATS", np.uint32).tolist()  # host state: the read waits for nothing
    out.append((rt.download("RGBA8", np.uint8).copy(), rt.get_buffer("MOTION", (W * H, 2), np.uint16).copy()))
    counters = rt.download("PT_QUEUE", np.uint32).copy()
    rt.cleanup()
    return out, counters, surfs, stats


def test_frames_are_not_disturbed(rtx, oracle, tmp_path, default_scene, rays):
    """Pipelined frames and synchronous draws with geometry motion on and a vertex update every frame,
    with and without a surface query (with motion) behind every frame: the same RGBA8 and motion-buffer
    bits, so no query consumed a displacement a frame was to apply; the launches ahead are reused as
    often; PT_QUEUE's error word is 0.  The queries themselves equal the oracle on each frame's vertices."""
    v, i, n = default_scene["vertices"], default_scene["indices"], default_scene["tri_count"]
    v2 = moved(v)
    seq = [v, v2, v, v2][:FRAMES]
    b2 = oracle.build_bvh(v2, i, n, oracle.smooth_normals(v2, i))
    want = [rays["surf"], pack_surfaces(oracle_hits(oracle, b2, rays["org"], rays["dir"])[0])]
    plain, pc, _ = _pipelined_frames(rtx, tmp_path, seq, rays, False)
    with_q, qc, surfs = _pipelined_frames(rtx, tmp_path, seq, rays, True)
    assert len(plain) == len(with_q) == FRAMES
    for f, (a, b) in enumerate(zip(plain, with_q)):
        assert np.array_equal(a[0], b[0]), ("pipelined", f + 1, "RGBA8")
        assert np.array_equal(a[1], b[1]), ("pipelined", f + 1, "MOTION")
    assert not np.array_equal(plain[0][1], plain[1][1])  # frame 2's motion is displaced
    assert np.array_equal(pc, qc) and qc[10] == 0
    for k, (_, s) in enumerate(surfs):
        assert_surfaces(s[:, :12], want[k % 2], ("pipelined", "query", k + 1))

    for read_each in (True, False):
        plain, pc, _, pstats = _sync_draws(rtx, tmp_path, seq, rays, False, read_each)
        with_q, qc, surfs, qstats = _sync_draws(rtx, tmp_path, seq, rays, True, read_each)
        assert len(plain) == len(with_q) == FRAMES + 3  # the frames, and the last one's buffers read at the end
        for f, (a, b) in enumerate(zip(plain, with_q)):
            assert np.array_equal(a[0], b[0]), ("draws", read_each, f + 1, "RGBA8" if read_each else "HDR")
            assert (a[1] is None) == (b[1] is None)
            if a[1] is not None:
                assert np.array_equal(a[1], b[1]), ("draws", read_each, f + 1, "MOTION")
        assert np.array_equal(pc, qc) and qc[10] == 0
        print("SPEC_STATS without / with queries (read_each %s):" % read_each, pstats, qstats)
        assert pstats == qstats, (read_each, pstats, qstats)
        if not read_each:
            assert qstats[1] >= 1, qstats  # launched ahead, and still reused beside the queries
        else:
            assert not np.array_equal(plain[0][1], plain[1][1])  # frame 2's motion is displaced
        for k, (_, s) in enumerate(surfs):
            assert_surfaces(s[:, :12], want[min(k, FRAMES - 1) % 2], ("draws", read_each, "query", k + 1))


def test_surfaces_from_another_torch_stream(rtx, tmp_path, rays):
    """rtx.query.trace(surface=True) from a torch stream that is not the renderer's: the origins are
    written on that stream right before the call and nothing synchronises the host in between; the
    surfaces are the oracle's, and a copy enqueued on that stream right after reads them."""
    import torch

    from rtx import query

    m = len(rays["org"])
    src_o, src_d = to_dev(rays["org"], rays["dir"])
    rt = make_rt(rtx, tmp_path)  # on its own stream
    rt.build_bvh()
    other = torch.cuda.Stream(device=0)
    with torch.cuda.stream(other):
        org = torch.full((m, 3), 1.0e6, device="cuda")  # from out there every ray misses
        big = torch.empty((256, m, 3), device="cuda")
        for k in range(256):  # work ahead of the fill, so the fill is late on this stream
            big[k].copy_(src_o)
        org.copy_(big[255])
        hits, surf = query.trace(rt, org, src_d, surface=True)
        snapshot = surf.clone()
        again = query.surfaces(rt, org, src_d, hits)
    torch.cuda.synchronize()
    assert np.array_equal(u32(hits), rays["rec"])
    assert_surfaces(snapshot, rays["surf"], "other stream")
    assert_surfaces(surf, rays["surf"], "other stream, in place")
    assert_surfaces(again, rays["surf"], "other stream, from hits")
    rt.cleanup()


def test_spawn_origins(rtx, tmp_path, rays):
    """spawn_origins on the device's surfaces equals its numpy statement, pos + s offset normal with
    s = -1 where dot(direction, normal) < 0: two roundings (the product, the sum), each within 2^-24
    relative, so rtol = 2^-22 covers them with room for the product's error carried into a smaller sum."""
    from rtx import query

    rt = make_rt(rtx, tmp_path)
    rt.build_bvh()
    org, d = to_dev(rays["org"], rays["dir"])
    _, surf = query.trace(rt, org, d, surface=True)
    s = surf.cpu().numpy()
    hit = rays["hit"]
    # reflected directions leave on the ray's side, the incoming ones go through
    nrm, ndr = s[:, 4:7], s[:, 7:8]
    refl = rays["dir"] - np.float32(2.0) * ndr * nrm
    for dirs, sign in ((refl, 1.0), (np.array(rays["dir"]), -1.0)):
        got = query.spawn_origins(surf, to_dev(dirs)[0]).cpu().numpy()
        side = np.where((dirs.astype(np.float64) * nrm).sum(1) < 0, -1.0, 1.0)
        assert (side[hit] == sign).all()
        want = s[:, 0:3].astype(np.float64) + (s[:, 3].astype(np.float64) * side)[:, None] * nrm
        assert np.allclose(got[hit], want[hit], rtol=2.0 ** -22, atol=0.0)
        assert (got[hit] != s[hit, 0:3]).any(1).all()  # off the surface
    rt.cleanup()
