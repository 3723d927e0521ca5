"""Closest-point queries on the device (rt_closest_points_device, rtx.query.closest).

The expected records are the host's exhaustive evaluation of the shared rule (rtx.closest_points_host)
over the context's own RT_ARR_TRI_POS rows that are leaves of its tree (bvh_check.tree_triangles over
RT_ARR_REORDER) and real triangles, under their own indices.  All eight words of every record are
compared as bit patterns: the traversal, its pruning and the small-stack fallback must not show."""
import numpy as np
import pytest

import limit_scenes
import mesh_scenes
from closest_scenes import FOUND, FRONT, MISS, bits, candidates, expected, extent_of, far_points, mixed_points, triangles_of
from test_gpu_ray_query import DT, H, W, displaced, make_rt, to_dev

pytestmark = pytest.mark.gpu
INF = float("inf")

MESHES = {
    "grid1023": lambda: mesh_scenes.grid(1023),
    "grid1025": lambda: mesh_scenes.grid(1025),
    "soup2": mesh_scenes.soup2,
    "runs_pad": mesh_scenes.DUPLICATE_SHAPES["runs_pad"],
    "all_equal": mesh_scenes.all_equal,
    "chain1201": limit_scenes.chain1201,
    "chain31": limit_scenes.chain31,
}


def records(t):
    """(n, 8) uint32 bit patterns of a device record tensor."""
    return t.cpu().numpy().view(np.uint32)


def small_stack_rt(rtx, tmp_path, cap, name="s.toml"):
    cfg = rtx.write_config(str(tmp_path / name), W, H, extra="\n[debug]\nclosestStack = %d\n" % cap)
    rt = rtx.RayTracer(W, H, cfg).init()
    rt.set_delta_time(DT)
    return rt


def load(rt, name):
    v, idx = MESHES[name]()
    rt.set_mesh(v, idx)
    rt.build_bvh()
    return v, idx


@pytest.fixture(scope="module")
def default_case(rtx, tmp_path_factory):
    """The default scene's candidates, 2,049 mixed points and their records, once for the module."""
    rt = make_rt(rtx, tmp_path_factory.mktemp("closest"))
    rt.build_bvh()
    tris, ids = candidates(rt)
    rt.cleanup()
    pts = mixed_points(tris, 2049)
    want = bits(rtx.closest_points_host(tris, pts, ids=ids)).reshape(-1, 8)
    for a in (tris, ids, pts, want):
        a.setflags(write=False)
    assert len(ids) == 60800
    return dict(tris=tris, ids=ids, pts=pts, want=want, extent=extent_of(tris))


def assert_same(got, want, what):
    bad = np.flatnonzero((got != want).any(1))
    assert len(bad) == 0, (what, len(bad), bad[:8].tolist(), got[bad[:2]].tolist(), want[bad[:2]].tolist())


def test_default_scene_packed_and_interleaved(rtx, tmp_path, default_case):
    import torch

    from rtx import query

    c = default_case
    rt = make_rt(rtx, tmp_path)
    rt.build_bvh()
    (packed,) = to_dev(c["pts"])
    wide = torch.full((len(c["pts"]), 8), float("nan"), device="cuda")
    wide[:, 0:3] = packed
    a = query.closest(rt, packed)
    b = query.closest(rt, wide[:, 0:3])
    out = torch.zeros((len(c["pts"]), 8), device="cuda")
    assert query.closest(rt, wide[:, 0:3], out=out) is out
    torch.cuda.synchronize()
    rt.cleanup()
    for name, t in (("packed", a), ("interleaved", b), ("out", out)):
        assert_same(records(t), c["want"], name)
    w = c["want"]
    found = (w[:, 7] & FOUND) != 0
    assert found.all() and set(np.unique(w[:, 7] & 7)) == set(range(7))  # every feature occurs
    assert np.array_equal(query.closest_position(a).cpu().numpy().view(np.uint32), w[:, 0:3])
    assert np.array_equal(query.distance2(a).cpu().numpy().view(np.uint32), w[:, 3])
    assert np.array_equal(query.closest_tri(a).cpu().numpy(), w[:, 4].view(np.int32))
    assert np.array_equal(query.closest_uv(a).cpu().numpy().view(np.uint32), w[:, 5:7])
    assert np.array_equal(query.closest_feature(a).cpu().numpy(), (w[:, 7] & 7).astype(np.int32))
    assert np.array_equal(query.closest_front(a).cpu().numpy(), (w[:, 7] & FRONT) != 0)
    assert np.array_equal(query.closest_found(a).cpu().numpy(), found)


def test_meshes_through_set_mesh(rtx, tmp_path):
    """257 mixed points on six meshes in one context, the last of them at vertex 0's position, where the
    padding triangles of a count that is no multiple of 4 lie: never reported.  In soup2 they displace
    both real triangles from the tree, as they do for rays: an empty candidate set, every record a miss."""
    from rtx import query

    rt = make_rt(rtx, tmp_path)
    try:
        for name in ("grid1025", "soup2", "runs_pad", "grid1023", "all_equal", "chain1201"):
            v, idx = load(rt, name)
            tris, ids = candidates(rt)
            pts = mixed_points(triangles_of(v, idx), 257, seed=len(idx))
            pts[-1] = v[0]
            want = bits(rtx.closest_points_host(tris, pts, ids=ids)).reshape(-1, 8)
            (dp,) = to_dev(pts)
            got = records(query.closest(rt, dp))
            assert_same(got, want, name)
            tri = got[:, 4].view(np.int32)
            if name == "soup2":  # its two padding triangles sort first and are the tree's two leaves: no candidate
                assert len(ids) == 0 and np.array_equal(got, np.tile(MISS, (257, 1)))
                continue
            assert ((got[:, 7] & FOUND) != 0).all() and (tri >= 0).all() and (tri < len(idx)).all(), name
            assert np.isin(tri, ids).all(), name
            if name in ("chain1201", "all_equal", "runs_pad"):  # the lowest index of the coincident group
                key = {}
                for t, i in zip(tris.reshape(len(tris), -1).view(np.uint32), ids):
                    k = t.tobytes()
                    key[k] = min(key.get(k, 1 << 32), int(i))
                first = np.asarray([key[tris[np.searchsorted(ids, t)].view(np.uint32).tobytes()] for t in tri])
                assert np.array_equal(first, tri), name
                assert len(key) < len(ids), name
    finally:
        rt.cleanup()


def test_far_points(rtx, tmp_path, default_case):
    """129 points at 1,000 to 100,000 times the extent: many triangles share one fp32 d2, and a bound that
    is too tight by an ulp prunes the one with the lowest index."""
    from rtx import query

    rt = make_rt(rtx, tmp_path)
    try:
        rt.build_bvh()
        pts = far_points(default_case["tris"], 129)
        want = bits(rtx.closest_points_host(default_case["tris"], pts, ids=default_case["ids"])).reshape(-1, 8)
        (dp,) = to_dev(pts)
        assert_same(records(query.closest(rt, dp)), want, "default scene")
        ties = 0
        load(rt, "grid1025")
        tris, ids = candidates(rt)
        pts = far_points(tris, 129)
        out = rtx.closest_points_host(tris, pts, ids=ids)
        (dp,) = to_dev(pts)
        assert_same(records(query.closest(rt, dp)), bits(out).reshape(-1, 8), "grid1025")
        for k in range(0, 129, 16):  # the premise: several triangles at the winning d2
            d2 = np.asarray([rtx.point_triangle(pts[k], t)[3] for t in tris])
            assert d2.min() == out[k, 3]
            ties += int((d2 == out[k, 3]).sum() > 1)
        assert ties > 0
    finally:
        rt.cleanup()


def test_small_stack_takes_the_leaf_list(rtx, tmp_path, default_case):
    """[debug] closestStack = 2: nearly every point's descent meets a full stack and rescans the build's
    leaf list.  The records equal the default capacity's and the host's."""
    from rtx import query

    small, full = small_stack_rt(rtx, tmp_path, 2), make_rt(rtx, tmp_path)
    try:
        for rt in (small, full):
            rt.build_bvh()
        c = default_case
        (dp,) = to_dev(c["pts"][:513])
        a, b = records(query.closest(small, dp)), records(query.closest(full, dp))
        assert_same(a, c["want"][:513], "default scene, small stack")
        assert_same(b, a, "default scene, default capacity")
        for name in ("chain31", "chain1201"):
            for rt in (small, full):
                load(rt, name)
            tris, ids = candidates(small)
            pts = mixed_points(tris, 513, seed=41)
            want = bits(rtx.closest_points_host(tris, pts, ids=ids)).reshape(-1, 8)
            (dp,) = to_dev(pts)
            a, b = records(query.closest(small, dp)), records(query.closest(full, dp))
            assert_same(a, want, name + ", small stack")
            assert_same(b, a, name + ", default capacity")
    finally:
        small.cleanup()
        full.cleanup()


def test_max_distance(rtx, tmp_path, default_case):
    from rtx import query

    c = default_case
    pts = c["pts"][:257]
    rt = make_rt(rtx, tmp_path)
    try:
        rt.build_bvh()
        (dp,) = to_dev(pts)
        counts = []
        for md in (0.0, 0.01 * c["extent"], INF):
            want = bits(rtx.closest_points_host(c["tris"], pts, ids=c["ids"], max_distance=md)).reshape(-1, 8)
            got = records(query.closest(rt, dp, max_distance=md))
            assert_same(got, want, md)
            found = (got[:, 7] & FOUND) != 0
            assert np.array_equal(got[~found], np.tile(MISS, (int((~found).sum()), 1))), md
            counts.append(int(found.sum()))
        assert 0 < counts[0] < counts[1] < counts[2] == 257, counts
        assert_same(want, c["want"][:257], "inf")
    finally:
        rt.cleanup()


def test_edge_counts_and_sentinels(rtx, tmp_path, default_case):
    import torch

    from rtx import query

    c = default_case
    rt = make_rt(rtx, tmp_path)
    try:
        rt.build_bvh()
        (dp,) = to_dev(c["pts"][:300])
        for n in (0, 1, 63, 64, 65, 255, 256, 257):
            out = torch.full((n + 2, 8), -7.5, device="cuda")
            got = query.closest(rt, dp[:n], out=out[:n])
            assert got.shape == (n, 8)
            assert_same(records(out[:n]), c["want"][:n], n)
            assert (out[n:] == -7.5).all(), n  # nothing past n is written
        # n == 0: nothing is written, done_event is recorded
        out = torch.full((4, 8), -7.5, device="cuda")
        done = torch.cuda.Event()
        done.record()
        torch.cuda.synchronize()
        rt.closest_points_device(0, 0, 0, done_event=done.cuda_event)
        rt.closest_points_device(dp.data_ptr(), 0, out.data_ptr(), done_event=done.cuda_event)
        done.synchronize()
        assert (out == -7.5).all()
    finally:
        rt.cleanup()


def test_points_that_are_not_finite(rtx, tmp_path, default_case):
    from rtx import query

    c = default_case
    pts = c["pts"][:64].copy()
    k = 0
    for bad in (np.nan, np.inf, -np.inf):
        for axis in range(3):
            pts[2 * k + 1, axis] = bad
            k += 1
    pts[31] = np.nan
    hurt = ~np.isfinite(pts).all(1)
    assert hurt.sum() == 10
    rt = make_rt(rtx, tmp_path)
    try:
        rt.build_bvh()
        (dp,) = to_dev(pts)
        for md in (INF, 1.0):
            got = records(query.closest(rt, dp, max_distance=md))
            assert np.array_equal(got[hurt], np.tile(MISS, (10, 1))), md
            want = bits(rtx.closest_points_host(c["tris"], pts, ids=c["ids"], max_distance=md)).reshape(-1, 8)
            assert_same(got, want, md)
    finally:
        rt.cleanup()


def _geometry(rtx, rt, v, pts):
    """The host's records for pts once vertices v are built into rt (synchronises)."""
    rt.update_vertices(v)
    rt.build_bvh()
    return expected(rtx, rt, pts)


def test_ordering_against_builds_without_host_sync(rtx, tmp_path, default_scene, default_case):
    """update(A), build, query, update(B), build, query, update(A), build, query on a pipelined context,
    enqueued without a host synchronisation: every query answers for the geometry built just before it,
    the first one although the third build writes the set it reads."""
    import torch

    from rtx import query

    v = default_scene["vertices"]
    pts = default_case["pts"][:513]
    va, vb = displaced(v, 1), displaced(v, -1)
    rt = make_rt(rtx, tmp_path)
    prev = torch.cuda.current_stream(0)
    try:
        want = {1: _geometry(rtx, rt, va, pts), -1: _geometry(rtx, rt, vb, pts)}
        assert (want[1] != want[-1]).any(1).mean() > 0.5  # most answers move with the surface
        assert (want[1] != default_case["want"][:513]).any(1).mean() > 0.5
        dp, da, db = to_dev(pts, va, vb)
        main, post = torch.cuda.Stream(device=0), torch.cuda.Stream(device=0)
        torch.cuda.set_stream(main)
        rt.set_stream(main.cuda_stream)
        rt.set_post_stream(post.cuda_stream)
        ready = torch.cuda.Event()
        ready.record(prev)  # the positions exist (to_dev synchronised)
        got = []
        for dv in (da, db, da):
            rt.update_vertices_device(dv.data_ptr(), len(v), 0, ready.cuda_event)
            rt.build_bvh()
            got.append(query.closest(rt, dp))
        torch.cuda.synchronize()
        for k, sign in enumerate((1, -1, 1)):
            assert_same(records(got[k]), want[sign], ("query", k))
    finally:
        rt.cleanup()
        torch.cuda.set_stream(prev)


FW, FH, FSPP, FRAMES = 128, 72, 4, 6


def _pipeline(rtx, tmp_path, pts, queries):
    """FramePipeline frames 1..6 at 128x72, 4 spp, a closest-point query behind every frame() when asked;
    every frame's RGBA8 is read.  Then the PT_QUEUE counters and the ray count."""
    import torch

    from rtx import query
    from rtx.frames import FramePipeline

    (dp,) = to_dev(pts)
    rt = make_rt(rtx, tmp_path, FW, FH, spp=FSPP)
    prev = torch.cuda.current_stream(0)
    out, recs = [], []
    try:
        fp = FramePipeline(rt, torch.device("cuda", 0), pipelined=True)
        for f in range(1, FRAMES + 1):
            fp.frame(f, hdr=True)
            if queries:
                recs.append(query.closest(rt, dp))
                recs.append(query.closest(rt, dp, max_distance=0.5))
            if f % 2 == 0:
                out.append(rt.download("RGBA8", np.uint8).copy())
        fp.finish()
        out.append(rt.download("RGBA8", np.uint8).copy())
        state = (rt.download("PT_QUEUE", np.uint32).copy(), rt.ray_count())
    finally:
        rt.cleanup()
        torch.cuda.set_stream(prev)
    return out, state, recs


def test_queries_do_not_disturb_pipelined_frames(rtx, tmp_path, default_case):
    c = default_case
    pts = c["pts"][:513]
    plain, ps, _ = _pipeline(rtx, tmp_path, pts, False)
    with_q, qs, recs = _pipeline(rtx, tmp_path, pts, True)
    assert len(plain) == len(with_q) == FRAMES // 2 + 1
    for f, (a, b) in enumerate(zip(plain, with_q)):
        assert np.array_equal(a, b), (f, "RGBA8")
    assert np.array_equal(ps[0], qs[0]) and ps[1] == qs[1] and ps[1] > 0
    assert len(recs) == 2 * FRAMES
    near = bits(rtx.closest_points_host(c["tris"], pts, ids=c["ids"], max_distance=0.5)).reshape(-1, 8)
    for k in range(FRAMES):
        assert_same(records(recs[2 * k]), c["want"][:513], ("frame", k + 1))
        assert_same(records(recs[2 * k + 1]), near, ("frame", k + 1, "0.5"))


def test_query_leaves_the_path_tracer_state_alone(rtx, tmp_path, default_case):
    """Synchronous draws with a query between consecutive draws equal the draws without: the query drains
    nothing, so what each draw launched ahead for the next is reused (RT_ARR_SPEC_STATS counts it, equal
    with and without), and RT_ARR_PT_QUEUE and rt_get_ray_count end as they do without queries."""
    from rtx import query

    (dp,) = to_dev(default_case["pts"][:513])
    res = []
    for queries in (False, True):
        rt = make_rt(rtx, tmp_path, FW, FH, spp=FSPP)
        try:
            frames, recs = [], []
            for f in range(4):
                hdr = np.zeros((FH, FW, 4), np.float32)
                rt.draw(None, hdr)  # the HDR image alone: the draw reads nothing of the context back
                frames.append(hdr.view(np.uint32))
                if queries:
                    recs.append(query.closest(rt, dp))
            stats = rt.download("SPEC_STATS", np.uint32).tolist()  # host state: the read waits for nothing
            frames.append(rt.download("RGBA8", np.uint8).copy())
            state = (rt.download("PT_QUEUE", np.uint32).copy(), rt.ray_count())
            for k, r in enumerate(recs):
                assert_same(records(r), default_case["want"][:513], ("after draw", k + 1))
            res.append((frames, stats, state))
        finally:
            rt.cleanup()
    (fa, sa, ta), (fb, sb, tb) = res
    for f in range(5):
        assert np.array_equal(fa[f], fb[f]), f
    assert sa == sb and sa[1] >= 3, (sa, sb)  # every launch ahead was reused, with queries in between too
    assert np.array_equal(ta[0], tb[0]) and ta[1] == tb[1] and ta[1] > 0
