"""Signed distance queries on the device (rt_set_signed_distance, rt_signed_distance_device,
rtx.query.signed_distance).

Everything is compared bit for bit with the host rule (rtx.pseudo_normals, rtx.signed_distance_rule), fed by
the context's own RT_ARR_VERTICES / RT_ARR_INDICES downloads; the closest records with the host's
exhaustive answer over the build's leaves (closest_scenes.expected)."""
import ctypes as C

import numpy as np
import pytest

import sdf_scenes as S
from closest_scenes import FOUND, MISS, bits, expected, mixed_points, triangles_of
from skin_scenes import random_pose, random_skin
from test_gpu_ray_query import DT, H, W, displaced, to_dev

pytestmark = pytest.mark.gpu
INF = float("inf")
FW, FH, FSPP = 128, 72, 2  # the frames of the draw tests
RT_OK, RT_ERR_STATE = 0, -4
MISS4 = np.asarray([0, 0, 0, 0x7F800000], np.uint32)


def make_rt(rtx, tmp_path, on=True, w=W, h=H, spp=1, extra="", name="sd.toml"):
    cfg = rtx.write_config(str(tmp_path / name), w, h, spp=spp, signed_distance=on if on else None, extra=extra)
    rt = rtx.RayTracer(w, h, cfg).init()
    rt.set_delta_time(DT)
    return rt


def mesh_of(rt):
    """(vertices, indices of the real triangles) as the context holds them."""
    v = rt.download("VERTICES", np.float32).reshape(-1, 3)
    idx = rt.download("INDICES", np.uint32).reshape(-1, 3)[:rt.info().triCount]
    return np.ascontiguousarray(v), np.ascontiguousarray(idx)


def device_table(rt):
    return rt.download("PSEUDO_NORMALS", np.float32).reshape(-1, 6, 4)


def assert_table(rtx, rt, what):
    v, idx = mesh_of(rt)
    got, want = device_table(rt), rtx.pseudo_normals(v, idx)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    bad = np.flatnonzero((bits(got) != bits(want)).reshape(len(idx), -1).any(1))
    assert len(bad) == 0, (what, len(bad), bad[:8].tolist(), got[bad[:1]].tolist(), want[bad[:1]].tolist())
    return v, idx, want


def answers(rtx, rt, pts, max_distance=INF):
    """The host's (records, quads) as uint32 for pts on rt's current build."""
    v, idx = mesh_of(rt)
    rec = expected(rtx, rt, pts, max_distance)
    sd = rtx.signed_distance_rule(pts, rec.view(np.float32), v, idx, rtx.pseudo_normals(v, idx))
    return rec, bits(sd)


def words(t):
    return t.cpu().numpy().view(np.uint32)


def assert_same(got, want, what):
    bad = np.flatnonzero((got != want).any(1))
    assert len(bad) == 0, (what, len(bad), bad[:8].tolist(), got[bad[:2]].tolist(), want[bad[:2]].tolist())


def state_of(rt, dp, n=4):
    """The return code of a query of n points, through the C entry point."""
    import torch

    rec, sd = torch.zeros((n, 8), device="cuda"), torch.zeros((n, 4), device="cuda")
    from rtx import ClosestQuery, DistanceQuery

    q = DistanceQuery(ClosestQuery(dp.data_ptr(), 3, n, INF, rec.data_ptr(), None, None), sd.data_ptr(), 0)
    rc = rt.lib.rt_signed_distance_device(rt.h, C.byref(q))
    torch.cuda.synchronize()
    return rc


def test_table_after_init_and_on_every_scene(rtx, tmp_path):
    """[render] signedDistance = true: the default scene's first build (60,800 triangles, 60 batches) and then
    every scene through set_mesh + build, in an order that shrinks after growing."""
    rt = make_rt(rtx, tmp_path)
    try:
        assert rt.signed_distance is True
        rt.build_bvh()
        v, idx, tab = assert_table(rtx, rt, "default")
        assert len(idx) == 60800 and rt.lib.rt_array_bytes(rt.h, rtx.ARR["PSEUDO_NORMALS"]) == 60800 * 96
        for name in ("grid1101", "wedge", "torus", "bad_fan", "grid1100", "fin", "notch", "welded_cube", "grid40", "cube"):
            mv, mi = S.SCENES[name]()
            rt.set_mesh(mv, mi)
            rt.build_bvh()
            v, idx, tab = assert_table(rtx, rt, name)
            assert np.array_equal(idx, mi) and np.array_equal(bits(v), bits(mv)), name
            assert not np.isnan(tab).any() and np.abs(tab).max() > 0.5, name
    finally:
        rt.cleanup()


def test_table_follows_updates_mesh_sets_and_poses(rtx, tmp_path):
    """rt_update_vertices_device, rt_set_mesh_device (torus -> notch) and rt_pose_skin_device, each followed by
    a build: the table is the host rule's over the vertices and indices the context then holds."""
    import torch

    rt = make_rt(rtx, tmp_path)
    try:
        rt.build_bvh()
        v0, _ = mesh_of(rt)
        before = device_table(rt).copy()
        (dv,) = to_dev(displaced(v0, 1))
        rt.update_vertices_device(dv.data_ptr(), len(v0))
        rt.build_bvh()
        assert_table(rtx, rt, "update_vertices_device")
        assert (bits(device_table(rt)) != bits(before)).any()
        tv, ti = S.torus()
        rt.set_mesh(tv, ti)
        rt.build_bvh()
        assert_table(rtx, rt, "torus")
        nv, ni = S.notch()
        dnv, dni = torch.from_numpy(nv).cuda(), torch.from_numpy(ni.view(np.int32)).cuda()
        torch.cuda.synchronize()
        rt.set_mesh_device(dnv.data_ptr(), len(nv), dni.data_ptr(), len(ni))
        rt.build_bvh()
        v, idx, tab = assert_table(rtx, rt, "set_mesh_device")
        assert np.array_equal(idx, ni) and len(tab) == len(ni)
        rt.set_mesh(tv, ti)
        rest, joints, weights = random_skin(len(tv), 3, seed=5, rest=tv)
        rt.set_skin(rest, joints, weights, 3)
        pose = random_pose(3, seed=9, amount=0.5)
        (dm,) = to_dev(pose)
        rt.pose_skin_device(dm, 3)
        rt.build_bvh()
        v, idx, tab = assert_table(rtx, rt, "pose_skin_device")
        assert np.array_equal(bits(v), bits(rtx.skin_vertices(rest, joints, weights, pose))) and not np.array_equal(v, tv)
    finally:
        rt.cleanup()


def test_off_and_enabled_until_the_next_build(rtx, tmp_path):
    """Size 0 and RT_ERR_STATE with the feature off, and after an enable until a build; again after a disable."""
    rt = make_rt(rtx, tmp_path, on=False)
    try:
        (dp,) = to_dev(np.zeros((4, 3), np.float32))
        nbytes = lambda: rt.lib.rt_array_bytes(rt.h, rtx.ARR["PSEUDO_NORMALS"])  # noqa: E731
        assert rt.signed_distance is False
        rt.build_bvh()
        assert nbytes() == 0 and len(device_table(rt)) == 0 and state_of(rt, dp) == RT_ERR_STATE
        rt.signed_distance = True
        assert rt.signed_distance is True
        assert nbytes() == 0 and len(device_table(rt)) == 0 and state_of(rt, dp) == RT_ERR_STATE
        assert "table" in rt.lib.rt_last_error(rt.h).decode()
        rt.build_bvh()
        assert nbytes() == 60800 * 96 and state_of(rt, dp) == RT_OK
        assert_table(rtx, rt, "enabled at run time")
        rt.signed_distance = False
        assert nbytes() == 0 and state_of(rt, dp) == RT_ERR_STATE
        rt.build_bvh()
        assert nbytes() == 0 and state_of(rt, dp) == RT_ERR_STATE
        rt.signed_distance = True
        rt.build_bvh()
        assert state_of(rt, dp) == RT_OK
    finally:
        rt.cleanup()


def test_enable_between_synchronous_draws(rtx, tmp_path):
    """Synchronous draws build the next frame's LBVH ahead.  An enable drops that build, so the draw after it
    builds with a table and a query behind it is answered; a disable likewise ends the answers at once."""
    rt = make_rt(rtx, tmp_path, on=False, w=FW, h=FH)
    try:
        (dp,) = to_dev(np.zeros((4, 3), np.float32))
        hdr = np.zeros((FH, FW, 4), np.float32)
        for _ in range(3):
            rt.draw(None, hdr)
        assert state_of(rt, dp) == RT_ERR_STATE
        rt.signed_distance = True
        assert state_of(rt, dp) == RT_ERR_STATE
        rt.draw(None, hdr)
        assert state_of(rt, dp) == RT_OK
        assert_table(rtx, rt, "draw after enable")
        rt.draw(None, hdr)
        assert state_of(rt, dp) == RT_OK
        rt.signed_distance = False
        assert state_of(rt, dp) == RT_ERR_STATE
        rt.draw(None, hdr)
        assert state_of(rt, dp) == RT_ERR_STATE
    finally:
        rt.cleanup()


def _query_cases(rtx, rt, pts, what, max_distance):
    """n = 1, 127, 128, 129, 1000 at strides 3 and 8, with out tensors guarded behind n; then
    RT_DISTANCE_FROM_RECORDS over the full query's records, and forged records."""
    import torch

    from rtx import query

    want_rec, want_sd = answers(rtx, rt, pts, max_distance)
    (packed,) = to_dev(pts)
    wide = torch.full((len(pts), 8), float("nan"), device="cuda")
    wide[:, 0:3] = packed
    for n in (1, 127, 128, 129, 1000):
        for name, p in (("stride 3", packed[:n]), ("stride 8", wide[:n, 0:3])):
            rec = torch.full((n + 2, 8), -7.5, device="cuda")
            sd = torch.full((n + 2, 4), -7.5, device="cuda")
            r, s = query.signed_distance(rt, p, max_distance=max_distance, out=rec[:n], signed_out=sd[:n])
            assert r.shape == (n, 8) and s.shape == (n, 4)
            assert_same(words(rec[:n]), want_rec[:n], (what, n, name, "records"))
            assert_same(words(sd[:n]), want_sd[:n], (what, n, name, "signed"))
            assert (rec[n:] == -7.5).all() and (sd[n:] == -7.5).all(), (what, n, name)  # nothing past n
    r, s = query.signed_distance(rt, packed, max_distance=max_distance)
    r2, s2 = query.signed_distance(rt, wide[:, 0:3], records=r)
    assert r2 is r
    assert_same(words(s2), words(s), (what, "from records"))
    assert_same(words(r), want_rec, (what, "records are left as they were"))
    assert np.array_equal(query.signed_distance_of(s).cpu().numpy().view(np.uint32), want_sd[:, 3])
    assert np.array_equal(query.pseudo_normal(s).cpu().numpy().view(np.uint32), want_sd[:, 0:3])
    assert np.array_equal(query.inside(s).cpu().numpy(), want_sd[:, 3].view(np.float32) < 0)
    # forged records: the miss record, index -1 under a found word, indices at and past the triangle count, a
    # feature code past 6; the rest stay
    tri_count = rt.info().triCount
    forged = want_rec.copy()
    found = np.flatnonzero((forged[:, 7] & FOUND) != 0)
    assert len(found) > 8
    forged[found[0]] = MISS
    forged[found[1], 4] = 0xFFFFFFFF
    forged[found[2], 4] = tri_count
    forged[found[3], 4] = 0x7FFFFFFF
    forged[found[4], 7] = FOUND | 7
    (df,) = to_dev(forged.view(np.float32))
    _, s3 = query.signed_distance(rt, packed, records=df)
    got = words(s3)
    want = want_sd.copy()
    want[found[:5]] = MISS4
    assert_same(got, want, (what, "forged"))
    return want_rec, want_sd


def test_queries_equal_the_host_rule(rtx, tmp_path):
    """The default scene (every feature, 60 batches) and the torus, whose points surround a closed mesh; an
    infinite max_distance and one that makes some points miss."""
    rt = make_rt(rtx, tmp_path)
    try:
        rt.build_bvh()
        v, idx = mesh_of(rt)
        pts = mixed_points(triangles_of(v, idx), 1000, seed=31)
        rec, sd = _query_cases(rtx, rt, pts, "default", INF)
        assert set(np.unique(rec[:, 7] & 7)) == set(range(7))
        assert 0 < (sd[:, 3].view(np.float32) < 0).sum() < 1000
        tv, ti = S.torus()
        rt.set_mesh(tv, ti)
        rt.build_bvh()
        pts = S.sign_points(tv, ti, 1000)
        rec, sd = _query_cases(rtx, rt, pts, "torus", INF)
        inside = sd[:, 3].view(np.float32) < 0
        assert np.array_equal(inside, S.winding64(tv, ti, pts) > 0.5)  # all 192 triangles are leaves of the tree
        rec, sd = _query_cases(rtx, rt, pts, "torus within 0.05", 0.05)
        miss = (rec[:, 7] & FOUND) == 0
        assert 50 < miss.sum() < 950 and np.array_equal(sd[miss], np.tile(MISS4, (int(miss.sum()), 1)))
    finally:
        rt.cleanup()


def test_small_stack_feeds_the_pass(rtx, tmp_path):
    """[debug] closestStack = 2: the records come from the leaf-list path; the quads are the same."""
    rt = make_rt(rtx, tmp_path, extra="\n[debug]\nclosestStack = 2\n")
    try:
        tv, ti = S.torus()
        rt.set_mesh(tv, ti)
        rt.build_bvh()
        _query_cases(rtx, rt, S.sign_points(tv, ti, 1000), "torus, small stack", INF)
    finally:
        rt.cleanup()


def test_n_zero_and_events(rtx, tmp_path):
    """n == 0 is RT_OK with NULL or real pointers, writes neither tensor and records done_event."""
    import torch

    rt = make_rt(rtx, tmp_path)
    try:
        rt.build_bvh()
        (dp,) = to_dev(np.zeros((4, 3), np.float32))
        rec = torch.full((4, 8), -7.5, device="cuda")
        sd = torch.full((4, 4), -7.5, device="cuda")
        done = torch.cuda.Event()
        done.record()
        torch.cuda.synchronize()
        rt.signed_distance_device(0, 0, 0, 0, done_event=done.cuda_event)
        for from_records in (False, True):
            rt.signed_distance_device(dp.data_ptr(), 0, rec.data_ptr(), sd.data_ptr(), from_records=from_records,
                                      done_event=done.cuda_event)
        done.synchronize()
        torch.cuda.synchronize()
        assert (rec == -7.5).all() and (sd == -7.5).all()
    finally:
        rt.cleanup()


def test_ordering_against_builds_without_host_sync(rtx, tmp_path):
    """update(A), build, query, update(B), build, query, update(A), build, query on a pipelined context,
    enqueued without a host synchronisation: every query answers, records and quads, for the geometry and the
    table built just before it, the first one although the third build writes the set it reads."""
    import torch

    from rtx import query

    rt = make_rt(rtx, tmp_path)
    prev = torch.cuda.current_stream(0)
    try:
        rt.build_bvh()
        v, idx = mesh_of(rt)
        pts = mixed_points(triangles_of(v, idx), 513, seed=43)
        va, vb = displaced(v, 1), displaced(v, -1)
        want = {}
        for sign, vv in ((1, va), (-1, vb)):
            rt.update_vertices(vv)
            rt.build_bvh()
            want[sign] = answers(rtx, rt, pts)
        assert (want[1][1] != want[-1][1]).any(1).mean() > 0.5  # most quads move with the surface
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
            got.append(query.signed_distance(rt, dp))
        torch.cuda.synchronize()
        for k, sign in enumerate((1, -1, 1)):
            assert_same(words(got[k][0]), want[sign][0], ("records", k))
            assert_same(words(got[k][1]), want[sign][1], ("signed", k))
    finally:
        rt.cleanup()
        torch.cuda.set_stream(prev)


def _draws(rtx, tmp_path, on, queries, name):
    """Five synchronous draws at the smoke camera, a query behind each of the last four when asked."""
    from rtx import query

    rt = make_rt(rtx, tmp_path, on=on, w=FW, h=FH, spp=FSPP, name=name)
    try:
        cam = rtx.Camera()
        cam.pos[:] = (8.0, 15.0, -6.0)
        cam.yaw, cam.pitch, cam.focal, cam.aperture, cam.fovX = 0.0, -0.7, 5.0, 0.001, 90.0 * 0.01745329251
        rt.camera = cam
        (dp,) = to_dev(np.asarray([(8.0, 2.0, 3.0), (1.0, 9.0, 1.0), (4.0, -3.0, 4.0), (20.0, 1.0, 20.0)], np.float32))
        frames, codes, quads = [], [], []
        rgba = np.zeros((FH, FW, 4), np.uint8)
        rt.draw(rgba)  # frame 1, read back: the frame the oracle pins
        frames.append(rgba)
        for f in range(4):
            hdr = np.zeros((FH, FW, 4), np.float32)
            rt.draw(None, hdr)  # the HDR image alone: the draw reads nothing of the context back
            frames.append(hdr.view(np.uint32))
            if queries and on:
                quads.append(query.signed_distance(rt, dp)[1])
            elif queries:
                codes.append(state_of(rt, dp))
        stats = rt.download("SPEC_STATS", np.uint32).tolist()
        return frames, stats, codes, [words(q) for q in quads]
    finally:
        rt.cleanup()


def test_feature_off_frames_are_the_oracles_and_queries_leave_the_draws_alone(rtx, oracle, tmp_path, default_scene):
    """A context that never enables the feature draws the frame the existing tests pin (the CPU oracle's,
    bit for bit) and a refused query changes neither the frames nor RT_ARR_SPEC_STATS.  With the feature on,
    frames and launch-ahead counts are the same, with and without queries between the draws."""
    plain = _draws(rtx, tmp_path, False, False, "a.toml")
    refused = _draws(rtx, tmp_path, False, True, "b.toml")
    on_plain = _draws(rtx, tmp_path, True, False, "c.toml")
    on_query = _draws(rtx, tmp_path, True, True, "d.toml")
    cam = oracle.default_camera(FW, FH)
    cam.pos[:] = (8.0, 15.0, -6.0)
    cam.pitch = -0.7
    g = oracle.pathtrace(default_scene["bvh"], FW, FH, frame_num=1, spp=FSPP, cam=cam)
    o = oracle.Denoiser(FW, FH).draw(g, 1, delta_time=DT)
    assert np.array_equal(plain[0][0].reshape(-1, 4), o["rgba"])
    assert refused[2] == [RT_ERR_STATE] * 4
    for other in (refused, on_plain, on_query):
        for f in range(5):
            assert np.array_equal(plain[0][f], other[0][f]), f
        assert other[1] == plain[1], (other[1], plain[1])
    assert plain[1][1] >= 3  # every launch ahead was reused
    assert len(on_query[3]) == 4 and all(np.array_equal(q, on_query[3][0]) for q in on_query[3])
    assert np.isfinite(on_query[3][0][:, 3].view(np.float32)).all()
