"""Emitter sampling on the GPU (rt_set_emitter_sampling).

The oracle has no emitter sampling, so every expectation is exact by construction or in closed form:
the list against numpy, rt_emitter_weight and the oracle's scan, bit for bit; q = 0 and an inert table
against the frame with sampling off, bit for bit; every emitter shadow ray against a float64 ray-triangle
test of the light it names; its throughput against the closed form of the pdf in the room
(tests/emitter_scenes.py), where the light is horizontal at height h over a flat floor; its pixel
against a float64 brute-force classification of the ray; E against 2 E; and three stream plans against
each other.  The path tracer's error counter (PT_QUEUE[10]) is 0 after every launch.
"""
import numpy as np
import pytest

import emitter_scenes as S
import material_scenes as M
from bvh_check import brute_force_hits
from scene_bin import write_bin
from test_gpu_materials import MIX8, terrain_rt, trace
from test_gpu_pathtrace import assert_gbuffers_equal

pytestmark = pytest.mark.gpu

W, H = S.W, S.H
DT = 16.667
HALF_MIN_NORMAL = 2.0 ** -14
SHADOW, EMITTER = 1, 1 << 7
LAMP_TRIS = np.arange(S.LAMP.start, S.LAMP.stop)


# ---------------------------------------------------------------- helpers
@pytest.fixture(scope="module")
def room_bin(tmp_path_factory):
    return write_bin(str(tmp_path_factory.mktemp("room") / "room.bin"), S.room_triangles())


def room_rt(rtx, oracle, tmp_path, room_bin, name, on=True, q=0.5, emission=S.E, extra="", tuning=None, build=True):
    cfg = rtx.write_config(str(tmp_path / (name + ".toml")), W, H, mesh_file=room_bin, extra=extra, tuning=tuning)
    rt = rtx.RayTracer(W, H, cfg).init()
    rt.set_delta_time(DT)
    assert rt.info().triCount == S.N_TRIS
    rt.camera = S.room_camera(rtx, oracle)[1]
    rt.set_triangle_materials(S.room_ids())
    for mid, m in S.room_materials(rtx, emission).items():
        rt.set_materials(mid, [m])
    if on is not None:
        rt.set_emitter_sampling(on, q)
        assert rt.emitter_sampling == (on, np.float32(q))
    if build:
        rt.build_bvh()
    return rt


def emitter_arrays(rt):
    return (rt.download("EMITTER_TRIS", np.uint32).copy(), rt.download("EMITTER_WEIGHTS", np.float32).copy(),
            rt.download("EMITTER_CDF", np.float32).copy())


def mesh_triangles(rt):
    """(triCount, 3, 3) float32 corner positions of the current mesh."""
    v = rt.download("VERTICES", np.float32).reshape(-1, 3)
    i = rt.download("INDICES", np.uint32).reshape(-1, 3)[:rt.info().triCount]
    return v[i.astype(np.int64)]


def check_list(rtx, oracle, rt, want_tris, emission):
    """The downloads of the last build against numpy, rt_emitter_weight and the oracle's scan."""
    tris, weights, cdf = emitter_arrays(rt)
    assert tris.dtype == np.uint32 and np.array_equal(tris, np.asarray(want_tris, np.uint32))
    xyz = mesh_triangles(rt)
    want_w = np.array([rtx.emitter_weight(xyz[t], emission) for t in want_tris], np.float32)
    assert (want_w > 0).all()
    assert np.array_equal(weights.view(np.uint32), want_w.view(np.uint32))
    n = rt.info().triCount
    P = 256
    while P < n:
        P *= 2
    assert cdf.size == P
    padded = np.zeros(P, np.float32)
    padded[:len(want_w)] = want_w
    assert np.array_equal(cdf.view(np.uint32), oracle.scan(padded, 256).view(np.uint32))
    return tris, weights, cdf


def queue(rt, k):
    """Entries of queue k (3 or 4) of the last launch: origins, directions, pixel, flags."""
    n = int(rt.download("PT_QUEUE", np.uint32)[k - 3])
    o = rt.download("PT_Q%d_ORIGINS" % k, np.float32).reshape(-1, 4)[:n].copy()
    d = rt.download("PT_Q%d_DIRS" % k, np.float32).reshape(-1, 4)[:n].copy()
    out = dict(n=n, org=o[:, :3], dir=d[:, :3], pixel=o[:, 3].copy().view(np.uint32), flags=d[:, 3].copy().view(np.uint32))
    if k == 3:
        out["beta1"] = rt.download("PT_Q3_BETA", np.float32).reshape(-1, 4)[:n, :3].copy()
    return out


def barycentrics(tri, org, dir):
    """float64 (u, v, t) of the rays against one triangle each (tri: (n, 3, 3))."""
    tri, org, dir = (np.asarray(a, np.float64) for a in (tri, org, dir))
    e1, e2 = tri[:, 1] - tri[:, 0], tri[:, 2] - tri[:, 0]
    p = np.cross(dir, e2)
    det = np.einsum("nk,nk->n", p, e1)
    s = org - tri[:, 0]
    u = np.einsum("nk,nk->n", s, p) / det
    qv = np.cross(s, e1)
    v = np.einsum("nk,nk->n", dir, qv) / det
    t = np.einsum("nk,nk->n", qv, e2) / det
    return u, v, t


@pytest.fixture(scope="module")
def room_frames(rtx, oracle, tmp_path_factory, room_bin):
    """The room at q = 1 and q = 0.5, one detail launch each: G-buffers, both queues, the list."""
    tmp = tmp_path_factory.mktemp("frames")
    out = {}
    for q in (1.0, 0.5):
        rt = room_rt(rtx, oracle, tmp, room_bin, "q%d" % int(q * 10), q=q)
        g = trace(rt, 1)
        out[q] = dict(g=g, q3=queue(rt, 3), q4=queue(rt, 4), em=emitter_arrays(rt))
        rt.cleanup()
    return out


# ---------------------------------------------------------------- 1: list and CDF
def test_list_and_cdf_of_the_room(rtx, oracle, tmp_path, room_bin):
    rt = room_rt(rtx, oracle, tmp_path, room_bin, "l1")
    tris, w, cdf = check_list(rtx, oracle, rt, LAMP_TRIS, S.E)
    # all positions doubled and a rebuild: areas, weights and every partial sum exactly x 4
    v = rt.download("VERTICES", np.float32).reshape(-1, 3)
    rt.update_vertices(np.ascontiguousarray(v * np.float32(2.0)))
    rt.build_bvh()
    tris2, w2, cdf2 = emitter_arrays(rt)
    assert np.array_equal(tris2, tris)
    assert np.array_equal(w2, w * np.float32(4.0)) and np.array_equal(cdf2, cdf * np.float32(4.0))
    check_list(rtx, oracle, rt, LAMP_TRIS, S.E)
    rt.cleanup()


def test_list_with_override_holds_every_triangle(rtx, oracle, tmp_path, room_bin):
    rt = room_rt(rtx, oracle, tmp_path, room_bin, "l2", extra="materialOverride = %d\n" % S.ID_LAMP)
    check_list(rtx, oracle, rt, np.arange(S.N_TRIS), S.E)
    rt.cleanup()


def test_list_follows_device_ids_and_the_mesh_on_the_terrain(rtx, oracle, tmp_path):
    import torch

    emission = (0.5, 1.0, 2.0)
    rt, _ = terrain_rt(rtx, oracle, tmp_path, "l3")
    n = rt.info().triCount
    ids = M.hashed_ids(n, (3, 3, 3, 0))
    rt.set_triangle_materials(ids)
    m = rtx.default_material(0)
    m.emission[:] = emission
    rt.set_materials(0, [m])
    rt.set_emitter_sampling(True, 0.5)
    for name in ("EMITTER_TRIS", "EMITTER_WEIGHTS", "EMITTER_CDF"):  # from the next build on
        assert rt.download(name).size == 0
    rt.build_bvh()
    xyz = mesh_triangles(rt)

    def emitters(table):  # the emitting id, and a weight > 0 by the rule itself
        return np.array([t for t in np.nonzero(table == 0)[0] if rtx.emitter_weight(xyz[t], emission) > 0], np.int64)

    want = emitters(ids)
    assert 0.2 * n < len(want) < 0.3 * n
    check_list(rtx, oracle, rt, want, emission)
    # the emitting id moved to other triangles on the device: the list follows at the next build
    ids2 = M.hashed_ids(n, (3, 0, 3, 3))
    assert not np.array_equal(ids2, ids)
    dev = torch.from_numpy(ids2).to("cuda")
    torch.cuda.synchronize()
    rt.set_triangle_materials_device(dev.data_ptr(), n, 0, rtx.MAT_CLASS_ALL)
    assert np.array_equal(rt.download("EMITTER_TRIS", np.uint32), want.astype(np.uint32))  # the last build's still
    rt.build_bvh()
    check_list(rtx, oracle, rt, emitters(ids2), emission)
    # a new mesh: the ids are back to 3, which does not emit: an empty list
    cube = M.cube_triangles()
    rt.set_mesh(np.ascontiguousarray(cube.reshape(-1, 3)), np.arange(3 * len(cube), dtype=np.uint32).reshape(-1, 3))
    rt.build_bvh()
    tris, w, cdf = emitter_arrays(rt)
    assert tris.size == 0 and w.size == 0
    assert cdf.size == 1024 and not cdf.any()
    rt.path_trace(1, detail=True)  # an empty list is never sampled
    rt.sync()
    assert rt.download("PT_QUEUE", np.uint32)[10] == 0
    rt.cleanup()


# ---------------------------------------------------------------- 2: identities
def test_q_zero_equals_sampling_off(rtx, oracle, tmp_path, room_bin):
    off = room_rt(rtx, oracle, tmp_path, room_bin, "i0", on=False)
    for name in ("EMITTER_TRIS", "EMITTER_WEIGHTS", "EMITTER_CDF"):
        assert off.download(name).size == 0
    want = trace(off, 1)
    off.cleanup()
    never = room_rt(rtx, oracle, tmp_path, room_bin, "i1", on=None)
    assert_gbuffers_equal(trace(never, 1), want)
    never.cleanup()
    on = room_rt(rtx, oracle, tmp_path, room_bin, "i2", on=True, q=0.0)
    assert on.download("EMITTER_TRIS", np.uint32).size == 8
    got = trace(on, 1)
    f3 = queue(on, 3)["flags"]
    on.cleanup()
    assert_gbuffers_equal(got, want)
    assert f3.size > 300 and not (f3 & EMITTER).any()


def test_inert_table_equals_sampling_off_on_the_terrain(rtx, oracle, tmp_path):
    frames = []
    for on in (False, True):
        rt, _ = terrain_rt(rtx, oracle, tmp_path, "t%d" % on)
        rt.set_triangle_materials(M.hashed_ids(rt.info().triCount, MIX8))
        rt.set_materials(0, [rtx.default_material(i) for i in range(256)])  # no emission: the feature is inert
        rt.set_emitter_sampling(on, 0.5)
        rt.build_bvh()
        assert rt.download("EMITTER_CDF").size == 0
        frames.append(trace(rt, 1))
        rt.cleanup()
    assert_gbuffers_equal(frames[1], frames[0])


# ---------------------------------------------------------------- 3: every emitter shadow ray points at its light
def test_every_emitter_shadow_ray_points_at_its_light(room_frames):
    tri_xyz = S.room_triangles()
    n3 = 0
    for q in (1.0, 0.5):
        f = room_frames[q]
        em_tris = f["em"][0]
        assert np.array_equal(em_tris, LAMP_TRIS)
        for k in ("q3", "q4"):
            e = f[k]
            shadow = (e["flags"] & SHADOW) != 0
            em = (e["flags"] & EMITTER) != 0
            assert not (em & ~shadow).any()  # only a shadow ray samples a light
            env = shadow & ~em
            assert ((e["flags"][env] >> 16) == 9999).all()
            assert ((e["flags"][~shadow] >> 16) == 7777).all()
            if q == 1.0:
                assert not env.any()  # every light sample went to the list
            light = (e["flags"][em] >> 8).astype(np.int64)
            assert np.isin(light, em_tris).all()
            u, v, t = barycentrics(tri_xyz[light], e["org"][em], e["dir"][em])
            assert (t > 0).all()
            assert (u >= -1e-4).all() and (v >= -1e-4).all() and (u + v <= 1 + 1e-4).all()
            if q == 1.0 and k == "q3":
                n3 = int(em.sum())
                assert len(set(light.tolist())) == 8  # every lamp triangle is selected
        if q == 0.5:
            assert ((f["q3"]["flags"] & (SHADOW | EMITTER)) == SHADOW).sum() > 100  # both strategies run
    print("queue-3 emitter entries at q = 1: %d" % n3)
    assert n3 >= 300


# ---------------------------------------------------------------- 4: the pdf, in closed form
def floor_emitter_entries(f):
    """Queue-3 emitter entries whose ray leaves the floor."""
    e = f["q3"]
    return np.nonzero(((e["flags"] & EMITTER) != 0) & (np.abs(e["org"][:, 1]) < 1e-3))[0]


@pytest.mark.parametrize("q", [1.0, 0.5])
def test_throughput_is_the_closed_form_of_the_pdf(room_frames, q):
    f = room_frames[q]
    e = f["q3"]
    tris, weights, cdf = f["em"]
    sel = floor_emitter_entries(f)
    dy = e["dir"][sel, 1].astype(np.float64)
    sel, dy = sel[dy >= 0.2], dy[dy >= 0.2]  # above kSafeCos, where cos^4 is well conditioned
    assert len(sel) >= 200
    slot = np.searchsorted(tris, e["flags"][sel] >> 8)
    below = np.where(slot > 0, cdf[np.maximum(slot, 1) - 1], np.float32(0.0)).astype(np.float32)
    pk = ((cdf[slot] - below) / cdf[len(tris) - 1]).astype(np.float64)  # fp32 difference over the total
    xyz = S.room_triangles()[tris[slot].astype(np.int64)].astype(np.float64)
    area = 0.5 * np.linalg.norm(np.cross(xyz[:, 1] - xyz[:, 0], xyz[:, 2] - xyz[:, 0]), axis=1)
    want = (np.asarray(S.C, np.float64)[None, :] * (area * dy ** 4 / (np.pi * q * pk * S.H_LAMP ** 2))[:, None])
    got = e["beta1"][sel].astype(np.float64)
    rel = np.abs(got - want) / want
    print("q = %g: %d entries, worst relative error %.3g (bound 1e-4)" % (q, len(sel), rel.max()))
    for k in np.argsort(rel.max(axis=1))[-3:]:
        print("  entry %d: light %d dy %.6f origin %s beta1 %s closed form %s" % (
            sel[k], e["flags"][sel[k]] >> 8, dy[k], e["org"][sel[k]], got[k], want[k]))
    assert rel.max() <= 1e-4


# ---------------------------------------------------------------- 5: visibility decides the pixel
@pytest.mark.parametrize("q", [1.0, 0.5])
def test_visibility_decides_the_pixel(oracle, room_frames, q):
    f = room_frames[q]
    e, g = f["q3"], f["g"]
    tri_xyz = S.room_triangles()
    sel = floor_emitter_entries(f)
    org, dr = e["org"][sel].astype(np.float64), e["dir"][sel].astype(np.float64)
    light = (e["flags"][sel] >> 8).astype(np.int64)
    # entries whose light-plane point is within 1e-3 of an edge of its triangle, or whose crossing of
    # the occluder's plane is within 1e-3 of the occluder's outline: fp32 may decide them either way
    lt = tri_xyz[light].astype(np.float64)
    _, _, tl = barycentrics(lt, org, dr)
    at_light = org + dr * tl[:, None]
    edge_dist = []
    for a, b in ((0, 1), (1, 2), (2, 0)):
        ab = lt[:, b] - lt[:, a]
        edge_dist.append(np.linalg.norm(np.cross(ab, at_light - lt[:, a]), axis=1) / np.linalg.norm(ab, axis=1))
    near_edge = np.minimum.reduce(edge_dist) < 1e-3
    at1 = org + dr * ((1.0 - org[:, 1]) / dr[:, 1])[:, None]
    (x0, x1), (z0, z1) = S.OCCLUDER_BOX
    dx = np.minimum(np.abs(at1[:, 0] - x0), np.abs(at1[:, 0] - x1))
    dz = np.minimum(np.abs(at1[:, 2] - z0), np.abs(at1[:, 2] - z1))
    in_x = (at1[:, 0] > x0 - 1e-3) & (at1[:, 0] < x1 + 1e-3)
    in_z = (at1[:, 2] > z0 - 1e-3) & (at1[:, 2] < z1 + 1e-3)
    near_outline = ((dx < 1e-3) & in_z) | ((dz < 1e-3) & in_x)
    skip = near_edge | near_outline
    print("q = %g: %d floor entries, %d skipped" % (q, len(sel), skip.sum()))
    assert skip.sum() <= 0.05 * len(sel)
    keep = ~skip
    t, tie, _ = brute_force_hits(tri_xyz, org[keep], dr[keep])
    closest = np.argmax(tie, axis=1)
    assert np.isfinite(t).all()
    lit = closest == light[keep]
    pix = e["pixel"][sel][keep].astype(np.int64)
    assert len(set(pix.tolist())) == len(pix)  # 1 spp: one entry per pixel
    color = oracle.h2f(np.ascontiguousarray(g["color"][pix, :3])).astype(np.float64)
    albedo = oracle.h2f(np.ascontiguousarray(g["albedo"][pix, :3])).astype(np.float64)
    beta1 = e["beta1"][sel][keep].astype(np.float64)
    print("lit %d, occluded %d (by the occluder %d)" % (lit.sum(), (~lit).sum(), ((closest[~lit] >= S.OCCLUDER.start) & (closest[~lit] < S.OCCLUDER.stop)).sum()))
    assert lit.sum() >= 200 and (~lit).sum() >= 30
    want = np.minimum(np.asarray(S.E, np.float64)[None, :] * beta1[lit], 10.0)
    got = color[lit] * albedo[lit]
    # two half roundings and the product, relative; a colour below the smallest normal half rounds in absolute steps
    miss = np.nonzero((np.abs(got - want) > 2.0 ** -9 * want + 2.0 ** -23).any(axis=1))[0]
    print("lit entries off the closed form: %d" % len(miss))
    for k in miss[:6]:
        j = np.nonzero(keep)[0][np.nonzero(lit)[0][k]]
        print("  pixel %d origin %s dir %s light %d t %.6f edge distance %.5f colour x albedo %s E beta1 %s" % (
            pix[lit][k], org[j], dr[j], light[j], tl[j], np.minimum.reduce(edge_dist)[j], got[k], want[k]))
    assert (np.abs(got - want) <= 2.0 ** -9 * want + 2.0 ** -23).all()
    assert (want > 0).all()
    assert (g["color"][pix[~lit], :3] == 0).all()


# ---------------------------------------------------------------- 6: linearity
def test_emission_scales_the_frame_linearly(rtx, oracle, tmp_path, room_bin):
    rt = room_rt(rtx, oracle, tmp_path, room_bin, "ln", q=0.5)
    frames = []
    for scale in (1.0, 2.0):
        rt.set_materials(S.ID_LAMP, [S.room_materials(rtx, tuple(scale * x for x in S.E))[S.ID_LAMP]])
        rt.build_bvh()
        g = trace(rt, 1)
        cnt = rt.download("PT_QUEUE", np.uint32)[:2].copy()
        q3 = queue(rt, 3)
        frames.append((g, cnt, q3["flags"][np.argsort(q3["pixel"], kind="stable")], emitter_arrays(rt)))
    rt.cleanup()
    (one, c1, f1, em1), (two, c2, f2, em2) = frames
    assert np.array_equal(c1, c2) and np.array_equal(f1, f2)  # doubling every weight changes no selection
    assert np.array_equal(em2[1], em1[1] * np.float32(2.0)) and np.array_equal(em2[2], em1[2] * np.float32(2.0))
    for k in ("normal", "albedo", "depth", "motion", "rays"):
        assert np.array_equal(one[k], two[k]), k
    assert np.array_equal(one["color"][:, 3], two["color"][:, 3])
    a = oracle.h2f(np.ascontiguousarray(one["color"][:, :3]))
    b = oracle.h2f(np.ascontiguousarray(two["color"][:, :3]))
    same = one["color"][:, :3] == two["color"][:, :3]
    doubled = (b == a * np.float32(2.0)) & ~same
    sub = (np.abs(a) < HALF_MIN_NORMAL) & (a != 0)
    bad = ~(same | doubled | sub)
    assert not bad.any(), "%d channels neither equal nor doubled" % bad.sum()
    skipped = (sub & ~same & ~doubled).any(axis=1)
    print("doubled pixels %d, subnormal pixels skipped %d" % (doubled.any(axis=1).sum(), skipped.sum()))
    assert doubled.all(axis=1).sum() > 500  # the lamp lights the floor through its shadow rays
    assert skipped.sum() <= W * H // 100


# ---------------------------------------------------------------- 7: plans, streams, lists in flight
FRAMES = 5


def moving_lamp(k):
    """Vertex positions of frame k + 1: the lamp moved by 0.25 per frame."""
    return np.ascontiguousarray(S.room_triangles(lamp_dx=0.25 * k).reshape(-1, 3))


def hdr_sequence(rtx, oracle, tmp_path, room_bin, name, mode):
    tuning = {"syncSpec": mode == "spec"} if mode != "pipelined" else None
    rt = room_rt(rtx, oracle, tmp_path, room_bin, name, q=0.5, tuning=tuning, build=False)
    post = None
    if mode == "pipelined":
        import torch

        post = torch.cuda.Stream(device=0)
        rt.set_post_stream(post.cuda_stream)
    hdr = np.zeros((H, W, 4), np.float32)
    seq = []
    for k in range(FRAMES):
        rt.update_vertices(moving_lamp(k))
        if mode == "pipelined":
            rt.build_bvh()
            rt.path_trace(k + 1)
            rt.denoise_post(k + 1, True)
            seq.append(rt.download("HDR", np.uint32).copy())
        else:
            rt.draw(None, hdr)
            seq.append(hdr.view(np.uint32).reshape(-1).copy())
        assert rt.download("PT_QUEUE", np.uint32)[10] == 0
        assert rt.download("EMITTER_TRIS", np.uint32).size == 8
    rt.cleanup()
    return seq


def test_plans_and_streams_give_one_sequence(rtx, oracle, tmp_path, room_bin):
    ref = hdr_sequence(rtx, oracle, tmp_path, room_bin, "s0", "nospec")
    for k in range(1, FRAMES):
        assert not np.array_equal(ref[k], ref[k - 1])  # the lamp moves
    for name, mode in (("s1", "spec"), ("s2", "pipelined")):
        got = hdr_sequence(rtx, oracle, tmp_path, room_bin, name, mode)
        for k in range(FRAMES):
            assert np.array_equal(got[k], ref[k]), "%s, frame %d" % (mode, k + 1)


def test_unread_draws_keep_the_list_of_their_build(rtx, oracle, tmp_path, room_bin):
    """Asynchronous draws into five targets with nothing read in between: every frame in flight traces
    the list of its own build.  The RGBA8 sequence equals the synchronous draws'."""
    import torch

    def run(asynchronous):
        rt = room_rt(rtx, oracle, tmp_path, room_bin, "u%d" % asynchronous, q=0.5, build=False)
        targets = [torch.zeros((H, W, 4), dtype=torch.uint8, device="cuda") for _ in range(FRAMES)]
        torch.cuda.synchronize()
        for k in range(FRAMES):
            rt.update_vertices(moving_lamp(k))
            rt.draw_device(targets[k].data_ptr(), 0, asynchronous)
        rt.sync()
        assert rt.download("PT_QUEUE", np.uint32)[10] == 0
        rt.cleanup()
        return [t.cpu().numpy() for t in targets]

    want, got = run(False), run(True)
    for k in range(FRAMES):
        assert np.array_equal(got[k], want[k]), "frame %d" % (k + 1)
    assert not np.array_equal(want[0], want[FRAMES - 1])
