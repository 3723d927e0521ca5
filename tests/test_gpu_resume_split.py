"""The split resume<3> ([tuning] resumeSplit): k_trace_queue<3> lists the queue-3
entries whose resume can shade (a bounce ray that hit a triangle), k_pt_resume3_shade runs over that
list and k_pt_resume3_lean over the other entries, in pipelined one-GPU frames on a stream of its
own (resumeSplit = 2).  Per entry the code is the unsplit kernel's, so every comparison here is
bit for bit: against the unsplit kernel (resumeSplit = 0), the CPU oracle and serial frames.
"""
import numpy as np
import pytest

from test_gpu_pathtrace import assert_gbuffers_equal, gpu_gbuffers, terrain_camera

pytestmark = pytest.mark.gpu

FRAME = 3
DT = 16.667


@pytest.fixture(scope="module")
def sky_tex(oracle):
    return oracle.sky(), oracle.textures()


def cameras(rtx, oracle, w, h, kind):
    if kind == "terrain":
        return terrain_camera(rtx, oracle, w, h)
    if kind == "sky":  # straight up from above the terrain: no camera ray hits, queue 3 stays empty
        return terrain_camera(rtx, oracle, w, h, pitch=1.5)
    return oracle.default_camera(w, h), None


def launch(rtx, tmp_path, name, w, h, spp, tuning, rcam=None, extra=""):
    """One detail launch of frame FRAME: G-buffers (with RAYS), counters, ray count, PT_STATS [P, 4]."""
    cfg = rtx.write_config(str(tmp_path / (name + ".toml")), w, h, spp=spp, extra=extra, tuning=tuning)
    rt = rtx.RayTracer(w, h, cfg).init()
    if rcam is not None:
        rt.camera = rcam
    rt.build_bvh()
    rt.path_trace(FRAME, detail=True)
    rt.sync()
    g = gpu_gbuffers(rt, w, h)
    q = rt.download("PT_QUEUE", np.uint32).copy()
    st = rt.download("PT_STATS", np.uint32).reshape(-1, 4)[:w * h].copy()
    rays = rt.ray_count()
    rt.cleanup()
    return g, q, rays, st


def trace(rtx, tmp_path, w, h, spp, split, rcam=None, extra=""):
    """... as four lean kernels (chain off): G-buffers, RAYS, counters."""
    return launch(rtx, tmp_path, "s%d" % split, w, h, spp, {"chain": "off", "resumeSplit": split}, rcam, extra)[:3]


@pytest.mark.parametrize("cam_kind", ["terrain", "default", "sky"])
@pytest.mark.parametrize("spp", [4, 1])
@pytest.mark.parametrize("w,h", [(100, 60), (192, 108)])
def test_split_matches_unsplit_and_oracle(rtx, oracle, tmp_path, default_scene, sky_tex, w, h, spp, cam_kind):
    ocam, rcam = cameras(rtx, oracle, w, h, cam_kind)
    ref, q0, rays0 = trace(rtx, tmp_path, w, h, spp, 0, rcam)
    assert q0[10] == 0  # kCntError
    assert q0[23] == 0  # no shading list without the split
    if cam_kind == "sky":
        assert q0[0] == 0  # queue 3 is empty
    elif cam_kind == "terrain":
        assert q0[0] > 256  # more than one workgroup's entries
    else:
        assert q0[0] > 0
    for split in (1, 2):
        g, q, rays = trace(rtx, tmp_path, w, h, spp, split, rcam)
        assert_gbuffers_equal(g, ref)
        assert rays == rays0
        assert q[10] == 0
        for k in (0, 1, 4, 11, 20, 21):  # queue lengths, pending and surface pixels, diffuse events
            assert q[k] == q0[k], k
        assert q[23] <= q[0]
        if (w, h) == (192, 108) and cam_kind == "terrain":
            s, tex = sky_tex
            o = oracle.pathtrace(default_scene["bvh"], w, h, frame_num=FRAME, spp=spp, cam=ocam, sky_out=s, tex=tex)
            assert_gbuffers_equal(g, o)
            assert rays == int(o["rays"].sum())


def test_shading_list_counts_the_d1_events(rtx, oracle, tmp_path):
    """Default materials: every triangle is Lambertian (update_material gives id 3, or 6 past the
    triangle count, both LAMBERTIAN in the reference table), so a listed entry (a bounce ray's
    triangle hit) is a D1 event and the reverse: the list's length equals resume<3>'s diffuse count."""
    w, h = 192, 108
    _, rcam = terrain_camera(rtx, oracle, w, h)
    for split in (1, 2):
        _, q, _ = trace(rtx, tmp_path, w, h, 4, split, rcam)
        assert q[21] > 0
        assert q[23] == q[21], (q[23], q[21])
        assert q[23] < q[0]  # shadow rays and misses are not listed


@pytest.mark.parametrize("w,h", [(192, 108), (100, 60)])  # 100x60: no multiple of the 64-lane batches
def test_chain_and_four_kernels_agree_on_detail_counts(rtx, oracle, tmp_path, w, h):
    """What a detail launch counts behind resume_entry — RAYS, PT_STATS, the ray total and the work
    counters — comes from one routine (finish_entry) in the fused chain, the unsplit resume<3> and the
    split one, so the three agree exactly.  The chain sums kCntDiffRes3 (counter 21) per wave like the
    kernels do.  Node visits and triangle tests (PT_STATS columns 1 and 2) are compared between the
    two four-kernel variants only: the chain's tracer loads its records differently and may count
    them differently."""
    _, rcam = terrain_camera(rtx, oracle, w, h)
    variants = [("chain", {"chain": "always"}), ("unsplit", {"chain": "off", "resumeSplit": 0}),
                ("split", {"chain": "off", "resumeSplit": 1})]
    (g0, q0, rays0, st0), unsplit, split = (launch(rtx, tmp_path, name, w, h, 4, tuning, rcam)
                                            for name, tuning in variants)
    assert q0[0] > 256  # more than one workgroup's entries
    assert q0[21] > 0 and st0[:, 3].sum() > 0
    for g, q, rays, st in (unsplit, split):
        assert_gbuffers_equal(g, g0)  # RAYS among them
        assert rays == rays0
        for col in (0, 3):  # rays, diffuse events per pixel
            assert np.array_equal(st[:, col], st0[:, col]), col
        for k in (0, 1, 4, 11, 20, 21):
            assert q[k] == q0[k], k
    for q in (q0, unsplit[1], split[1]):
        assert q[10] == 0  # kCntError
    assert np.array_equal(unsplit[3][:, 1:3], split[3][:, 1:3])
    assert np.array_equal(st0[:, 0], g0["rays"])  # the two per-pixel ray counts are one count
    assert rays0 == int(g0["rays"].sum())


def test_frame_tracers_dynamic_fetch_agrees_and_matches_oracle(rtx, oracle, tmp_path, default_scene, sky_tex):
    """The frame tracers' dynamic fetch.  At the other tests' sizes the static first batches
    (cus x tracePerCu x 256 entries) take all of queue 3; here one workgroup per CU ([tuning]
    tracePerCu = 1) leaves queue 3 longer than those batches plus one 64-entry reserve per fetch part,
    so k_trace_queue<3> (unsplit, and split with its shading list) and the chain's phase 1, which
    fetches every entry, run the refilling loop's top-ups, ragged part ends and tail.  The three agree
    on everything a detail launch counts, and with the CPU oracle bit for bit."""
    import torch

    w, h, spp = 320, 180, 4
    ocam, rcam = terrain_camera(rtx, oracle, w, h)
    variants = [("chain", {"chain": "always"}), ("unsplit", {"chain": "off", "resumeSplit": 0}),
                ("split", {"chain": "off", "resumeSplit": 1})]
    (g0, q0, rays0, st0), unsplit, split = (launch(rtx, tmp_path, name, w, h, spp, dict(tuning, tracePerCu=1), rcam)
                                            for name, tuning in variants)
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    print("queue 3: %d entries, %d CUs" % (q0[0], cus))
    assert q0[0] > cus * 256 + 8 * 64, (q0[0], cus)
    for g, q, rays, st in (unsplit, split):
        assert_gbuffers_equal(g, g0)  # RAYS among them
        assert rays == rays0
        for k in (0, 1, 4, 11, 20, 21):
            assert q[k] == q0[k], k
    for q in (q0, unsplit[1], split[1]):
        assert q[10] == 0  # kCntError
    s, tex = sky_tex
    o = oracle.pathtrace(default_scene["bvh"], w, h, frame_num=FRAME, spp=spp, cam=ocam, sky_out=s, tex=tex)
    assert_gbuffers_equal(g0, o)
    assert rays0 == int(o["rays"].sum())


def test_emissive_override_finishes_without_shading(rtx, oracle, tmp_path, default_scene, sky_tex):
    """materialOverride = 0 (emissive): no entry may shade.  The override covers every triangle, so a
    camera ray's hit already ends its path (hitLight) and nothing reaches queue 3: the shading list
    and both resume kernels run over empty ranges."""
    s, tex = sky_tex
    w, h = 100, 60
    ocam, rcam = terrain_camera(rtx, oracle, w, h)
    extra = "materialOverride = 0\n"
    ref, q0, _ = trace(rtx, tmp_path, w, h, 4, 0, rcam, extra)
    o = oracle.pathtrace(default_scene["bvh"], w, h, frame_num=FRAME, spp=4, cam=ocam, sky_out=s, tex=tex,
                         material_override=0)
    assert_gbuffers_equal(ref, o)
    for split in (1, 2):
        g, q, _ = trace(rtx, tmp_path, w, h, 4, split, rcam, extra)
        assert_gbuffers_equal(g, ref)
        assert_gbuffers_equal(g, o)
        assert q[10] == 0 and q[21] == 0  # no error, no D1 event
        assert q[23] == q0[0] == 0


def pipeline(rtx, tmp_path, pipelined, split, per_frame, frames=8, w=192, h=108):
    """`frames` frames through FramePipeline with the camera turning: every frame's RGBA8
    (per_frame: a host read per frame) and the final history."""
    import torch

    from rtx.frames import FramePipeline

    cfg = rtx.write_config(str(tmp_path / ("p%d%d%d.toml" % (pipelined, split, per_frame))), w, h, spp=4,
                           tuning={"resumeSplit": split})
    rt = rtx.RayTracer(w, h, cfg).init()
    rt.set_delta_time(DT)
    prev = torch.cuda.current_stream(0)
    fp = FramePipeline(rt, torch.device("cuda", 0), pipelined=pipelined)
    images = []
    try:
        cam0 = rt.camera
        for f in range(1, frames + 1):
            c = rt.camera
            c.yaw = cam0.yaw + 0.02 * f
            rt.camera = c
            fp.frame(f)
            if per_frame:
                images.append(rt.download("RGBA8", np.uint8).copy())
        fp.finish()
        out = dict(rgba=rt.download("RGBA8", np.uint8).copy(), hist=rt.get_buffer("HISTORY_COLOR").copy(),
                   acc=rt.get_buffer("ACCUMULATION").copy(), expo=rt.download("EXPOSURE", np.uint8).copy())
    finally:
        rt.cleanup()
        torch.cuda.set_stream(prev)
    return out, images


@pytest.fixture(scope="module")
def serial_frames(rtx, tmp_path_factory):
    return pipeline(rtx, tmp_path_factory.mktemp("serial"), False, 0, True)


def test_pipelined_forked_lean_pass_matches_serial(rtx, tmp_path, serial_frames):
    ref, ref_imgs = serial_frames
    got, _ = pipeline(rtx, tmp_path, True, 2, False)  # frames in flight: no host read between them
    for k in ref:
        assert np.array_equal(ref[k], got[k]), k
    got, imgs = pipeline(rtx, tmp_path, True, 2, True)
    assert len(imgs) == len(ref_imgs) == 8
    for f, (a, b) in enumerate(zip(ref_imgs, imgs)):
        assert np.array_equal(a, b), "frame %d" % (f + 1)
    for k in ref:
        assert np.array_equal(ref[k], got[k]), k


def test_two_strips_match_serial(rtx, tmp_path, serial_frames, monkeypatch):
    """Two strip ranks on one GPU (tests/test_gpu_multirank_pipeline.py's helper, whose configs take
    RTX_TUNING) with resumeSplit = 2: both ranks equal the one-rank pipelined run, which equals the
    serial frames."""
    from test_gpu_multirank_pipeline import run

    monkeypatch.setenv("RTX_TUNING", "resumeSplit=2")
    run(tmp_path, 2, (192, 108), 8, "rs", False)
    one = np.load(tmp_path / "rsr0_of1.npz")
    ref, _ = serial_frames
    for k in ("rgba", "hist", "acc", "expo"):
        assert np.array_equal(one[k], ref[k]), k
