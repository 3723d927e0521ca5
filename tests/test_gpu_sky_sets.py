"""Sky sets on the GPU ([scene] skySets): a sky change or a device environment
before every pipelined frame, with no host wait in the loop, against the same script on a serial
context with one set, and against the oracle; the launches ahead of synchronous draws across a sky
change.  With 2 sets frame f + 2 recycles frame f's set while f + 1 is in flight; 4 is the probe's
count.  Frames are 96 x 54 on the default terrain; every comparison is bit-exact."""
import numpy as np
import pytest

from test_gpu_pathtrace import terrain_camera

pytestmark = pytest.mark.gpu

W, H, SPP, FRAMES = 96, 54, 2, 6
DT = 16.667
ORACLE_FRAMES = (3, 6)  # with two sets, frame 3 is the first on a recycled set


def time_of_day(f):
    return float(np.float32(0.25 + 0.015 * f))


def env_image(f):
    """Frame f's environment: a 64 x 32 half LATLONG image, different for every frame."""
    rng = np.random.default_rng(100 + f)
    img = (rng.random((32, 64, 4)) * (0.5 + f)).astype(np.float16)
    img[3, 5 * f, :3] = 900.0  # one bright texel that moves
    return img


ENV_SCALE = 1.25


def make(rtx, oracle, tmp_path, name, sky_sets, tuning=None):
    cfg = rtx.write_config(str(tmp_path / (name + ".toml")), W, H, spp=SPP, sky_sets=sky_sets, tuning=tuning or {})
    rt = rtx.RayTracer(W, H, cfg).init()
    rt.set_delta_time(DT)
    ocam, rcam = terrain_camera(rtx, oracle, W, H)
    rt.camera = rcam
    return rt, ocam


def set_time(rt, f):
    p = rt.params
    p.sky.timeOfDay = time_of_day(f)
    rt.params = p


def end_state(rt):
    out = dict(SKY=rt.get_buffer("SKY").copy(), SUN=rt.get_buffer("SUN").copy(), SKY_CDF=rt.download("SKY_CDF").copy(),
               RENDER_COLOR=rt.get_buffer("RENDER_COLOR").copy(), ACCUMULATION=rt.get_buffer("ACCUMULATION").copy(),
               HISTORY_COLOR=rt.get_buffer("HISTORY_COLOR").copy(), EXPOSURE=rt.download("EXPOSURE").copy())
    assert rt.download("PT_QUEUE", np.uint32)[10] == 0
    return out


def serial(rtx, oracle, tmp_path, env):
    """The script on a serial context with one sky set: the RGBA8 image of every frame and the end state."""
    rt, _ = make(rtx, oracle, tmp_path, "serial%d" % env, None)
    assert rt.sky_sets == 1
    frames = []
    for f in range(1, FRAMES + 1):
        if env:
            rt.set_environment(env_image(f), rtx.ENV_LAYOUT_LATLONG, ENV_SCALE)
        else:
            set_time(rt, f)
        rt.build_bvh()
        rt.path_trace(f)
        rt.denoise_post(f)
        frames.append(rt.download("RGBA8", np.uint8).copy())
        assert rt.download("PT_QUEUE", np.uint32)[10] == 0
    state = end_state(rt)
    rt.cleanup()
    return frames, state


@pytest.fixture(scope="module")
def serial_runs(rtx, oracle, tmp_path_factory):
    d = tmp_path_factory.mktemp("serial")
    return {env: serial(rtx, oracle, d, env) for env in (False, True)}


@pytest.fixture(scope="module")
def oracle_frames(rtx, oracle, default_scene):
    """The oracle's RGBA8 of ORACLE_FRAMES for both scripts (its denoiser runs every frame up to them)."""
    tex = oracle.textures()
    ocam = terrain_camera(rtx, oracle, W, H)[0]
    out = {}
    for env in (False, True):
        dn = oracle.Denoiser(W, H)
        base = oracle.sky()
        for f in range(1, FRAMES + 1):
            if env:
                table, pdf = rtx.environment_table(env_image(f), rtx.ENV_LAYOUT_LATLONG, ENV_SCALE)
                s = dict(base, sky=table, sky_cdf=oracle.scan(pdf.reshape(-1), 256))
            else:
                s = oracle.sky(dict(timeOfDay=time_of_day(f)))
            gb = oracle.pathtrace(default_scene["bvh"], W, H, frame_num=f, spp=SPP, cam=ocam, hist_cam=ocam, sky_out=s, tex=tex)
            o = dn.draw(gb, f, delta_time=DT)
            if f in ORACLE_FRAMES:
                out[env, f] = o["rgba"].copy()
            if f == FRAMES:
                out[env, "sky"] = np.ascontiguousarray(s["sky"], np.float32).copy()
    return out


def pipelined(rtx, oracle, tmp_path, sky_sets, env):
    """The script on a pipelined context (rtx.frames.FramePipeline) with no wait in the loop.  The RGBA8
    buffer is a tensor of the test's (rt_bind_buffer, ahead of the loop); frame f's image is copied out of
    it on the post stream once frame f + 1 is enqueued, which is when frame f's deferred denoise has
    been, and ahead of frame f + 1's."""
    import torch

    from rtx.frames import FramePipeline

    rt, _ = make(rtx, oracle, tmp_path, "pipe%d_%d" % (sky_sets, env), sky_sets)
    assert rt.sky_sets == sky_sets
    dev = torch.device("cuda", 0)
    prev = torch.cuda.current_stream(0)
    rgba = torch.zeros(W * H, dtype=torch.int32, device=dev)
    snaps = [torch.zeros_like(rgba) for _ in range(FRAMES)]
    images = torch.stack([torch.from_numpy(env_image(f)) for f in range(1, FRAMES + 1)]).to(dev)
    src = torch.zeros_like(images[0])
    producer = torch.cuda.Stream(dev)
    torch.cuda.synchronize()
    rt.bind_buffer("RGBA8", rgba.data_ptr(), W * H * 4)
    pipe = FramePipeline(rt, dev, pipelined=True)
    try:
        for f in range(1, FRAMES + 1):
            if env:
                producer.wait_stream(torch.cuda.current_stream(dev))  # behind the last overwrite of src
                with torch.cuda.stream(producer):
                    src.copy_(images[f - 1])
                    ready = torch.cuda.Event()
                    ready.record(producer)
                rt.set_environment_device(src, 64, 32, rtx.ENV_FORMAT_F16X4, rtx.ENV_LAYOUT_LATLONG, ENV_SCALE,
                                          ready_event=ready.cuda_event)
                src.fill_(7.0)  # on the context stream, right after the call: it follows the read
            else:
                set_time(rt, f)
            pipe.frame(f)
            if f > 1:
                with torch.cuda.stream(pipe.post):
                    snaps[f - 2].copy_(rgba)
        pipe.finish()
        snaps[FRAMES - 1].copy_(rgba)
        torch.cuda.synchronize()
        frames = [s.cpu().numpy().view(np.uint8) for s in snaps]
        state = end_state(rt)
    finally:
        torch.cuda.set_stream(prev)
        rt.cleanup()
    return frames, state


@pytest.mark.parametrize("env", [False, True], ids=["timeOfDay", "device-environment"])
@pytest.mark.parametrize("sky_sets", [2, 4])
def test_pipelined_sky_changes_match_serial_and_oracle(rtx, oracle, tmp_path, serial_runs, oracle_frames, sky_sets, env):
    want_frames, want_state = serial_runs[env]
    frames, state = pipelined(rtx, oracle, tmp_path, sky_sets, env)
    for f, (a, b) in enumerate(zip(frames, want_frames), start=1):
        assert np.array_equal(a, b), "frame %d against the serial context" % f
    for f in ORACLE_FRAMES:
        assert np.array_equal(frames[f - 1].reshape(-1, 4), oracle_frames[env, f]), "frame %d against the oracle" % f
    for k in want_state:  # RT_BUF_SKY after the loop is the last set's
        assert np.array_equal(state[k], want_state[k]), k
    assert np.array_equal(state["SKY"].view(np.uint32), oracle_frames[env, "sky"].reshape(-1).view(np.uint32))


def test_serial_frames_differ(serial_runs):
    """The scripts do change the image from frame to frame (the comparisons above are not of one picture)."""
    for env in (False, True):
        frames = serial_runs[env][0]
        assert all(not np.array_equal(a, b) for a, b in zip(frames, frames[1:]))


def test_synchronous_draws_across_a_sky_change(rtx, oracle, tmp_path):
    """Draws that launch ahead on a two-set context: no change is a reuse; a sky change, and a device
    environment, each raise SPEC_STATS[2] by one, and every frame is what [tuning] syncSpec = false renders."""
    import torch

    d_img = torch.from_numpy(env_image(1)).cuda()
    torch.cuda.synchronize()

    def run(name, tuning):
        rt, _ = make(rtx, oracle, tmp_path, name, 2, tuning)
        frames, stats = [], []
        for k in range(7):
            if k in (2, 5):
                set_time(rt, k)
            if k == 4:
                rt.set_environment_device(d_img, 64, 32, rtx.ENV_FORMAT_F16X4, rtx.ENV_LAYOUT_LATLONG, ENV_SCALE)
            hdr = np.zeros((H, W, 4), np.float32)
            rt.draw(None, hdr)  # keeps what it launched ahead alive
            frames.append(hdr.view(np.uint32))
            stats.append(rt.download("SPEC_STATS", np.uint32).tolist())
        errors = int(rt.download("PT_QUEUE", np.uint32)[10])
        rt.cleanup()
        assert errors == 0
        return frames, stats

    on, stats = run("on", {"syncSpec": True})
    off, off_stats = run("off", {"syncSpec": False})
    assert off_stats[-1][:3] == [0, 0, 0]
    for k, (a, b) in enumerate(zip(on, off)):
        assert np.array_equal(a, b), "draw %d" % k
    launched = [s[0] for s in stats]
    reused = [s[1] for s in stats]
    dropped = [s[2] for s in stats]
    assert launched == [1, 2, 3, 4, 5, 6, 7]
    # draw k uses or drops what draw k - 1 launched: changes before draws 2, 4 and 5
    assert dropped == [0, 0, 1, 1, 2, 3, 3]
    assert reused == [0, 1, 1, 2, 2, 2, 3]


def test_device_variant_needs_two_sets(rtx, oracle, tmp_path):
    import torch

    rt, _ = make(rtx, oracle, tmp_path, "one", None)
    d_img = torch.from_numpy(env_image(1)).cuda()
    torch.cuda.synchronize()
    rt.build_bvh()
    rt.path_trace(1)
    before = rt.get_buffer("SKY").copy()
    with pytest.raises(rtx.RtError, match="rt_set_environment_device: RT_ERR_STATE"):
        rt.set_environment_device(d_img, 64, 32, rtx.ENV_FORMAT_F16X4, rtx.ENV_LAYOUT_LATLONG, ENV_SCALE)
    assert not rt.environment_active and np.array_equal(rt.get_buffer("SKY"), before)
    rt.cleanup()
