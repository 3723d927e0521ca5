"""The denoise launcher's kernel variants that the default settings never reach, bit for bit
against the oracle.

The host picks a kernel instantiation per pass from run-time settings: the depth weights' divisor
as a reciprocal (kRcp: sigma_depth within 2^-20..2^20), the paired normal weights (kPk:
sigma_normal finite and > 0), the active-tile lists at one or two threads per pixel ([tuning]
dnSplit), the folded chain ([tuning] dnFold), and the frame-wide kernels when a pass is off.
Three frames at 128x72: frame 1 takes the non-temporal path, frames 2 and 3 the list chain on
both tile-list parities.
"""
import numpy as np
import pytest

from test_gpu_denoise import run_sequence

pytestmark = pytest.mark.gpu

W, H, FRAMES = 128, 72, 3
FILTERS = ("temporal", "local", "large")
SIGMAS = {"pk-off": dict(sigma_normal=0.0), "rcp-off": dict(sigma_depth=float(2 ** 21)),
          "pk-rcp-off": dict(sigma_normal=0.0, sigma_depth=float(2 ** 21))}
TUNINGS = {"default": "", "fold": "\n[tuning]\ndnFold = 1\n", "split": "\n[tuning]\ndnSplit = 2\n"}


def tweak(sigmas=None, **passes):
    """params_fn of run_sequence: the sigmas on all three filters, the pass switches by name."""
    def fn(p, op):
        for k, v in (sigmas or {}).items():
            for f in FILTERS:
                setattr(p.denoise, "%s_denoise_%s" % (f, k), v)
                setattr(op, "%s_denoise_%s" % (f, k), v)
        for k, v in passes.items():
            setattr(p.pass_, k, v)
            setattr(op, k, v)
    return fn


class RecordingOracle:
    """The oracle with its path-traced G-buffers shared between the cases (they do not depend on
    the denoise settings) and every Denoiser.draw result kept for the case's own conditions."""
    gbuffers = {}

    def __init__(self, oracle):
        self._o = oracle
        self.draws = []

    def __getattr__(self, k):
        return getattr(self._o, k)

    def pathtrace(self, bvh, w, h, frame_num, spp, **kw):
        key = (w, h, frame_num, spp)
        if key not in self.gbuffers:
            g = self._o.pathtrace(bvh, w, h, frame_num=frame_num, spp=spp, **kw)
            for a in g.values():
                a.setflags(write=False)
            self.gbuffers[key] = g
        return self.gbuffers[key]

    def Denoiser(self, *a, **kw):
        dn = self._o.Denoiser(*a, **kw)
        draw = dn.draw

        def recorded(*a, **kw):
            o = draw(*a, **kw)
            self.draws.append(o)
            return o
        dn.draw = recorded
        return dn


def assert_both_tile_kinds(rec, op):
    """Frames 2 and 3 put tiles on the lists and leave tiles off them, for both thresholds."""
    assert len(rec.draws) == FRAMES
    for f in (2, 3):
        n16 = rec.draws[f - 1]["noise16"].view(np.float16).astype(np.float32)
        for thr in (op.noise_threshold_large, op.noise_threshold_local):
            assert (n16 >= thr).any() and (n16 < thr).any(), (f, thr, n16)


def run(rtx, oracle, tmp_path, default_scene, params_fn, extra=""):
    rec = RecordingOracle(oracle)
    run_sequence(rtx, rec, tmp_path, default_scene, W, H, FRAMES, extra=extra, params_fn=params_fn)
    return rec


@pytest.mark.parametrize("tuning", list(TUNINGS))
@pytest.mark.parametrize("sigma", list(SIGMAS))
def test_list_chain_sigma_variants(rtx, oracle, tmp_path, default_scene, sigma, tuning):
    """kPk / kRcp off in the list chain: k_temporal<1,1,r,p>, k_spatial7_list[2]<r,p>,
    k_spatial5_list[2]<3|6|12,r,..,p,..> with the kCopy first pass and the albedo-folding last pass
    (fold, split), or the redirecting k_spatial5<12,1,r,1,p> (default)."""
    fn = tweak(SIGMAS[sigma])
    rec = run(rtx, oracle, tmp_path, default_scene, fn, TUNINGS[tuning])
    op = oracle.default_params()
    fn(rtx.Params(), op)
    assert_both_tile_kinds(rec, op)


@pytest.mark.parametrize("sigma", ["default", "rcp-off"])
@pytest.mark.parametrize("off", ["enableWideSpatialFilter", "enableLocalSpatialFilter", "enableTemporalDenoising"])
def test_frame_wide_paths(rtx, oracle, tmp_path, default_scene, off, sigma):
    """One of the three filters off, so the lists are not used: no wide filter runs
    k_temporal<1,0,r>, k_spatial7<0,r> and k_apply_albedo; no local filter k_temporal<0,0,r>, the
    stand-alone noise kernels and the frame-wide k_spatial5<3|6|12>; no temporal filter
    k_spatial7<1,r> and the frame-wide k_spatial5."""
    run(rtx, oracle, tmp_path, default_scene, tweak(SIGMAS.get(sigma), **{off: 0}))


@pytest.mark.parametrize("off", ["enableTemporalDenoising2", "enableDownScalePasses"])
def test_tail_paths(rtx, oracle, tmp_path, default_scene, off):
    """The tail without TemporalFilter2 (k_downscale_chain<false>, the history-depth copy) and
    without the downscale passes (the histogram of the levels as they are).  Without the histogram
    (three k_downscale4 launches and the cleared histogram) AutoExposure divides 0 by 0: every image
    matches, but the NaN it stores has its sign clear on the GPU and set in the oracle, so that case
    is not here."""
    run(rtx, oracle, tmp_path, default_scene, tweak(**{off: 0}))
