"""bench.py's CPU-baseline legs on a small size (no GPU): BASELINE config 1's host frame and the
thread-count rule the JSON reports."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import bench  # noqa: E402


def test_c1_frame_small(oracle):
    r = bench.c1_frame(oracle, threads=2, size=64)
    assert r["size"] == [64, 64] and r["spp"] == 1
    assert r["rays"] >= 64 * 64  # every pixel traces its camera ray
    for k in ("lbvh_build_ms", "path_trace_ms", "denoise_post_ms", "hdr_dump_ms"):
        assert r[k] > 0.0
    assert abs(r["frame_ms"] - (r["lbvh_build_ms"] + r["path_trace_ms"] + r["denoise_post_ms"] + r["hdr_dump_ms"])) < 1.0


def test_host_threads_respects_cap(monkeypatch):
    monkeypatch.setenv("OMP_NUM_THREADS", "3")
    assert 1 <= bench.host_threads() <= 3
    monkeypatch.delenv("OMP_NUM_THREADS")
    assert bench.host_threads() >= 1


def test_dump_outputs_sample_is_fixed_and_bounded(tmp_path):
    """--dump-outputs: float32 files; a frame above the budget is cut to the same pixels every time."""
    import numpy as np

    w, h = 2560, 1440  # 3.7 M pixels: above each array's share of the budget
    rng = np.random.default_rng(7)
    final = dict(rgba=rng.integers(0, 256, w * h * 4, dtype=np.uint8),
                 color=rng.random(w * h * 4, dtype=np.float32).astype(np.float16).view(np.uint8),
                 exposure=np.array([1.5, 0.25, 3.0, 0.125], np.float32).view(np.uint8))
    bench.dump_outputs(str(tmp_path / "a"), final)
    bench.dump_outputs(str(tmp_path / "b"), final)
    total = 0
    for name in ("rgba8", "hdr", "exposure"):
        a, b = np.load(tmp_path / "a" / (name + ".npy")), np.load(tmp_path / "b" / (name + ".npy"))
        assert a.dtype == np.float32 and np.array_equal(a, b)
        total += os.path.getsize(tmp_path / "a" / (name + ".npy"))
    assert total <= 64 * 10 ** 6
    keep = len(np.load(tmp_path / "a" / "rgba8.npy"))
    assert keep < w * h and np.load(tmp_path / "a" / "hdr.npy").shape == (keep, 4)
    assert np.load(tmp_path / "a" / "exposure.npy").tolist() == [1.5, 0.25, 3.0, 0.125]
    # a frame within the budget is written whole, and widening half to float32 is exact
    small = dict(rgba=final["rgba"][:64 * 4], color=final["color"][:64 * 8], exposure=final["exposure"])
    bench.dump_outputs(str(tmp_path / "c"), small)
    assert np.array_equal(np.load(tmp_path / "c" / "rgba8.npy"), small["rgba"].reshape(64, 4))
    assert np.array_equal(np.load(tmp_path / "c" / "hdr.npy").astype(np.float16).view(np.uint8).ravel(), small["color"])
