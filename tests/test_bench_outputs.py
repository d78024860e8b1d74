"""bench.py --dump-outputs: the files a run leaves for comparing two builds (CPU only)."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
import bench  # noqa: E402


def _dump(tmp_path, name, frame, rays):
    d = str(tmp_path / name)
    bench.dump_outputs(d, frame, rays)
    assert sorted(os.listdir(d)) == ["framebuffer.npy", "segments.npy"]
    return np.load(os.path.join(d, "framebuffer.npy")), np.load(os.path.join(d, "segments.npy"))


def test_small_frame_is_dumped_whole(tmp_path):
    frame = np.arange(7 * 5 * 3, dtype=np.float64).reshape(-1, 3)
    fb, segs = _dump(tmp_path, "a", frame, 12345.0)
    assert fb.dtype == np.float64 and np.array_equal(fb, frame)
    assert segs.dtype == np.float64 and segs.tolist() == [12345.0]


def test_large_frame_is_a_fixed_sample_within_the_size_limit(tmp_path, monkeypatch):
    monkeypatch.setattr(bench, "DUMP_MAX_BYTES", 4096 + 24 * 1000)  # room for 1000 pixels
    frame = np.repeat(np.arange(5000, dtype=np.float64), 3).reshape(-1, 3)
    fb, _ = _dump(tmp_path, "a", frame, 1.0)
    fb2, _ = _dump(tmp_path, "b", frame, 1.0)
    assert fb.shape == (1000, 3) and np.array_equal(fb, fb2)
    idx = fb[:, 0].astype(np.int64)
    assert np.all(np.diff(idx) > 0) and np.array_equal(fb, frame[idx])  # distinct pixels, in index order
    total = sum(os.path.getsize(os.path.join(str(tmp_path / "a"), f)) for f in ("framebuffer.npy", "segments.npy"))
    assert total <= bench.DUMP_MAX_BYTES
