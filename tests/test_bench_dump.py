"""bench.py --dump-outputs (host side): what ``dump_outputs`` writes for a small output and for one
over the 64 MB limit (a fixed seeded sample with its indices)."""

import sys
from pathlib import Path

import numpy as np
import torch

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))

import bench  # noqa: E402


def test_small_output_is_written_whole(tmp_path):
    t = torch.arange(3 * 50, dtype=torch.float32).reshape(3, 50)
    bench.dump_outputs(tmp_path, t, 0)
    assert sorted(f.name for f in tmp_path.iterdir()) == ["color.npy"]
    got = np.load(tmp_path / "color.npy")
    assert got.dtype == np.float32 and np.array_equal(got, t.numpy())
    # float64 stays float64; uint8 frames are written as float32; other ranks write their own file
    bench.dump_outputs(tmp_path, t.double(), 1)
    assert np.load(tmp_path / "color_rank1.npy").dtype == np.float64
    u8 = torch.arange(24, dtype=torch.uint8).reshape(2, 4, 3)
    bench.dump_outputs(tmp_path / "u8", u8, 0)
    got = np.load(tmp_path / "u8" / "color.npy")
    assert got.dtype == np.float32 and np.array_equal(got, u8.numpy().astype(np.float32))
    bench.dump_outputs(tmp_path / "none", None, 1)  # a tiles-mode peer has no frame
    assert not (tmp_path / "none").exists()


def test_large_output_is_a_fixed_sample_within_the_limit(tmp_path):
    n = bench.DUMP_MAX_BYTES // 4 + 1000  # just over the limit as float32
    t = torch.arange(n, dtype=torch.int32).to(torch.float32).reshape(2, -1)
    bench.dump_outputs(tmp_path / "a", t, 0)
    bench.dump_outputs(tmp_path / "b", t, 0)
    files = sorted((tmp_path / "a").iterdir())
    assert [f.name for f in files] == ["color.npy", "color_index.npy"]
    assert sum(f.stat().st_size for f in files) <= bench.DUMP_MAX_BYTES
    idx = np.load(tmp_path / "a" / "color_index.npy")
    val = np.load(tmp_path / "a" / "color.npy")
    assert val.dtype == np.float32 and val.shape == idx.shape and len(idx) > 1_000_000
    assert np.all(np.diff(idx) > 0) and idx[0] >= 0 and idx[-1] < n
    assert np.array_equal(val, t.reshape(-1).numpy()[idx])
    assert np.array_equal(idx, np.load(tmp_path / "b" / "color_index.npy"))
    assert np.array_equal(val, np.load(tmp_path / "b" / "color.npy"))
