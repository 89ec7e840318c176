"""CPU: bench.py --dump-outputs (bench.dump_outputs) -- float32 .npy files, the 64 MB cap, a sample that is the same on every run."""
import os

import numpy as np
import torch

import bench


def test_dump_outputs_writes_small_arrays_whole(tmp_path):
    x = torch.randn(2, 4, 3, 5, 7, dtype=torch.float64)
    info = bench.dump_outputs(str(tmp_path), {"latents": x})
    got = np.load(tmp_path / "latents.npy")
    assert got.dtype == np.float32 and got.shape == tuple(x.shape)
    assert np.array_equal(got, x.float().numpy())
    assert info == {"latents": {"shape": list(x.shape), "saved": x.numel()}}


def test_dump_outputs_caps_the_total_with_a_fixed_sample(tmp_path):
    cap = 1 << 20
    arrays = {"a": torch.arange(300_000, dtype=torch.float32), "b": -torch.arange(200_000, dtype=torch.float32).reshape(400, 500)}
    info = bench.dump_outputs(str(tmp_path / "r1"), arrays, max_bytes=cap)
    bench.dump_outputs(str(tmp_path / "r2"), arrays, max_bytes=cap)
    assert sum(os.path.getsize(tmp_path / "r1" / f"{k}.npy") for k in arrays) <= cap
    assert info["b"]["shape"] == [400, 500] and 0 < info["b"]["saved"] < info["a"]["saved"] < 300_000
    for k in arrays:
        s1, s2 = np.load(tmp_path / "r1" / f"{k}.npy"), np.load(tmp_path / "r2" / f"{k}.npy")
        assert s1.dtype == np.float32 and np.array_equal(s1, s2)               # same positions on every run
        assert np.isin(s1, arrays[k].numpy()).all() and np.unique(s1).size == s1.size
