"""bench.py --dump-outputs: the writer keeps every array float32/float64, all of them together under the
byte budget, and cuts a larger array to the same seeded sample on every call."""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def test_dump_writes_whole_arrays_within_the_budget(tmp_path):
    import bench
    assert bench.DUMP_BUDGET_BYTES <= 64 * 10 ** 6
    g = torch.Generator().manual_seed(0)
    arrays = {"loss": torch.rand((), generator=g), "params": torch.randn(1000, generator=g).to(torch.bfloat16),
              "grads": torch.randn(10, 7, generator=g, dtype=torch.float64)}
    info = bench._dump_outputs(str(tmp_path / "d"), arrays)
    assert sorted(os.listdir(tmp_path / "d")) == ["grads.npy", "loss.npy", "params.npy"]
    for name, t in arrays.items():
        a = np.load(tmp_path / "d" / f"{name}.npy")
        assert a.dtype == (np.float64 if t.dtype == torch.float64 else np.float32)
        assert info[name] == {"numel": t.numel(), "saved": t.numel()}
        assert np.array_equal(a, t.reshape(-1).to(torch.float64 if t.dtype == torch.float64 else torch.float32).numpy())


def test_dump_samples_a_large_array_the_same_way_every_time(tmp_path, monkeypatch):
    import bench
    monkeypatch.setattr(bench, "DUMP_BUDGET_BYTES", 4000)       # small whole (1200 bytes), 2800 left = 700 float32
    big = torch.arange(100_000, dtype=torch.float32)
    small = torch.arange(300, dtype=torch.float32)
    for d in ("a", "b"):
        info = bench._dump_outputs(str(tmp_path / d), {"big": big, "small": small})
        assert info == {"big": {"numel": 100_000, "saved": 700}, "small": {"numel": 300, "saved": 300}}
    a, b = np.load(tmp_path / "a" / "big.npy"), np.load(tmp_path / "b" / "big.npy")
    assert a.shape == (700,) and np.array_equal(a, b)
    assert np.all(np.diff(a) >= 0) and a.min() >= 0 and a.max() < 100_000     # values are their own indices
    assert len(np.unique(a)) > 400                                          # spread over the array, not one corner
    assert np.array_equal(np.load(tmp_path / "a" / "small.npy"), small.numpy())
    total = sum(os.path.getsize(tmp_path / "a" / f) for f in os.listdir(tmp_path / "a"))
    assert total <= 4000 + 2 * 128                                          # payload + the two .npy headers
