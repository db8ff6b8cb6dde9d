"""bench.py's host side: the --dump-outputs writer."""
import os

import numpy as np
import torch

import bench


def test_dump_outputs_writes_float32_and_keeps_small_outputs_whole(tmp_path):
  audio = torch.randn(3, 1000, dtype=torch.float16)
  bench.dump_outputs(str(tmp_path), {"audio": audio, "loss": torch.tensor([1.5], dtype=torch.float64)})
  a = np.load(tmp_path / "audio.npy")
  assert a.dtype == np.float32 and a.shape == (3, 1000) and np.array_equal(a, audio.float().numpy())
  loss = np.load(tmp_path / "loss.npy")
  assert loss.dtype == np.float64 and loss.tolist() == [1.5]


def test_dump_outputs_samples_large_outputs_within_budget_and_reproducibly(tmp_path, monkeypatch):
  monkeypatch.setattr(bench, "DUMP_BUDGET_BYTES", 2 << 20)
  big = torch.arange(3_000_000, dtype=torch.float32)
  for d in ("a", "b"):
    bench.dump_outputs(str(tmp_path / d), {"x": big, "y": big[:10]})
  total = sum(os.path.getsize(tmp_path / "a" / n) for n in os.listdir(tmp_path / "a"))
  assert total <= 2 << 20, total
  x = np.load(tmp_path / "a" / "x.npy")
  assert x.dtype == np.float32 and x.ndim == 1 and 100_000 < x.size < 3_000_000
  assert np.all(np.diff(x) >= 0) and np.all(x == np.round(x))      # sorted positions of the flattened tensor
  assert np.array_equal(x, np.load(tmp_path / "b" / "x.npy"))        # same sample in every run
  assert np.load(tmp_path / "a" / "y.npy").tolist() == list(range(10))
