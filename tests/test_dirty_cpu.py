"""CPU: the allocation hook of tests/_dirty.py does what its docstring says, and its ``ENTRY_POINTS`` table covers every C
function of include/waveglow_amd.h that takes a ``workspace`` or a ``saved`` buffer."""
import os
import re
import struct

import numpy as np
import pytest
import torch

import _dirty as D

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))


def _as(pattern, fmt):
  """The bytes of ``pattern`` read as one value of the struct format ``fmt``."""
  return struct.unpack("<" + fmt, bytes([pattern]) * struct.calcsize(fmt))[0]


def test_the_patterns_read_as_stated():
  """A uint8 workspace of the pattern, seen through the types the kernels carve it into."""
  for fmt in "efd":
    assert _as(D.CLEAN, fmt) == 0.0
    assert np.isnan(_as(D.ONES, fmt))
  assert _as(D.CLEAN, "i") == 0 and _as(D.ONES, "i") == -1
  assert abs(_as(D.FINITE, "e") - 7.28) < 5e-3                  # fp16 0x4747
  assert abs(_as(D.FINITE, "f") - 51015.3) < 0.1                # fp32 0x47474747
  assert 2.3e35 < _as(D.FINITE, "d") < 2.5e35
  assert _as(D.FINITE, "i") == 0x47474747 > 1 << 30
  # the same through torch's own views of a filled byte buffer
  for p in D.PATTERNS:
    buf = torch.full((16,), p, dtype=torch.uint8)
    for dt, fmt in ((torch.float16, "e"), (torch.float32, "f"), (torch.float64, "d"), (torch.int32, "i")):
      want = _as(p, fmt)
      got = buf.view(dt)[0].item()
      assert (got != got and want != want) or got == want, (p, dt)


def test_poison_fills_by_type():
  """The dtype rules of ``_poison``.  There is no GPU here, so host tensors of a subclass that answers ``is_cuda`` with
  True stand in for GPU tensors."""

  class OnGpu(torch.Tensor):
    is_cuda = True

  def gpu(*shape, dtype):
    return torch.ones(*shape, dtype=dtype).as_subclass(OnGpu)

  for p in D.PATTERNS:
    assert D._poison(gpu(5, dtype=torch.uint8), p).tolist() == [p] * 5
    for dt in (torch.float16, torch.float32, torch.float64):
      t = D._poison(gpu(2, 3, dtype=dt), p)
      assert bool(torch.isnan(t).all()) if p != D.CLEAN else not t.any(), (p, dt)
    for dt in (torch.int16, torch.int32, torch.int64, torch.bool):
      assert D._poison(gpu(4, dtype=dt), p).tolist() == gpu(4, dtype=dt).tolist(), (p, dt)
  # a host tensor of any type is left alone
  for dt in (torch.uint8, torch.float32, torch.int32):
    t = torch.zeros(4, dtype=dt).add_(3)
    assert D._poison(t, D.ONES).tolist() == [3] * 4


def test_the_hook_restores_torch_empty_and_leaves_host_tensors_alone(monkeypatch):
  empty, empty_like = torch.empty, torch.empty_like
  seen = []
  for p in D.PATTERNS:
    with D.poisoned_allocations(monkeypatch, p):
      assert torch.empty is not empty and torch.empty_like is not empty_like
      a = torch.empty(7, dtype=torch.uint8)
      b = torch.empty((2, 3), dtype=torch.float32)
      c = torch.empty_like(torch.arange(6, dtype=torch.int32))
      d = torch.empty(3, dtype=torch.float64, pin_memory=False)
      assert a.shape == (7,) and a.dtype == torch.uint8 and b.shape == (2, 3) and c.dtype == torch.int32 and d.dtype == torch.float64
      seen.append(p)
    assert torch.empty is empty and torch.empty_like is empty_like
  assert seen == list(D.PATTERNS)
  with pytest.raises(RuntimeError):
    with D.poisoned_allocations(monkeypatch, D.ONES):
      raise RuntimeError("a failing test body")
  assert torch.empty is empty and torch.empty_like is empty_like


def test_same_bytes_tells_nan_payloads_and_signed_zeros():
  nan = torch.tensor([float("nan"), 1.0])
  D.same_bytes(nan, nan.clone(), "equal NaNs")
  with pytest.raises(AssertionError, match="1 of 2 entries differ"):
    D.same_bytes(torch.tensor([0.0, 1.0]), torch.tensor([-0.0, 1.0]), "signed zero")
  with pytest.raises(AssertionError):
    D.same_bytes(torch.zeros(2), torch.zeros(2, dtype=torch.float64), "dtype")
  with pytest.raises(AssertionError, match="q"):
    D.same_outputs({"q": torch.zeros(3)}, {"q": torch.ones(3)}, "outputs")


def workspace_entry_points():
  """Every prototype of the header with a ``void* workspace`` or ``void* saved`` parameter (const or not)."""
  text = open(os.path.join(ROOT, "include", "waveglow_amd.h")).read()
  text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
  out = set()
  for name, args in re.findall(r"\b(wg_[a-z0-9_]+)\s*\(([^;{}]*?)\)\s*;", text, flags=re.S):
    if re.search(r"\bvoid\s*\*\s*(workspace|saved)\b", args):
      out.add(name)
  return out


def test_every_entry_point_with_a_workspace_is_in_the_table():
  found = workspace_entry_points()
  # 34 before the twelve _ragged / _saved twins were folded into their dense calls
  assert len(found) == 34 - 12 and {"wg_infer", "wg_stoi_backward", "wg_train_infer_backward", "wg_loss"} <= found
  assert "wg_metrics_dtw" not in found and "wg_resample" not in found            # no workspace: outputs only
  assert found == set(D.ENTRY_POINTS), sorted(found ^ set(D.ENTRY_POINTS))
  # every test the table names exists
  for fn, tests in D.ENTRY_POINTS.items():
    assert tests, fn
    for t in tests:
      path, name = t.split("::")
      src = open(os.path.join(ROOT, path)).read()
      assert re.search(rf"^def {name}\(", src, flags=re.M), f"{fn}: {t} does not exist"
      assert "pytestmark = pytest.mark.gpu" in src, path
