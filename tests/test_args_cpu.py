"""CPU: ``waveglow_amd._args``, the one place that decides how per-utterance counts are accepted, what a tensor argument
must be and who releases a library handle.  ``counts`` runs with ``device="cpu"`` here: it must not care."""
import ctypes as C

import numpy as np
import pytest
import torch

from waveglow_amd import _args
from waveglow_amd._lib import WgError

NAME = "entry: lengths"

# (lo, hi, multiple_of) of every call site, at small sizes: N = 4096 samples, T = 12 frames
RANGES = {
  "stft loss (need 1024)": (1025, 4096, 1),
  "mel front-end": (513, 4096, 1),
  "denoiser": (1024, 4096, 256),
  "resample / STOI loss / metrics lengths": (0, 4096, 1),
  "metrics frames / soft-DTW": (1, 12, 1),
  "likelihood": (1, min(12, 4096 // 256), 1),
  "infer_differentiable": (1, 12, 1),
}


@pytest.mark.parametrize("values", [
  [5, 7], (5, 7), range(5, 9, 2), [np.int32(5), np.int32(7)], [np.int64(5), 7],
  torch.tensor([5, 7], dtype=torch.int16), torch.tensor([5, 7], dtype=torch.int32), torch.tensor([5, 7]),
], ids=lambda v: f"{type(v).__name__}-{getattr(v, 'dtype', type(v[0]).__name__)}")
def test_counts_accepted_forms(values):
  dev, host = _args.counts(NAME, values, 2, 0, 10, device="cpu")
  assert host == [5, 7] and all(type(n) is int for n in host)
  assert dev.dtype == torch.int32 and dev.shape == (2,) and dev.is_contiguous() and dev.device.type == "cpu"
  assert dev.tolist() == [5, 7]


@pytest.mark.parametrize("values,word", [
  ([True, 7], "True"), ([3.0, 7], "3.0"), ([5, 7.5], "7.5"), ([5, 7 + 0j], "7"), ([5, "7"], "'7'"), ([5, None], "None"),
  (torch.tensor([5.0, 7.0]), "float32"), (torch.tensor([5, 7], dtype=torch.float16), "float16"),
  (torch.tensor([True, False]), "bool"), (torch.tensor([5, 7], dtype=torch.complex64), "complex64"),
  (torch.tensor([[5, 7]]), "(1, 2)"), (torch.tensor(5), "()"), ("57", "str"), (5, "int"), (None, "NoneType"),
  ({5, 7}, "set"), (np.array([5, 7]), "ndarray"),
  ([5], "1 lengths for a batch of 2"), ([5, 7, 9], "3 lengths for a batch of 2"), (torch.tensor([5]), "1 lengths"),
], ids=lambda v: None if isinstance(v, str) else repr(v).replace("\n", ""))
def test_counts_refused_forms(values, word):
  with pytest.raises(WgError) as e:
    _args.counts(NAME, values, 2, 0, 10, device="cpu")
  assert str(e.value).startswith(NAME) and word in str(e.value), str(e.value)


@pytest.mark.parametrize("site", sorted(RANGES))
def test_counts_boundaries(site):
  lo, hi, step = RANGES[site]
  assert _args.counts(NAME, [lo, hi], 2, lo, hi, device="cpu", multiple_of=step)[1] == [lo, hi]
  for bad in (lo - 1, hi + 1):
    with pytest.raises(WgError) as e:
      _args.counts(NAME, [lo, bad], 2, lo, hi, device="cpu", multiple_of=step)
    msg = str(e.value)
    assert msg.startswith(f"{NAME}[1] = {bad} ") and f"[{lo}, {hi}]" in msg, msg
  if step != 1:
    with pytest.raises(WgError, match=f"multiples of {step}"):
      _args.counts(NAME, [lo, lo + step // 2], 2, lo, hi, device="cpu", multiple_of=step)      # 1024 + 128
    assert _args.counts(NAME, [lo, lo + step], 2, lo, hi, device="cpu", multiple_of=step)[1] == [lo, lo + step]


class OnGpu(torch.Tensor):
  """A host tensor that says it is on a GPU: what the checks see, with no device behind it."""
  device = torch.device("cuda:0")


def _gpu(data, dtype):
  return torch.tensor(data, dtype=dtype).as_subclass(OnGpu)


def test_counts_device_form_needs_permission_and_is_trusted():
  """A tensor that is not on the host is refused unless the call site allows it; allowed, it must be int32 [B] on the
  call's device and comes back as it is, with no host list and its values unchecked (99 and -5 are outside [0, 10])."""
  t = _gpu([99, -5], torch.int32)
  for device in ("cuda:0", None):                                  # None: the check alone, nothing uploaded
    with pytest.raises(WgError, match="host integers"):
      _args.counts(NAME, t, 2, 0, 10, device=device)
  assert _args.counts(NAME, [5, 7], 2, 0, 10, device=None) == (None, [5, 7])
  dev, host = _args.counts(NAME, t, 2, 0, 10, device="cuda:0", allow_device=True)
  assert host is None and dev.dtype == torch.int32 and dev.shape == (2,) and dev.data_ptr() == t.data_ptr()
  for bad in (_gpu([5, 7], torch.int64), _gpu([5, 7, 9], torch.int32), _gpu([[5, 7]], torch.int32),
              _gpu([5, 7], torch.float32)):
    with pytest.raises(WgError, match="int32") as e:
      _args.counts(NAME, bad, 2, 0, 10, device="cuda:0", allow_device=True)
    assert str(e.value).startswith(NAME)
  for other in ("cuda:1", "cpu"):                                  # on another device than the call's
    with pytest.raises(WgError, match="int32"):
      _args.counts(NAME, t, 2, 0, 10, device=other, allow_device=True)


def test_tensor_refusals():
  cpu = torch.zeros((2, 3))
  with pytest.raises(WgError, match="no CPU fallback") as e:
    _args.tensor("entry: audio", cpu, ndim=2)
  assert str(e.value).startswith("entry: audio")
  for bad in ([[0.0] * 3] * 2, np.zeros((2, 3), np.float32), None):
    with pytest.raises(WgError, match="entry: audio must be a tensor"):
      _args.tensor("entry: audio", bad, ndim=2)
  ok = cpu.as_subclass(OnGpu)
  assert _args.tensor("entry: audio", ok, ndim=2) is ok and _args.tensor("entry: audio", ok, device="cuda:0", ndim=2) is ok
  assert _args.tensor("entry: audio", ok.half(), dtypes=(torch.float32, torch.float16), ndim=2).dtype == torch.float16
  with pytest.raises(WgError, match="no CPU fallback"):            # the right kind of device, the wrong one
    _args.tensor("entry: audio", ok, device="cuda:1", ndim=2)
  with pytest.raises(WgError, match="entry: audio takes float32, got torch.float64"):
    _args.tensor("entry: audio", ok.double(), ndim=2)
  with pytest.raises(WgError, match="float32 or int16"):
    _args.tensor("entry: audio", ok.double(), dtypes=(torch.float32, torch.int16), ndim=2)
  with pytest.raises(WgError, match=r"entry: audio takes 2 dimensions, got shape \(3,\)"):
    _args.tensor("entry: audio", ok[0], ndim=2)


def test_ptr_is_none_safe():
  t = torch.zeros(4)
  assert _args.ptr(None) is None
  p = _args.ptr(t)
  assert isinstance(p, C.c_void_p) and p.value == t.data_ptr()


def test_workspace_refuses_zero_bytes():
  ws = _args.workspace(16, "cpu", "entry: batch 2 x 3")
  assert ws.dtype == torch.uint8 and ws.numel() == 16
  with pytest.raises(WgError, match="entry: batch 2 x 3: unsupported"):
    _args.workspace(0, "cpu", "entry: batch 2 x 3")


class _Lib:
  def __init__(self, fail=False):
    self.calls, self.fail = [], fail

  def wg_x_destroy(self, h):
    self.calls.append(h.value)
    if self.fail:
      raise RuntimeError("the library is gone")


def test_handle_destroys_exactly_once_and_never_raises():
  lib = _Lib()
  h = _args.Handle(lib, "wg_x_destroy")
  assert isinstance(h.value, C.c_void_p) and not h.value
  C.cast(C.byref(h.value), C.POINTER(C.c_void_p))[0] = 1234          # what a *_create call does through byref
  assert h.value.value == 1234
  h.__del__()
  h.__del__()
  del h
  assert lib.calls == [1234]
  empty = _args.Handle(lib, "wg_x_destroy")                          # a create that failed: nothing to release
  del empty
  assert lib.calls == [1234]
  for bad in (_Lib(fail=True), object()):                           # a destroy that raises, a library without the symbol
    h = _args.Handle(bad, "wg_x_destroy")
    h.value.value = 7
    h.__del__()
    del h
