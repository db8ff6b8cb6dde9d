"""What every binding in this package decides the same way: how per-utterance counts are accepted, what a tensor argument
must be, and who releases a library handle -- with the three lines of plumbing that stand around every library call.

Counts (``lengths``, ``frames``) are B integers: a list, a tuple, a range or a 1-D CPU tensor of an integer dtype, every
entry an ``int`` or a ``numpy.integer`` within the limits of the call; floats, bools and everything else raise WgError,
here and nowhere else.  Where a call allows it, an int32 tensor ``[B]`` on the device is taken as it is: trusted, never
read on the host.  Pure host code but for the one small upload; nothing here launches or synchronises.
"""
from __future__ import annotations

import ctypes as C

import numpy as np
import torch

from . import _lib
from ._lib import WgError


def counts(name: str, values, B: int, lo: int, hi: int, *, device, multiple_of: int = 1, allow_device: bool = False):
  """``(dev, host)`` of B per-utterance counts, each a multiple of ``multiple_of`` in ``[lo, hi]``: ``dev`` int32 ``[B]``,
  contiguous, on ``device`` (one small copy, nothing synchronised; None for ``device=None``, the check alone) and ``host``
  the list of ints.  With ``allow_device`` an int32 ``[B]`` tensor on ``device`` comes back as ``dev`` with ``host`` None:
  its values are never read here.  Anything else raises a WgError that starts with ``name`` (``"entry point: noun"``) and
  names the offending value and the bound."""
  what = name.rsplit(": ", 1)[-1]
  if isinstance(values, torch.Tensor) and values.device.type != "cpu":
    if not allow_device:
      raise WgError(f"{name} must be host integers (a list, a tuple or a CPU tensor), got a tensor on {values.device}")
    device = torch.device(device)
    if values.dtype != torch.int32 or values.dim() != 1 or values.numel() != B or values.device.type != device.type or \
        _lib.device_index(values.device) != _lib.device_index(device):
      raise WgError(f"{name} on the device must be int32 [{B}] on {device}, got {values.dtype} {tuple(values.shape)} on "
                    f"{values.device}")
    return values.contiguous(), None
  if isinstance(values, torch.Tensor):
    if values.dim() != 1 or values.dtype.is_floating_point or values.dtype.is_complex or values.dtype == torch.bool:
      raise WgError(f"{name}: a 1-d tensor of integer {what} expected, got {values.dtype} of shape {tuple(values.shape)}")
    values = values.tolist()
  elif not isinstance(values, (list, tuple, range)):
    raise WgError(f"{name}: a list, a tuple or a tensor of integer {what} expected, got {type(values).__name__}")
  if len(values) != B:
    raise WgError(f"{name}: {len(values)} {what} for a batch of {B}")
  host = []
  for b, n in enumerate(values):
    if isinstance(n, bool) or not isinstance(n, (int, np.integer)):
      raise WgError(f"{name}[{b}] = {n!r} is not an integer: integer {what} expected, got {list(values)}")
    if not lo <= n <= hi or n % multiple_of:
      step = f"multiples of {multiple_of} " if multiple_of != 1 else ""
      raise WgError(f"{name}[{b}] = {n} is outside [{lo}, {hi}]: {what} {step}in [{lo}, {hi}] expected, got {list(values)}")
    host.append(int(n))
  return (None if device is None else torch.tensor(host, dtype=torch.int32).to(device)), host


def tensor(name: str, t, *, device=None, dtypes=(torch.float32,), ndim: int):
  """``t`` if it is a tensor on the GPU -- on ``device``'s index when one is given -- of one of ``dtypes`` and of rank
  ``ndim``; WgError otherwise.  Shape limits that belong to one kernel stay with its caller."""
  if not isinstance(t, torch.Tensor) or t.device.type != "cuda" or \
      (device is not None and _lib.device_index(t.device) != _lib.device_index(device)):
    where = "the GPU" if device is None else str(device)
    got = t.device if isinstance(t, torch.Tensor) else type(t).__name__
    raise WgError(f"{name} must be a tensor on {where}, got {got}: the GPU library only, no CPU fallback")
  if t.dtype not in dtypes:
    raise WgError(f"{name} takes {' or '.join(str(d).replace('torch.', '') for d in dtypes)}, got {t.dtype}")
  if t.dim() != ndim:
    raise WgError(f"{name} takes {ndim} dimensions, got shape {tuple(t.shape)}")
  return t


def ptr(t):
  """The device pointer of a tensor as the library takes it; None stays None (an optional argument left out)."""
  return C.c_void_p(t.data_ptr()) if t is not None else None


def stream(device) -> C.c_void_p:
  """torch's current stream on ``device``, as the library takes it."""
  return C.c_void_p(torch.cuda.current_stream(device).cuda_stream)


def workspace(nbytes: int, device, what: str) -> torch.Tensor:
  """A uint8 scratch tensor of the size the library asked for; 0 bytes is its answer for a shape it does not take."""
  if nbytes == 0:
    raise WgError(f"{what}: unsupported")
  return torch.empty(nbytes, dtype=torch.uint8, device=device)


class Handle:
  """Owns one library handle.  ``C.byref(h.value)`` goes to the ``*_create`` call, ``h.value`` to every call after it, and
  ``destroy_name`` runs once when the owner goes -- silently: at interpreter shutdown the library may be gone first."""

  def __init__(self, lib, destroy_name: str):
    self.lib, self.destroy_name, self.value = lib, destroy_name, C.c_void_p()

  def __del__(self):
    try:
      if self.value:
        value, self.value = self.value, None
        getattr(self.lib, self.destroy_name)(value)
    except Exception:
      pass
