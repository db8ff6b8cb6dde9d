"""Resampling by a rational ratio on the device (``wg_resample``): wav data of any sampling rate in, any rate out.

The definition is ``scipy.signal.resample_poly(x, up, down)`` with its defaults (``window=('kaiser', 5.0)``,
``padtype='constant'``) in closed form.  With ``up / down`` reduced, ``M = max(up, down)``, ``half = 10 M`` and
``h = up * firwin(2 half + 1, 1 / M, window=('kaiser', 5.0))`` in fp64::

    out_len(len) = ceil(len up / down)
    y[n] = sum over m ascending, 0 <= m < len with 0 <= half + n down - m up <= 2 half, of x[m] h[half + n down - m up]

The taps come from ``scipy.signal.firwin`` itself (no restatement) and go to the device as the reversed polyphase table
the kernel reads (include/waveglow_amd.h).  Every product is fp32 x fp64 in fp64, the sum is fp64 in ascending ``m`` and is
rounded to fp32 once: a call gives the same bits every time and a row of a batch the bits of its own call.  No CPU
fallback.
"""
from __future__ import annotations

import ctypes as C
import math
from typing import Dict, List, Tuple

import numpy as np
import torch

from . import _args, _lib

MAX_RATE = 1024          # max(up, down) of the reduced ratio (csrc/wg_resample.h)
MAX_SAMPLES = 1 << 26    # row pitch of the input
TILE = 1024              # consecutive outputs one workgroup computes; checked against the library's on first use
MAX_PITCH = (1 << 31) - 1 - TILE     # row pitch of the output

_plans: Dict[Tuple[int, int], tuple] = {}            # reduced (up, down) -> (up, down, half, taps)
_tables: Dict[Tuple[int, int, int], torch.Tensor] = {}   # (up, down, device index) -> polyphase table on that device


def _rate(sr, what: str) -> int:
  if isinstance(sr, bool) or not isinstance(sr, (int, np.integer)):
    if not isinstance(sr, (float, np.floating)) or not float(sr).is_integer():
      raise _lib.WgError(f"resample: {what} must be a positive integer, got {sr!r}")
  sr = int(sr)
  if sr < 1:
    raise _lib.WgError(f"resample: {what} must be a positive integer, got {sr}")
  return sr


def resample_plan(sr_in, sr_out):
  """``(up, down, half, taps)`` of the step from ``sr_in`` to ``sr_out`` Hz: the reduced ratio ``up / down = sr_out /
  sr_in``, ``half = 10 max(up, down)`` and the ``2 half + 1`` fp64 taps ``up * firwin(...)`` of scipy's default filter
  (read-only; cached per ratio).  Equal rates give ``(1, 1, 0, [1.0])``: a copy.  Rates that are not positive integers and
  a reduced ratio with ``max(up, down) > 1024`` (192 kHz against 22.05 kHz is 147 / 1280) raise WgError."""
  sr_in, sr_out = _rate(sr_in, "sr_in"), _rate(sr_out, "sr_out")
  g = math.gcd(sr_in, sr_out)
  up, down = sr_out // g, sr_in // g
  if max(up, down) > MAX_RATE:
    raise _lib.WgError(f"resample: {sr_in} -> {sr_out} Hz is the ratio {up}/{down}; max(up, down) <= {MAX_RATE} is the limit")
  plan = _plans.get((up, down))
  if plan is None:
    if up == down:
      half, taps = 0, np.ones(1, dtype=np.float64)
    else:
      from scipy.signal import firwin
      M = max(up, down)
      half = 10 * M
      taps = up * firwin(2 * half + 1, 1.0 / M, window=("kaiser", 5.0))
    taps = np.ascontiguousarray(taps, dtype=np.float64)
    taps.setflags(write=False)
    plan = _plans[(up, down)] = (up, down, half, taps)
  return plan


def out_len(n: int, up: int, down: int) -> int:
  """Samples ``n`` input samples become: ``ceil(n up / down)``."""
  return (int(n) * int(up) + int(down) - 1) // int(down)


def polyphase_table(up: int, half: int, taps: np.ndarray) -> np.ndarray:
  """The layout ``wg_resample`` reads: fp64 ``[up, K]``, ``K = ceil((2 half + 1) / up)``, every row reversed --
  ``table[p, j] = taps[p + (K - 1 - j) up]``, 0 where that index exceeds ``2 half`` -- so that ascending ``j`` is
  ascending ``m`` of the definition."""
  n = 2 * half + 1
  K = (n + up - 1) // up
  padded = np.zeros(K * up, dtype=np.float64)
  padded[:n] = taps
  return np.array(padded.reshape(K, up).T[:, ::-1], dtype=np.float64, order="C", copy=True)


def kernel_plan(sr_in, sr_out) -> Tuple[int, int, bool]:
  """What ``wg_resample_plan`` says of the step from ``sr_in`` to ``sr_out`` Hz: ``(K, tile, staged)`` -- the taps of one
  polyphase row, the consecutive outputs one workgroup computes, and whether the workgroups stage their samples in LDS
  (``down / up`` up to about 7) or read them through the cache.  Host arithmetic only."""
  up, down, half, _ = resample_plan(sr_in, sr_out)
  K, tile, staged = C.c_int32(), C.c_int32(), C.c_int32()
  _lib.check(_lib.load().wg_resample_plan(up, down, half, 1, None, C.byref(K), C.byref(tile), C.byref(staged)))
  return K.value, tile.value, bool(staged.value)


def _device_table(up: int, down: int, half: int, taps: np.ndarray, device: torch.device) -> torch.Tensor:
  key = (up, down, _lib.device_index(device))
  t = _tables.get(key)
  if t is None:
    tile = C.c_int32()
    _lib.check(_lib.load().wg_resample_plan(up, down, half, 1, None, None, C.byref(tile), None))
    if tile.value != TILE:                                  # a retuned kernel: TILE above has to follow it
      raise _lib.WgError(f"resample: the library computes tiles of {tile.value} outputs, this module states {TILE}")
    t = _tables[key] = torch.from_numpy(polyphase_table(up, half, taps)).to(device)
  return t


def _check_audio(audio, what: str, dtypes=(torch.float32, torch.int16)):
  _args.tensor(f"{what}: audio", audio, dtypes=dtypes, ndim=2)
  if audio.shape[0] < 1 or not 1 <= audio.shape[1] <= MAX_SAMPLES:
    raise _lib.WgError(f"{what}: audio [B, N] with B >= 1 and 1 <= N <= {MAX_SAMPLES} expected, got {tuple(audio.shape)}")


def resample_enqueue(audio: torch.Tensor, lengths_dev: torch.Tensor, sr_in, sr_out, *, clip: bool = False,
                     pitch: int = None) -> torch.Tensor:
  """Enqueue ``wg_resample`` on the current stream; nothing is read back and nothing synchronises.

  ``audio``: fp32 or int16 ``[B, N]`` on the GPU (int16 counts as ``x / 32768``), ``lengths_dev``: int32 ``[B]`` on that
  GPU, read by the kernel only (a length outside ``[0, N]`` counts as 0; nothing at or behind a row's length is read).
  Returns fp32 ``[B, out_len(N)]`` -- ``[B, pitch]`` for a ``pitch >= out_len(N)`` -- with row b holding
  ``out_len(lengths[b])`` samples and zeros behind them.  ``clip`` clamps the result to [-1, 1]."""
  _check_audio(audio, "resample")
  B, N = audio.shape
  lengths_dev, _ = _args.counts("resample_enqueue: lengths", lengths_dev, B, 0, N, device=audio.device, allow_device=True)
  up, down, half, taps = resample_plan(sr_in, sr_out)
  n_out = out_len(N, up, down)
  if pitch is not None:
    if int(pitch) < n_out:
      raise _lib.WgError(f"resample: pitch {pitch} below the {n_out} outputs of {N} samples")
    n_out = int(pitch)
  if n_out > MAX_PITCH:
    raise _lib.WgError(f"resample: rows of {n_out} outputs ({N} samples at {up}/{down}) are beyond {MAX_PITCH}")
  audio = audio.contiguous()
  table = _device_table(up, down, half, taps, audio.device)
  out = torch.empty((B, n_out), dtype=torch.float32, device=audio.device)
  _lib.check(_lib.load().wg_resample(_args.ptr(audio), _lib.WG_PCM_I16 if audio.dtype == torch.int16 else _lib.WG_PCM_F32,
                                     _args.ptr(lengths_dev), _args.ptr(out), _args.ptr(table), up, down, half,
                                     _lib.WG_RESAMPLE_CLIP if clip else 0, B, N, n_out, _args.stream(audio.device)))
  return out


def check_lengths(lengths, B: int, N: int) -> List[int]:
  """``lengths`` (None: all N; B integers in [0, N] as ``_args.counts`` takes them) as a list."""
  return [N] * B if lengths is None else _args.counts("resample: lengths", lengths, B, 0, N, device=None)[1]


def resample(audio: torch.Tensor, lengths, sr_in, sr_out, *, clip: bool = False):
  """``(out, out_lengths)``: ``audio`` (fp32 or int16 ``[B, N]`` on the GPU) resampled from ``sr_in`` to ``sr_out`` Hz.

  ``lengths``: None (all N), or B integers as ``_args.counts`` takes them (a list, a tuple or a 1-D CPU tensor of an
  integer dtype; a float or a bool entry raises WgError), each in [0, N].  ``out``: fp32 ``[B, out_len(N)]`` on the
  device, row b holding ``out_lengths[b] = out_len(lengths[b])`` samples -- ``scipy.signal.resample_poly`` of the crop,
  rounded to fp32 once -- and zeros behind them; ``out_lengths`` is a list.  Enqueues on the current stream (one small
  upload for the lengths, one launch) and never synchronises.  ``sr_in == sr_out`` copies.  CPU tensors, other dtypes,
  other ranks and lengths outside the range raise WgError."""
  _check_audio(audio, "resample")
  up, down, _, _ = resample_plan(sr_in, sr_out)
  B, N = audio.shape
  lens_dev, lens = _args.counts("resample: lengths", [N] * B if lengths is None else lengths, B, 0, N, device=audio.device)
  return resample_enqueue(audio, lens_dev, sr_in, sr_out, clip=clip), [out_len(n, up, down) for n in lens]


# ------------------------------------------------------------------------------------------------- the differentiable path
_tables_t: Dict[Tuple[int, int, int], torch.Tensor] = {}   # (up, down, device index) -> transposed table on that device


def polyphase_table_backward(down: int, half: int, taps: np.ndarray) -> np.ndarray:
  """The layout ``wg_resample_backward`` reads: fp64 ``[down, Kt]``, ``Kt = ceil((2 half + 1) / down)``,
  ``table[r, i] = taps[r + i down]``, 0 where that index exceeds ``2 half``.  Input sample ``m`` reads row
  ``r = (half - m up) mod down`` in ascending ``i``, which is ascending ``n`` of the definition."""
  n = 2 * half + 1
  Kt = (n + down - 1) // down
  padded = np.zeros(Kt * down, dtype=np.float64)
  padded[:n] = taps
  return np.array(padded.reshape(Kt, down).T, dtype=np.float64, order="C", copy=True)


def _device_table_backward(up: int, down: int, half: int, taps: np.ndarray, device: torch.device) -> torch.Tensor:
  key = (up, down, _lib.device_index(device))
  t = _tables_t.get(key)
  if t is None:
    t = _tables_t[key] = torch.from_numpy(polyphase_table_backward(down, half, taps)).to(device)
  return t


def resample_backward_enqueue(d_out: torch.Tensor, lengths_dev: torch.Tensor, sr_in, sr_out, n_in: int) -> torch.Tensor:
  """Enqueue ``wg_resample_backward`` on the current stream: the gradient with respect to the fp32 ``[B, n_in]`` input of
  ``resample_enqueue(audio, lengths_dev, sr_in, sr_out)`` (not clipped) from ``d_out``, fp32 or fp64 ``[B, n_out]`` with
  ``n_out >= out_len(n_in)``, the gradient with respect to its result.  ``lengths_dev`` are the lengths of the INPUT rows,
  int32 ``[B]`` on the device.  Returns fp32 ``[B, n_in]``: written below a row's length, exact zeros behind; nothing of
  ``d_out`` at or behind ``out_len(length)`` is read."""
  _args.tensor("resample backward: d_out", d_out, dtypes=(torch.float32, torch.float64), ndim=2)
  B, n_out = d_out.shape
  n_in = int(n_in)
  if B < 1 or not 1 <= n_in <= MAX_SAMPLES:
    raise _lib.WgError(f"resample backward: B >= 1 and 1 <= n_in <= {MAX_SAMPLES} expected, got {B} and {n_in}")
  lengths_dev, _ = _args.counts("resample backward: lengths", lengths_dev, B, 0, n_in, device=d_out.device,
                                allow_device=True)
  up, down, half, taps = resample_plan(sr_in, sr_out)
  if n_out < out_len(n_in, up, down) or n_out > MAX_PITCH:
    raise _lib.WgError(f"resample backward: rows of {n_out} gradients do not fit {n_in} samples at {up}/{down}")
  d_out = d_out.contiguous()
  table = _device_table_backward(up, down, half, taps, d_out.device)
  d_in = torch.empty((B, n_in), dtype=torch.float32, device=d_out.device)
  _lib.check(_lib.load().wg_resample_backward(
    _args.ptr(d_out), _lib.WG_PCM_F64 if d_out.dtype == torch.float64 else _lib.WG_PCM_F32, _args.ptr(lengths_dev),
    _args.ptr(d_in), _args.ptr(table), up, down, half, B, n_in, n_out, _args.stream(d_out.device)))
  return d_in


class _ResampleFn(torch.autograd.Function):
  """audio [B, N] fp32 -> ``resample_enqueue`` of it; the backward is one ``wg_resample_backward`` launch and writes to
  nothing the forward left, so a second backward under retain_graph gives the same bits."""

  @staticmethod
  def forward(ctx, audio, lens_dev, sr_in, sr_out):
    ctx.lens, ctx.rates, ctx.n_in = lens_dev, (sr_in, sr_out), audio.shape[1]
    return resample_enqueue(audio.detach(), lens_dev, sr_in, sr_out)

  @staticmethod
  def backward(ctx, g):
    with torch.cuda.device(g.device):
      return resample_backward_enqueue(g, ctx.lens, ctx.rates[0], ctx.rates[1], ctx.n_in), None, None, None


def resample_differentiable(audio: torch.Tensor, lengths, sr_in, sr_out, *, clip: bool = False):
  """``(out, out_lengths)`` with the bits of ``resample(audio, lengths, sr_in, sr_out, clip=False)`` and a graph back to
  ``audio`` (fp32 ``[B, N]`` on the GPU only): ``audio.grad`` is the transposed polyphase filter of the incoming gradient
  (``wg_resample_backward``), exactly 0 behind a row's length.  There is no clipped variant: ``clip=True`` raises WgError.
  Without grad mode, or when ``audio`` does not require grad, this is plain ``resample``.  No double backward."""
  if clip:
    raise _lib.WgError("resample_differentiable: there is no clipped variant of the differentiable path")
  _check_audio(audio, "resample_differentiable", (torch.float32,))
  up, down, _, _ = resample_plan(sr_in, sr_out)
  B, N = audio.shape
  graph = torch.is_grad_enabled() and audio.requires_grad
  lens_dev, lens = _args.counts("resample_differentiable: lengths", [N] * B if lengths is None else lengths, B, 0, N,
                                device=audio.device if graph else None)
  if not graph:
    return resample(audio, lens, sr_in, sr_out)
  with torch.cuda.device(audio.device):
    out = _ResampleFn.apply(audio, lens_dev, sr_in, sr_out)
  return out, [out_len(n, up, down) for n in lens]
