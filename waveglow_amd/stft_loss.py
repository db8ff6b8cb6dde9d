"""Multi-resolution STFT loss (spectral convergence + log-magnitude L1, as in Parallel WaveGAN) computed by the HIP
library (``wg_stftloss_*``): conv-STFTs at run-time geometry on exact-fp32 MFMA, device-side reductions in a fixed
order, and the matching backward.  The waveform-domain loss that ``WaveGlow.infer_differentiable`` is built for.

For one resolution ``(n_fft, hop, win)``: ``X = STFT(x)`` with reflect padding by ``n_fft / 2`` and the periodic window
of ``win`` samples centred in ``n_fft`` (``torch.stft(x, n_fft, hop, win, hann_window(win), center=True,
pad_mode="reflect")``), ``M = sqrt(max(re^2 + im^2, eps))``,

  sc_r  = ||M(y) - M(x)||_F / ||M(y)||_F        (norms over the whole batch)
  mag_r = mean |log M(y) - log M(x)|            (over all B K F elements)

and ``loss = factor_sc * mean_r sc_r + factor_mag * mean_r mag_r``.  No torch / CPU fallback.

With ``lengths`` (a padded batch of utterances of different lengths) utterance ``b`` is transformed as its own crop
``x[b, :lengths[b]]``: reflect padding about its own last sample, ``F_b = lengths[b] // hop + 1`` frames; the norms run
over the frames of all crops and the mean divides by ``K * sum_b F_b``.  That is the loss of the cropped utterances with
their frames concatenated; the samples behind an utterance's end are never read and get a zero gradient.
"""
from __future__ import annotations

import ctypes as C

import numpy as np
import torch
from scipy.signal import get_window

from . import _args, _lib

MAX_RESOLUTIONS, MAX_FFT = 8, 2048


def forward_basis(n_fft: int, win_length: int, window: str = "hann") -> np.ndarray:
  """The windowed Fourier basis [2 * (n_fft / 2 + 1), n_fft] fp32, real rows then imaginary rows: the forward basis of
  ``denoiser.stft_bases(n_fft, hop, win_length, window)``, value for value, without its pseudo-inverse."""
  fb = np.fft.fft(np.eye(n_fft))
  cutoff = n_fft // 2 + 1
  fb = np.vstack([np.real(fb[:cutoff]), np.imag(fb[:cutoff])])
  win = get_window(window, win_length, fftbins=True)
  lpad = (n_fft - win_length) // 2
  win = np.pad(win, (lpad, n_fft - win_length - lpad))
  return np.ascontiguousarray(fb * win, dtype=np.float32)


def check_geometry(fft_sizes, hop_sizes, win_lengths):
  """Raise WgError unless the resolutions are ones the kernels support (see MultiResolutionSTFTLoss)."""
  if not (len(fft_sizes) == len(hop_sizes) == len(win_lengths)):
    raise _lib.WgError("fft_sizes, hop_sizes and win_lengths must have the same length")
  if not 1 <= len(fft_sizes) <= MAX_RESOLUTIONS:
    raise _lib.WgError(f"1 to {MAX_RESOLUTIONS} resolutions are supported, got {len(fft_sizes)}")
  for n, h, w in zip(fft_sizes, hop_sizes, win_lengths):
    if n < 32 or n > MAX_FFT or n % 32:
      raise _lib.WgError(f"n_fft must be a multiple of 32 in [32, {MAX_FFT}], got {n}")
    if not 1 <= h <= n:
      raise _lib.WgError(f"hop must be in [1, n_fft], got {h} for n_fft {n}")
    if not 1 <= w <= n:
      raise _lib.WgError(f"win_length must be in [1, n_fft], got {w} for n_fft {n}")


def check_lengths(lengths, B: int, N: int, min_exclusive: int):
  """``lengths`` of a padded batch [B, N] as a list of B ints, each in (min_exclusive, N]; anything else raises WgError
  naming the offending value (``_args.counts``).  Pure host code."""
  return _args.counts("lengths", lengths, B, min_exclusive + 1, N, device=None)[1]


class _LossFn(torch.autograd.Function):
  """Inputs: the module (a _WaveformLoss), prediction and target [B, N], and the device copy of the lengths or None.
  Output: the module's device vector of three.  The forward keeps what the module's _run saved and the lengths on ctx;
  the module's _backward rewrites nothing a later backward reads, so a second backward under retain_graph gives the same
  bits."""

  @staticmethod
  def forward(ctx, crit, x, y, lens):
    out, state = crit._run(x, y, saved=True, lens=lens)
    ctx.crit, ctx.state, ctx.dims, ctx.lens = crit, state, tuple(x.shape), lens
    return out

  @staticmethod
  def backward(ctx, g_out):
    B, N = ctx.dims
    gx = ctx.crit._backward(ctx.state, g_out.to(torch.float32).contiguous(), ctx.lens, B, N)
    return None, gx, None, None


class _WaveformLoss(torch.nn.Module):
  """What the waveform losses over conv-STFTs share: input checks, the upload of the lengths, the choice between the
  graph and the no-graph path.  A subclass sets ``_NAME`` (its name in messages) and ``self._h`` (its library handle, with
  the ``_args.Handle`` that owns it in ``self._owner``), and supplies ``_need()`` (the largest ``n_fft // 2``),
  ``_run(x, y, saved, lens) -> (out3, state)`` (one library call on fp32 [B, N]; ``state`` is what the backward needs,
  nothing of it allocated unless ``saved``) and ``_backward(state, g, lens, B, N) -> gx``.  ``lens``: int32 [B] on the
  device, or None."""

  def _check(self, x, y):
    for name, t in (("audio", x), ("target", y)):
      _args.tensor(f"{self._NAME}: {name}", t, device=self.device, ndim=2)
    if x.shape != y.shape:
      raise _lib.WgError(f"audio {tuple(x.shape)} and target {tuple(y.shape)} differ in shape")
    if y.requires_grad:
      raise _lib.WgError(f"{self._NAME}: only audio gets a gradient; detach the target")
    if x.shape[0] < 1 or x.shape[1] <= self._need():
      raise _lib.WgError(f"audio of {x.shape[1]} samples is too short (reflect padding needs > {self._need()})")

  def _out3(self, audio, target, lengths=None):
    self._check(audio, target)
    B, N = audio.shape
    lens = None if lengths is None else \
        _args.counts(f"{self._NAME}: lengths", lengths, B, self._need() + 1, N, device=audio.device)[0]
    if torch.is_grad_enabled() and audio.requires_grad:
      return _LossFn.apply(self, audio, target, lens)
    return self._run(audio, target, saved=False, lens=lens)[0]

  def terms(self, audio: torch.Tensor, target: torch.Tensor, lengths=None):
    """The two terms of the loss (see the class), each averaged over the resolutions or scales."""
    out = self._out3(audio, target, lengths)
    return out[0], out[1]

  def forward(self, audio: torch.Tensor, target: torch.Tensor, lengths=None) -> torch.Tensor:
    return self._out3(audio, target, lengths)[2]


class MultiResolutionSTFTLoss(_WaveformLoss):
  """``crit(audio, target, lengths=None)`` -> 0-dim fp32 loss on the device with a graph back to ``audio``;
  ``crit.terms(audio, target, lengths=None)`` -> ``(sc, mag)``.

  ``lengths``: B integers as ``_args.counts`` takes them (a list, a tuple or a 1-D CPU tensor of an integer dtype; a
  float or a bool entry raises WgError), the sample count of every utterance of a padded batch, each in
  ``(max(fft_sizes) / 2, N]``; they go up in one small copy per call.  The loss is then that of the crops ``audio[b,
  :lengths[b]]`` with their frames concatenated (see the module docstring), ``audio.grad[b, lengths[b]:]`` is 0, and
  ``lengths=[N] * B`` gives the bits of ``lengths=None``.

  ``audio``, ``target``: fp32 ``[B, N]`` on the module's device, same shape, ``N > max(fft_sizes) / 2``; anything else
  raises WgError.  Only ``audio`` gets a gradient (a ``target`` that requires grad raises WgError); the clamp at ``eps``
  passes no gradient where ``re^2 + im^2 < eps`` and ``sign(0) = 0``, as in plain torch.  Without grad mode, or when
  ``audio`` does not require grad, the same values come back with no graph and nothing saved.  No host synchronisation
  in forward or backward; values and gradients are bit-reproducible (fixed-order reductions, no atomics).

  Supported geometries: 1 to 8 resolutions, each with ``n_fft`` a multiple of 32 in [32, 2048], ``1 <= hop <= n_fft``
  (it need not divide ``n_fft``) and ``1 <= win_length <= n_fft``; ``window`` is any name ``scipy.signal.get_window``
  knows.  Everything else raises WgError at construction."""

  _NAME = "MultiResolutionSTFTLoss"

  def __init__(self, fft_sizes=(1024, 2048, 512), hop_sizes=(120, 240, 50), win_lengths=(600, 1200, 240),
               window="hann", factor_sc=1.0, factor_mag=1.0, eps=1e-7, device="cuda"):
    super().__init__()
    device = torch.device(device)
    if device.type != "cuda":
      raise _lib.WgError("the STFT loss runs on the GPU library only")
    fft_sizes, hop_sizes, win_lengths = (tuple(int(v) for v in t) for t in (fft_sizes, hop_sizes, win_lengths))
    check_geometry(fft_sizes, hop_sizes, win_lengths)
    if not eps > 0:
      raise _lib.WgError(f"eps must be positive, got {eps}")
    self.resolutions = tuple(zip(fft_sizes, hop_sizes, win_lengths))
    self.factor_sc, self.factor_mag, self.eps = float(factor_sc), float(factor_mag), float(eps)
    self.device = device
    self.lib = _lib.load()
    n = len(fft_sizes)
    bases = [forward_basis(nf, w, window) for nf, _, w in self.resolutions]
    arr = lambda v: (C.c_int32 * n)(*v)
    ptrs = (C.c_void_p * n)(*[b.ctypes.data for b in bases])
    self._owner = _args.Handle(self.lib, "wg_stftloss_destroy")
    self._h = self._owner.value                # what every call takes; the owner releases it
    _lib.check(self.lib.wg_stftloss_create(n, arr(fft_sizes), arr(hop_sizes), arr(win_lengths), ptrs, self.eps,
                                           _lib.device_index(device), C.byref(self._h)))

  def workspace_bytes(self, B: int, N: int) -> int:
    """Bytes one forward with a graph keeps until its backward (0 when N <= max(fft_sizes) / 2): per resolution the
    prediction's (re, im) [B, n_fft, F] and M(target) [B, n_fft / 2 + 1, F] (F rounded up to 64), the per-workgroup
    sums, and one frame-gradient scratch [B, F, win] that the backward reuses for every resolution."""
    return int(self.lib.wg_stftloss_workspace_bytes(self._h, B, N, 1))

  def _need(self):
    return max(n for n, _, _ in self.resolutions) // 2

  def _run(self, x, y, saved, lens=None):
    """One library call on contiguous fp32 [B, N]: (out3, workspace).  lens: int32 [B] on the device, or None."""
    x, y = x.detach().contiguous(), y.detach().contiguous()
    B, N = x.shape
    ws = _args.workspace(self.lib.wg_stftloss_workspace_bytes(self._h, B, N, 1 if saved else 0), x.device,
                         f"MultiResolutionSTFTLoss: batch {B} x {N}")
    out = torch.empty(3, dtype=torch.float32, device=x.device)
    _lib.check(self.lib.wg_stftloss_forward(self._h, _args.ptr(x), _args.ptr(y), _args.ptr(lens), self.factor_sc,
                                            self.factor_mag, _args.ptr(out), B, N, 1 if saved else 0, _args.ptr(ws),
                                            ws.numel(), _args.stream(x.device)))
    return out, ws

  def _backward(self, ws, g, lens, B, N):
    gx = torch.empty((B, N), dtype=torch.float32, device=ws.device)
    _lib.check(self.lib.wg_stftloss_backward(self._h, _args.ptr(g), _args.ptr(lens), self.factor_sc,
                                             self.factor_mag, _args.ptr(gx), B, N, _args.ptr(ws), ws.numel(),
                                             _args.stream(ws.device)))
    return gx
