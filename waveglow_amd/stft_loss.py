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

from . import _lib

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
  naming the offending value.  ``lengths``: a list, tuple or CPU tensor of integers.  Pure host code."""
  if isinstance(lengths, torch.Tensor):
    if lengths.device.type != "cpu":
      raise _lib.WgError("lengths must be host integers (a list, a tuple or a CPU tensor)")
    if lengths.dim() != 1 or lengths.dtype.is_floating_point or lengths.dtype.is_complex or lengths.dtype == torch.bool:
      raise _lib.WgError(f"lengths must be a 1-D integer tensor, got {lengths.dtype} of shape {tuple(lengths.shape)}")
    lengths = lengths.tolist()
  elif not isinstance(lengths, (list, tuple)):
    raise _lib.WgError(f"lengths must be a list, a tuple or a CPU tensor, got {type(lengths).__name__}")
  if len(lengths) != B:
    raise _lib.WgError(f"{len(lengths)} lengths for a batch of {B}")
  out = []
  for b, n in enumerate(lengths):
    if isinstance(n, bool) or not isinstance(n, (int, np.integer)):
      raise _lib.WgError(f"lengths[{b}] = {n!r} is not an integer")
    if not min_exclusive < n <= N:
      raise _lib.WgError(f"lengths[{b}] = {n} is outside ({min_exclusive}, {N}] (reflect padding needs > "
                         f"{min_exclusive} samples, the batch holds {N})")
    out.append(int(n))
  return out


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
  graph and the no-graph path, and the handle's release.  A subclass sets ``_NAME`` (its name in messages) and
  ``_DESTROY`` (the library function that frees ``self._h``), and supplies ``_need()`` (the largest ``n_fft // 2``),
  ``_run(x, y, saved, lens) -> (out3, state)`` (one library call on fp32 [B, N]; ``state`` is what the backward needs,
  nothing of it allocated unless ``saved``) and ``_backward(state, g, lens, B, N) -> gx``.  ``lens``: int32 [B] on the
  device, or None."""

  def __del__(self):
    try:
      if getattr(self, "_h", None):
        getattr(self.lib, self._DESTROY)(self._h)
    except Exception:
      pass

  def _check(self, x, y):
    for name, t in (("audio", x), ("target", y)):
      if not isinstance(t, torch.Tensor) or t.device.type != "cuda" or \
          _lib.device_index(t.device) != _lib.device_index(self.device):
        raise _lib.WgError(f"{self._NAME}: {name} must be on {self.device} (no CPU fallback)")
      if t.dtype != torch.float32:
        raise _lib.WgError(f"{self._NAME} takes float32 {name}, got {t.dtype}")
      if t.dim() != 2:
        raise _lib.WgError(f"{self._NAME} takes {name} [B, N], got shape {tuple(t.shape)}")
    if x.shape != y.shape:
      raise _lib.WgError(f"audio {tuple(x.shape)} and target {tuple(y.shape)} differ in shape")
    if y.requires_grad:
      raise _lib.WgError(f"{self._NAME}: only audio gets a gradient; detach the target")
    if x.shape[0] < 1 or x.shape[1] <= self._need():
      raise _lib.WgError(f"audio of {x.shape[1]} samples is too short (reflect padding needs > {self._need()})")

  def _lens(self, lengths, x):
    """The checked lengths as an int32 tensor on x's device (one small copy), or None."""
    if lengths is None:
      return None
    B, N = x.shape
    return torch.tensor(check_lengths(lengths, B, N, self._need()), dtype=torch.int32).to(x.device)

  def _out3(self, audio, target, lengths=None):
    self._check(audio, target)
    lens = self._lens(lengths, audio)
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

  ``lengths``: B host integers (list, tuple or CPU tensor), the sample count of every utterance of a padded batch, each
  in ``(max(fft_sizes) / 2, N]`` (checked on the host by ``check_lengths``, WgError otherwise); they go up in one small
  copy per call.  The loss is then that of the crops ``audio[b, :lengths[b]]`` with their frames concatenated (see the
  module docstring), ``audio.grad[b, lengths[b]:]`` is 0, and ``lengths=[N] * B`` gives the bits of ``lengths=None``.

  ``audio``, ``target``: fp32 ``[B, N]`` on the module's device, same shape, ``N > max(fft_sizes) / 2``; anything else
  raises WgError.  Only ``audio`` gets a gradient (a ``target`` that requires grad raises WgError); the clamp at ``eps``
  passes no gradient where ``re^2 + im^2 < eps`` and ``sign(0) = 0``, as in plain torch.  Without grad mode, or when
  ``audio`` does not require grad, the same values come back with no graph and nothing saved.  No host synchronisation
  in forward or backward; values and gradients are bit-reproducible (fixed-order reductions, no atomics).

  Supported geometries: 1 to 8 resolutions, each with ``n_fft`` a multiple of 32 in [32, 2048], ``1 <= hop <= n_fft``
  (it need not divide ``n_fft``) and ``1 <= win_length <= n_fft``; ``window`` is any name ``scipy.signal.get_window``
  knows.  Everything else raises WgError at construction."""

  _NAME, _DESTROY = "MultiResolutionSTFTLoss", "wg_stftloss_destroy"

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
    self._h = C.c_void_p()
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
    nbytes = self.lib.wg_stftloss_workspace_bytes(self._h, B, N, 1 if saved else 0)
    if nbytes == 0:
      raise _lib.WgError(f"MultiResolutionSTFTLoss: unsupported batch {B} x {N}")
    out = torch.empty(3, dtype=torch.float32, device=x.device)
    ws = torch.empty(nbytes, dtype=torch.uint8, device=x.device)
    stream = torch.cuda.current_stream(x.device).cuda_stream
    _lib.check(self.lib.wg_stftloss_forward(self._h, x.data_ptr(), y.data_ptr(),
                                            lens.data_ptr() if lens is not None else None, self.factor_sc,
                                            self.factor_mag, out.data_ptr(), B, N, 1 if saved else 0, ws.data_ptr(),
                                            ws.numel(), C.c_void_p(stream)))
    return out, ws

  def _backward(self, ws, g, lens, B, N):
    gx = torch.empty((B, N), dtype=torch.float32, device=ws.device)
    stream = torch.cuda.current_stream(ws.device).cuda_stream
    _lib.check(self.lib.wg_stftloss_backward(self._h, g.data_ptr(), lens.data_ptr() if lens is not None else None,
                                             self.factor_sc, self.factor_mag, gx.data_ptr(), B, N, ws.data_ptr(),
                                             ws.numel(), C.c_void_p(stream)))
    return gx
