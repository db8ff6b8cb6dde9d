"""Multi-scale mel-spectrogram loss (HiFi-GAN's mel L1 in the multi-scale form of DAC and BigVGAN) computed by the HIP
library (``wg_melloss_*``): the conv-STFTs of the STFT loss on exact-fp32 MFMA, a sparse mel projection, device-side
reductions in a fixed order, and the matching backward.

For one scale ``(n_fft, hop, win, n_mels)`` with the bank ``W`` ``[n_mels, n_fft / 2 + 1]``: ``X = STFT(x)`` as in
``stft_loss`` (``torch.stft(x, n_fft, hop, win, hann_window(win), center=True, pad_mode="reflect")``),
``M = sqrt(re^2 + im^2)``, ``mel = W M``, ``lmel = ln(max(mel, clamp))``,

  log_r = mean |lmel(x) - lmel(y)|              (over all n_mels * sum_b F_b cells)
  lin_r = mean |mel(x) - mel(y)|

and ``loss = factor_log * mean_r log_r + factor_lin * mean_r lin_r``.  No torch / CPU fallback.  DAC takes ``log10``
where this loss takes ``ln``: a factor ``ln 10`` on the log term.

With ``lengths`` utterance ``b`` is its own crop ``x[b, :lengths[b]]``, exactly as in the ragged STFT loss: reflect
padding about its own last sample, ``F_b = lengths[b] // hop + 1`` frames, the means over the cells of all crops; the
samples behind an utterance's end are never read and get a zero gradient.
"""
from __future__ import annotations

import ctypes as C
import math

import numpy as np
import torch

from . import _args, _lib
from .stft_loss import _WaveformLoss, check_geometry, forward_basis
from .taco_stft import slaney_mel_filterbank

DAC_N_FFTS = (32, 64, 128, 256, 512, 1024, 2048)
DAC_N_MELS = (5, 10, 20, 40, 80, 160, 320)


def check_scales(n_ffts, hop_sizes, win_lengths, n_mels):
  """Raise WgError unless the scales are ones the kernels support (see MultiScaleMelLoss)."""
  if len(n_mels) != len(n_ffts):
    raise _lib.WgError("n_ffts and n_mels must have the same length")
  check_geometry(n_ffts, hop_sizes, win_lengths)
  for n, m in zip(n_ffts, n_mels):
    if not 1 <= m <= n // 2 + 1:
      raise _lib.WgError(f"n_mels must be in [1, n_fft / 2 + 1], got {m} for n_fft {n}")


class MultiScaleMelLoss(_WaveformLoss):
  """``crit(audio, target, lengths=None)`` -> 0-dim fp32 loss on the device with a graph back to ``audio``;
  ``crit.terms(audio, target, lengths=None)`` -> ``(log, lin)``.

  Scales: ``n_ffts`` and ``n_mels`` of equal length (the defaults are DAC's); ``hop_sizes=None`` means ``n_fft // 4``,
  ``win_lengths=None`` means ``n_fft``, ``fmax=None`` means ``sampling_rate / 2``.  The banks are
  ``taco_stft.slaney_mel_filterbank(sampling_rate, n_fft, n_mels, fmin, fmax)``; ``mel_bases=`` takes a list of dense
  fp32 arrays ``[n_mels, n_fft / 2 + 1]`` instead (``sampling_rate``, ``fmin`` and ``fmax`` are then unused).  A bank row
  of zeros is legal.

  ``lengths``: B integers as ``_args.counts`` takes them (a list, a tuple or a 1-D CPU tensor of an integer dtype; a
  float or a bool entry raises WgError), each in ``(max(n_ffts) / 2, N]``; they go up in one small copy per call.
  ``audio.grad[b, lengths[b]:]`` is 0 and ``lengths=[N] * B`` gives the bits of ``lengths=None``.

  ``audio``, ``target``: fp32 ``[B, N]`` on the module's device, same shape, ``N > max(n_ffts) / 2``; anything else
  raises WgError.  Only ``audio`` gets a gradient (a ``target`` that requires grad raises WgError): ``sign(0) = 0``, the
  log term passes nothing where ``mel(x) < clamp``, a bin with ``re^2 + im^2 = 0`` gets 0.  Without grad mode, or when
  ``audio`` does not require grad, the same value bits come back with no graph and nothing saved.  The current stream is
  used, nothing synchronises, and values and gradients are bit-reproducible (fixed-order reductions, no atomics).  No
  double backward.

  Supported: 1 to 8 scales, ``n_fft`` a multiple of 32 in [32, 2048], ``1 <= hop, win <= n_fft``,
  ``1 <= n_mels <= n_fft / 2 + 1``, ``clamp > 0`` and finite.  Everything else raises WgError at construction."""

  _NAME = "MultiScaleMelLoss"

  def __init__(self, sampling_rate=22050, n_ffts=DAC_N_FFTS, hop_sizes=None, win_lengths=None, n_mels=DAC_N_MELS,
               fmin=0.0, fmax=None, clamp=1e-5, factor_log=1.0, factor_lin=0.0, device="cuda", mel_bases=None):
    super().__init__()
    device = torch.device(device)
    if device.type != "cuda":
      raise _lib.WgError("the mel loss runs on the GPU library only")
    n_ffts = tuple(int(v) for v in n_ffts)
    hop_sizes = tuple(n // 4 for n in n_ffts) if hop_sizes is None else tuple(int(v) for v in hop_sizes)
    win_lengths = n_ffts if win_lengths is None else tuple(int(v) for v in win_lengths)
    n_mels = tuple(int(v) for v in n_mels)
    check_scales(n_ffts, hop_sizes, win_lengths, n_mels)
    clamp = float(clamp)
    if not (clamp > 0 and math.isfinite(clamp)):
      raise _lib.WgError(f"clamp must be positive and finite, got {clamp}")
    if mel_bases is None:
      fmax = sampling_rate / 2.0 if fmax is None else float(fmax)
      banks = [slaney_mel_filterbank(sampling_rate, n, m, float(fmin), fmax) for n, m in zip(n_ffts, n_mels)]
    else:
      if len(mel_bases) != len(n_ffts):
        raise _lib.WgError(f"{len(mel_bases)} mel_bases for {len(n_ffts)} scales")
      banks = [np.ascontiguousarray(np.asarray(w), dtype=np.float32) for w in mel_bases]
    for w, n, m in zip(banks, n_ffts, n_mels):
      if w.shape != (m, n // 2 + 1):
        raise _lib.WgError(f"a mel basis of shape {w.shape} for n_fft {n}, n_mels {m}: expected {(m, n // 2 + 1)}")
      if not np.isfinite(w).all():
        raise _lib.WgError("a mel basis holds a non-finite value")
    self.scales = tuple(zip(n_ffts, hop_sizes, win_lengths, n_mels))
    self.mel_bases = banks
    self.factor_log, self.factor_lin, self.clamp = float(factor_log), float(factor_lin), clamp
    self.device = device
    self.lib = _lib.load()
    n = len(n_ffts)
    bases = [forward_basis(nf, w) for nf, _, w, _ in self.scales]
    arr = lambda v: (C.c_int32 * n)(*v)
    ptrs = lambda a: (C.c_void_p * n)(*[b.ctypes.data for b in a])
    self._owner = _args.Handle(self.lib, "wg_melloss_destroy")
    self._h = self._owner.value                # what every call takes; the owner releases it
    _lib.check(self.lib.wg_melloss_create(n, arr(n_ffts), arr(hop_sizes), arr(win_lengths), arr(n_mels), ptrs(bases),
                                          ptrs(banks), self.clamp, _lib.device_index(device), C.byref(self._h)))

  def workspace_bytes(self, B: int, N: int) -> int:
    """Bytes one forward with a graph keeps until its backward (0 when N <= max(n_ffts) / 2): per scale the prediction's
    (re, im) [B, n_fft, F] and both linear mels [B, n_mels, F] (F rounded up to 64), and the cell counts."""
    h = self._h
    return 4 * int(self.lib.wg_melloss_spectra_elems(h, B, N) + self.lib.wg_melloss_mels_elems(h, B, N))

  def _need(self):
    return max(s[0] for s in self.scales) // 2

  def _run(self, x, y, saved, lens=None):
    """One library call on contiguous fp32 [B, N]: (out3, (spectra, mels)), the last two None without saved state.
    lens: int32 [B] on the device, or None."""
    x, y = x.detach().contiguous(), y.detach().contiguous()
    B, N = x.shape
    h = self._h
    ns, nm = self.lib.wg_melloss_spectra_elems(h, B, N), self.lib.wg_melloss_mels_elems(h, B, N)
    if ns == 0 or nm == 0:
      raise _lib.WgError(f"MultiScaleMelLoss: unsupported batch {B} x {N}")
    out = torch.empty(3, dtype=torch.float32, device=x.device)
    spectra = torch.empty(ns, dtype=torch.float32, device=x.device) if saved else None
    mels = torch.empty(nm, dtype=torch.float32, device=x.device) if saved else None
    _lib.check(self.lib.wg_melloss_forward(h, _args.ptr(x), _args.ptr(y), _args.ptr(lens), self.factor_log,
                                           self.factor_lin, _args.ptr(out), _args.ptr(spectra), _args.ptr(mels), B, N,
                                           _args.stream(x.device)))
    return out, (spectra, mels)

  def _backward(self, state, g, lens, B, N):
    spectra, mels = state
    gx = torch.empty((B, N), dtype=torch.float32, device=mels.device)
    _lib.check(self.lib.wg_melloss_backward(self._h, _args.ptr(g), _args.ptr(lens), self.factor_log,
                                            self.factor_lin, _args.ptr(spectra), _args.ptr(mels), _args.ptr(gx), B, N,
                                            _args.stream(mels.device)))
    return gx
