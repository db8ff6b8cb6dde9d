"""Bias-removal post-filter with the reference's surface (src/waveglow/denoiser.py:14-57), computed by the HIP
library (``wg_stft_*``: conv-STFT of src/waveglow/stft.py:98-198 as exact-fp32 MFMA GEMMs).

The Fourier / pseudo-inverse bases are built on the host exactly like ``STFT.__init__`` (stft.py:108-132) and handed
to the library once.  librosa's ``pad_center`` is restated (the reference imports it; librosa is absent here).  The
post-filter is pinned against ``oracle/stft_oracle.py`` (numpy fp64 restatement) and against outputs of the reference's own
``STFT`` and ``Denoiser`` classes, run with functional stand-ins for the librosa names (tests/golden/stft_ref.npz,
tests/test_gpu_stft_ref.py; ``stft_bases`` row by row in tests/test_stft_ref_cpu.py).  No torch/CPU fallback.

``Denoiser.forward_differentiable`` is ``forward`` with an autograd graph back to the audio (``wg_stft_denoise_forward_saved``
/ ``wg_stft_denoise_backward``), so that a waveform loss can be computed on the signal a listener hears.  The bias is a
constant of that graph; ``Denoiser.refresh_bias`` recomputes it after the vocoder's weights have moved.
"""
from __future__ import annotations

import ctypes as C
import math

import numpy as np
import torch
from scipy.signal import get_window

from . import _args, _lib

BIAS_MEL_LENGTH = 88   # denoiser.py:11


def stft_bases(filter_length=1024, hop_length=256, win_length=1024, window="hann"):
  """forward basis, inverse basis [2*(N/2+1), N] and squared window [N] (stft.py:108-132, :45-95)."""
  scale = filter_length / hop_length
  fb = np.fft.fft(np.eye(filter_length))
  cutoff = filter_length // 2 + 1
  fb = np.vstack([np.real(fb[:cutoff]), np.imag(fb[:cutoff])])
  inv = np.linalg.pinv(scale * fb).T
  win = get_window(window, win_length, fftbins=True)
  lpad = (filter_length - win_length) // 2
  win = np.pad(win, (lpad, filter_length - win_length - lpad))          # librosa.util.pad_center
  # C-contiguous copies: the pinv transpose is a Fortran-ordered view and the library reads raw row-major memory
  return (np.ascontiguousarray(fb * win, dtype=np.float32), np.ascontiguousarray(inv * win, dtype=np.float32),
          np.ascontiguousarray(win ** 2, dtype=np.float32))


def stft_handle(lib, hparams, device, window="hann") -> _args.Handle:
  """The ``wg_stft`` handle of ``stft_bases(hparams.filter_length, hparams.hop_length, hparams.win_length, window)`` on
  ``device``, with its owner: what the denoiser and the mel front-end both run on."""
  fwd, inv, wsq = stft_bases(hparams.filter_length, hparams.hop_length, hparams.win_length, window)
  h = _args.Handle(lib, "wg_stft_destroy")
  _lib.check(lib.wg_stft_create(fwd.ctypes.data, inv.ctypes.data, wsq.ctypes.data, hparams.filter_length,
                                hparams.hop_length, _lib.device_index(device), C.byref(h.value)))
  return h


class _DenoiseFn(torch.autograd.Function):
  """Inputs: the Denoiser, the audio [B, N], the strength, the device copy of the lengths (int32 [B]) or None, and the
  phase mode.  The forward keeps the library's workspace (the raw spectrum) and a private copy of the bias on ctx; the
  backward writes its d (re, im) to another part of that workspace, so the saved state survives and a second backward
  under retain_graph gives the same gradient."""

  @staticmethod
  def forward(ctx, den, audio, strength, lens, phase_grad):
    audio = audio.contiguous()
    B, N = audio.shape
    h = den._h
    ws = _args.workspace(den.lib.wg_stft_denoise_grad_workspace_bytes(h, B, N), audio.device,
                         f"denoiser: audio length {N} (multiple of 256, >= 1024)")
    bias = den.bias_spec.detach().reshape(-1).clone()          # refresh_bias writes bias_spec in place
    out = torch.empty_like(audio)
    _lib.check(den.lib.wg_stft_denoise_forward_saved(h, _args.ptr(audio), _args.ptr(lens), _args.ptr(bias), strength,
                                                     _args.ptr(out), B, N, _args.ptr(ws), ws.numel(),
                                                     _args.stream(audio.device)))
    ctx.den, ctx.ws, ctx.bias, ctx.lens = den, ws, bias, lens
    ctx.args = (B, N, strength, 1 if phase_grad else 0)
    return out[:, None, :]

  @staticmethod
  @torch.autograd.function.once_differentiable
  def backward(ctx, g_out):
    den, ws = ctx.den, ctx.ws
    B, N, strength, phase_grad = ctx.args
    g = g_out.to(torch.float32).reshape(B, N).contiguous()
    gx = torch.empty((B, N), dtype=torch.float32, device=ws.device)
    _lib.check(den.lib.wg_stft_denoise_backward(den._h, _args.ptr(g), _args.ptr(ctx.lens), _args.ptr(ctx.bias),
                                                strength, phase_grad, _args.ptr(gx), B, N, _args.ptr(ws), ws.numel(),
                                                _args.stream(ws.device)))
    return None, gx, None, None, None


class Denoiser(torch.nn.Module):
  """Removes model bias from audio produced with waveglow (denoiser.py:14-57)."""

  def __init__(self, waveglow, hparams, mode: str, device):
    super().__init__()
    device = torch.device(device)
    if device.type != "cuda":
      raise _lib.WgError("the denoiser runs on the GPU library only")
    self.lib = _lib.load()
    self._owner = stft_handle(self.lib, hparams, device)
    self._h = self._owner.value                # what every call takes; the owner releases it
    self.device = device
    self._n_mel, self._n_bins = hparams.n_mel_channels, hparams.filter_length // 2 + 1
    self.register_buffer("bias_spec", self._bias(waveglow, mode))      # [1, 513, 1] like bias_spec[:, :, 0][:, :, None]

  def _bias(self, waveglow, mode: str):
    """denoiser.py:38-49: |STFT| of frame 0 of what ``waveglow`` makes of an empty (or random) mel at sigma 0."""
    w = waveglow.upsample.weight
    if mode == "zeros":
      mel = torch.zeros((1, self._n_mel, BIAS_MEL_LENGTH), dtype=w.dtype, device=w.device)
    elif mode == "normal":
      mel = torch.randn((1, self._n_mel, BIAS_MEL_LENGTH), dtype=w.dtype, device=w.device)
    else:
      raise Exception(f"Mode {mode} if not supported")
    with torch.no_grad():
      bias_audio = waveglow.infer(mel, sigma=0.0).float()              # denoiser.py:45-47 (the HIP hot path)
      mag0 = torch.empty((1, self._n_bins), dtype=torch.float32, device=bias_audio.device)
      self._run(bias_audio, None, 0.0, None, mag0)
    return mag0[:, :, None]

  def refresh_bias(self, waveglow, mode: str = "zeros"):
    """Recomputes ``bias_spec`` in place from ``waveglow``'s CURRENT weights, exactly as ``__init__`` computed it, under
    no-grad.  The bias is measured once at construction; after the vocoder has been fine-tuned (``weight_grads=True``)
    it describes weights that no longer exist until this is called.  ``waveglow.infer`` after a weight change pays the
    engine's re-finalisation of the weights.  Graphs of earlier ``forward_differentiable`` calls keep the bias they were
    built with.  Returns ``bias_spec``."""
    new = self._bias(waveglow, mode)
    with torch.no_grad():
      self.bias_spec.copy_(new.to(self.bias_spec.device))
    return self.bias_spec

  def _run(self, audio, bias, strength, out, mag0, lengths_dev=None):
    """The one wg_stft_denoise call: fp32 ``audio`` [B, N], ``lengths_dev`` int32 [B] on the device or None."""
    audio = audio.contiguous()
    B, N = audio.shape
    ws = _args.workspace(self.lib.wg_stft_workspace_bytes(self._h, B, N), audio.device,
                         f"denoiser: audio length {N} (multiple of 256, >= 1024)")
    _lib.check(self.lib.wg_stft_denoise(self._h, _args.ptr(audio), _args.ptr(lengths_dev), _args.ptr(bias),
                                        float(strength), _args.ptr(out), _args.ptr(mag0), B, N, _args.ptr(ws), ws.numel(),
                                        _args.stream(audio.device)))

  def _lens(self, lengths, audio, device, allow_device=True):
    """The one length check of the denoiser: B multiples of 256 in [1024, N] (``_args.counts``), as int32 on ``device``."""
    B, N = audio.shape
    return _args.counts("denoiser: lengths", lengths, B, 1024, N, device=device, multiple_of=256,
                        allow_device=allow_device)[0]

  def forward(self, audio: torch.Tensor, strength: float, lengths=None):
    """denoiser.py:51-57; returns [B, 1, N] like the reference's conv_transpose1d output.

    ``lengths`` (B sample counts, see ``forward_differentiable``) makes the rows of ``audio`` [B, N] utterances of
    different lengths, denoised in ONE call: utterance b comes out bit for bit as ``forward(audio[b:b+1, :lengths[b]])``
    gives it, with zeros behind it.  Every length is a multiple of 256 in [1024, N], as for the call without lengths."""
    audio = audio.float()
    out = torch.empty_like(audio)
    lens = None if lengths is None else self._lens(lengths, audio, audio.device)
    self._run(audio, self.bias_spec.reshape(-1).contiguous(), strength, out, None, lens)
    return out[:, None, :]

  def grad_workspace_bytes(self, B: int, N: int) -> int:
    """Bytes of device memory a ``forward_differentiable`` of audio [B, N] keeps alive until its backward has run (the
    library's workspace; 513 more floats hold the bias).  0 for a shape the denoiser does not take."""
    return int(self.lib.wg_stft_denoise_grad_workspace_bytes(self._h, int(B), int(N)))

  def forward_differentiable(self, audio: torch.Tensor, strength: float, lengths=None, phase_grad: bool = True):
    """``forward(audio, strength, lengths)`` with an autograd graph back to ``audio``: [B, N] fp32 on the module's device
    -> [B, 1, N], ``torch.equal`` to ``forward``.  Enqueued on the current stream, nothing synchronised.

    ``phase_grad=True``: the backward is the derivative of what the forward computes, ``max(|X| - c, 0) X / |X|`` with
    ``c = strength * bias_spec`` per bin.  ``phase_grad=False``: the gradient the reference's own autograd gives, whose
    ``STFT.transform`` detaches the phase (stft.py:160-161), so only the path through ``|X|`` is followed.  Both are 0
    where ``|X| == 0`` (the reference gives NaN there) and where ``|X| - c < 0``.

    ``lengths``: B integers as ``_args.counts`` takes them (a list, a tuple or a 1-D CPU tensor of an integer dtype; a
    float or a bool entry raises WgError), or an int32 tensor ``[B]`` on the device, which is trusted and never read on
    the host (a count outside the limits zeroes that row's output and gradient): the sample counts of a padded batch,
    multiples of 256 in [1024, N], uploaded in one small copy.  ``audio.grad[b, :lengths[b]]`` has the bits of the
    backward of that utterance alone, ``audio.grad[b, lengths[b]:]`` is 0; audio and incoming gradient behind a length
    are never read.

    ``strength`` and ``bias_spec`` are constants of the graph (no gradient; no graph from the bias to the vocoder's
    weights).  Without grad mode, or when ``audio`` does not require grad, this is ``forward`` and nothing is saved.  No
    CPU fallback and no double backward; other devices, dtypes, ranks and a non-finite strength raise WgError."""
    _args.tensor("forward_differentiable: audio", audio, device=self.device, ndim=2)
    strength = float(strength)
    if not math.isfinite(strength):
      raise _lib.WgError(f"forward_differentiable: strength must be finite, got {strength}")
    B, N = audio.shape
    if self.grad_workspace_bytes(B, N) == 0:
      raise _lib.WgError(f"denoiser: unsupported audio length {N} (multiple of 256, >= 1024)")
    lens = None if lengths is None else self._lens(lengths, audio, audio.device)
    if torch.is_grad_enabled() and audio.requires_grad:
      return _DenoiseFn.apply(self, audio, strength, lens, bool(phase_grad))
    out = torch.empty_like(audio, memory_format=torch.contiguous_format)
    self._run(audio.detach(), self.bias_spec.reshape(-1).contiguous(), strength, out, None, lens)
    return out[:, None, :]

  def run_ragged(self, audio, lengths, lengths_dev, strength, out):
    """One wg_stft_denoise call with lengths on fp32 ``audio`` [B, N] into ``out``; ``lengths`` is checked here on the host,
    ``lengths_dev`` is the same as an int32 tensor on the device (the library never reads it on the host)."""
    self._lens(lengths, audio, None, allow_device=False)
    self._run(audio, self.bias_spec, strength, out, None, lengths_dev)
