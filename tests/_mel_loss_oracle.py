"""Yardsticks of MultiScaleMelLoss, shared by tests/test_mel_loss_cpu.py and tests/test_gpu_mel_loss.py.

Two independent restatements of the loss (waveglow_amd/mel_loss.py has the definition):
  (a) ``loss_stft``    ``torch.stft`` in fp64 under autograd on the CPU
  (b) ``loss_unfold``  reflect padding + ``unfold`` + a matmul with the windowed Fourier basis the library packs
                       (``stft_loss.forward_basis``), in fp64 or in fp32
Both take the fp32 bank cast up, and both take ``lengths`` by cropping: utterance b is ``x[b, :lengths[b]]``, the means
run over the cells of all crops.  Both follow the library's gradient conventions: ``sign(0) = 0`` (``abs``), no
gradient of the log term under the clamp (``clamp``), and a zero gradient for a bin with ``re^2 + im^2 = 0`` (``_root``).

``fragile_cells`` counts the mel cells whose sign or clamp an fp32 computation may flip; tests that bound a gradient in L2
require it to be 0 for their inputs.  It is computed from (a) alone.
"""
import functools

import torch
import torch.nn.functional as Fn

from waveglow_amd.stft_loss import forward_basis
from waveglow_amd.taco_stft import slaney_mel_filterbank

SR = 22050
CLAMP = 1e-5
# (n_fft, hop, win, n_mels): small; one tile; hop not dividing n_fft and win < n_fft; the model's geometry; the largest
SCALES = ((64, 16, 64, 10), (256, 64, 256, 40), (512, 120, 400, 64), (1024, 256, 1024, 80), (2048, 512, 2048, 320))
EMPTY_ROWS = (256, 64, 256, 80)          # 80 mels over 129 bins: some filters hold no bin
SHAPES = [(1, 1025), (2, 2048), (3, 4096), (2, 16000)]


def scales_for(N, scales=SCALES):
  """The scales a batch of N samples can take: reflect padding needs N > n_fft / 2."""
  return tuple(s for s in scales if s[0] // 2 < N)


@functools.lru_cache(maxsize=None)
def bank(scale, fmin=0.0, fmax=None):
  n_fft, _, _, n_mels = scale
  return torch.from_numpy(slaney_mel_filterbank(SR, n_fft, n_mels, fmin, SR / 2.0 if fmax is None else fmax))


@functools.lru_cache(maxsize=None)
def _basis(n_fft, win):
  return torch.from_numpy(forward_basis(n_fft, win))


def _root(p):
  """sqrt(p) with a zero gradient where p = 0."""
  pos = p > 0
  return torch.where(pos, torch.where(pos, p, torch.ones_like(p)).sqrt(), torch.zeros_like(p))


def spec_stft(x, n_fft, hop, win, dtype):
  """(a)'s complex transform as (re, im), each [B, K, F]."""
  x = x.to(dtype)
  X = torch.stft(x, n_fft, hop, win, torch.hann_window(win, dtype=dtype), center=True, pad_mode="reflect",
                 return_complex=True)
  return X.real, X.imag


def frames_unfold(x, n_fft, hop, dtype):
  """The reflect-padded frames of (b): [B, F, n_fft]."""
  xp = Fn.pad(x.to(dtype)[:, None, :], (n_fft // 2, n_fft // 2), mode="reflect")[:, 0]
  return xp.unfold(1, n_fft, hop)


def spec_of_frames(fr, n_fft, win):
  """(b)'s transform of frames [B, F, n_fft] with the library's fp32 basis in the frames' dtype: (re, im), each [B, K, F]."""
  X = torch.matmul(fr, _basis(n_fft, win).to(fr.dtype).t())            # [B, F, 2K]
  K = n_fft // 2 + 1
  return X[..., :K].transpose(1, 2), X[..., K:].transpose(1, 2)


def spec_unfold(x, n_fft, hop, win, dtype):
  return spec_of_frames(frames_unfold(x, n_fft, hop, dtype), n_fft, win)


def mag_stft(x, n_fft, hop, win, dtype):
  re, im = spec_stft(x, n_fft, hop, win, dtype)
  return _root(re ** 2 + im ** 2)                                     # [B, K, F]


def mag_unfold(x, n_fft, hop, win, dtype):
  re, im = spec_unfold(x, n_fft, hop, win, dtype)
  return _root(re ** 2 + im ** 2)


def mels(mag_fn, x, scale, W, lengths, dtype):
  """Linear mels of the crops, frames concatenated: [n_mels, sum_b F_b]."""
  n_fft, hop, win, _ = scale
  B, N = x.shape
  lens = [N] * B if lengths is None else lengths
  W = W.to(dtype)
  return torch.cat([W @ mag_fn(x[b:b + 1, :n], n_fft, hop, win, dtype)[0] for b, n in enumerate(lens)], dim=1)


def _loss(mag_fn, x, y, scales, banks, clamp, factor_log, factor_lin, lengths, dtype):
  banks = [bank(s) for s in scales] if banks is None else banks
  log = lin = 0.0
  for s, W in zip(scales, banks):
    mx, my = mels(mag_fn, x, s, W, lengths, dtype), mels(mag_fn, y, s, W, lengths, dtype)
    log = log + (torch.clamp(mx, min=clamp).log() - torch.clamp(my, min=clamp).log()).abs().mean()
    lin = lin + (mx - my).abs().mean()
  log, lin = log / len(scales), lin / len(scales)
  return log, lin, factor_log * log + factor_lin * lin


def loss_stft(x, y, scales, banks=None, clamp=CLAMP, factor_log=1.0, factor_lin=0.0, lengths=None):
  """(a): (log, lin, loss) in fp64 with torch.stft; differentiable in x."""
  return _loss(mag_stft, x, y, scales, banks, clamp, factor_log, factor_lin, lengths, torch.float64)


def loss_unfold(x, y, scales, banks=None, clamp=CLAMP, factor_log=1.0, factor_lin=0.0, lengths=None,
                dtype=torch.float64):
  """(b): the same by pad + unfold + matmul with the library's fp32 basis, computed in ``dtype``."""
  return _loss(mag_unfold, x, y, scales, banks, clamp, factor_log, factor_lin, lengths, dtype)


def grad_of(fn, x, y, scales, **kw):
  xg = x.detach().clone().requires_grad_(True)
  (g,) = torch.autograd.grad(fn(xg, y, scales, **kw)[2], xg)
  return g


def fragile_cells(x, y, scales, tau=1e-4, banks=None, clamp=CLAMP, lengths=None, frames=None, margin=None):
  """The number of mel cells with |lmel(x) - lmel(y)| < tau or |mel(x) - clamp| < tau clamp, from (a) alone.  A cell
  where both log-mels are exactly equal (a silent stretch in both signals) is as fragile as any other: inputs that must
  qualify have none.  ``frames``: None, or ``frames[i][b]`` the frame indices of scale i and utterance b to which the
  count is restricted (where prediction and target are equal by construction everywhere else, tests/_loss_cells.py).
  ``margin``: None, or per scale an absolute distance that takes the place of ``tau``: a cell then counts when
  |mel(x) - mel(y)| < margin or |mel(x) - clamp| < margin, i.e. when two mels that are each off by less than margin / 2
  can exchange their order or cross the clamp."""
  banks = [bank(s) for s in scales] if banks is None else banks
  B, N = x.shape
  lens = [N] * B if lengths is None else lengths
  bad = 0
  for i, (s, W) in enumerate(zip(scales, banks)):
    for b, n in enumerate(lens):
      mx = mels(mag_stft, x[b:b + 1, :n], s, W, None, torch.float64)
      my = mels(mag_stft, y[b:b + 1, :n], s, W, None, torch.float64)
      if frames is not None:
        mx, my = mx[:, frames[i][b]], my[:, frames[i][b]]
      if margin is not None:
        bad += int((((mx - my).abs() < margin[i]) | ((mx - clamp).abs() < margin[i])).sum())
        continue
      d = torch.clamp(mx, min=clamp).log() - torch.clamp(my, min=clamp).log()
      bad += int(((d.abs() < tau) | ((mx - clamp).abs() < tau * clamp)).sum())
  return bad


def rel(a, b):
  return float((a.double() - b.double()).norm() / b.double().norm())


DENSE_SCALE = (256, 64, 256, 12)


def dense_bank():
  """A bank [12, 129] that is no triangular one: rows that overlap widely, a row of zeros, negative entries, zeros inside a
  span."""
  gen = torch.Generator().manual_seed(5)
  W = torch.rand(12, 129, generator=gen) * 0.1
  W[:, 1::7] = 0.0
  W[3] = 0.0
  W[5, :100] = 0.0
  W[7, 40:] = 0.0
  W[9] -= 0.02
  return W


def noise(B, N, seed):
  """Uniform noise under a slow envelope (``audio`` of tests/test_stft_loss_cpu.py without its silent stretch)."""
  gen = torch.Generator().manual_seed(seed)
  return (torch.rand(B, N, generator=gen) * 1.6 - 0.8) * torch.linspace(0.3, 1.0, N)[None, :]


def inputs(B, N, seed, silent=True):
  """A prediction and a target whose log-mels stay apart: the target is the prediction at half the level in the first
  half and at twice the level in the second (both signs of the difference occur), plus noise of its own; with ``silent``
  the prediction has a silent stretch, whose cells lie under the clamp while the target's do not."""
  x = noise(B, N, seed)
  gain = torch.where(torch.arange(N) < N // 2, 0.5, 2.0)[None, :]
  y = gain * x + 0.1 * noise(B, N, seed + 50)
  if silent:
    x = x.clone()
    a, n = (N // 4, 2600) if N >= 8000 else (N // 5, N // 3)
    x[:, a:a + n] = 0.0
  return x, y


# Seeds of ``inputs`` at which (a) finds no fragile cell, dense and at RAGGED's lengths, found by trying 0, 1, ... on the
# CPU; tests/test_mel_loss_cpu.py asserts it.
SEEDS = {(1, 1025): 0, (2, 2048): 0, (3, 4096): 0, (2, 16000): 4}

# shape -> lengths: one just above max n_fft / 2 of the shape's scales, one that no hop divides, one equal to N
RAGGED = {(3, 4096): [1025, 3001, 4096]}
