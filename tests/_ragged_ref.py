"""fp64 yardstick of ``MultiResolutionSTFTLoss(audio, target, lengths=...)``: the loss of the cropped utterances with
their frames concatenated, built from the helpers of tests/test_stft_loss_cpu.py.

Per resolution every crop ``x[b:b+1, :lens[b]]`` is transformed on its own (``torch.stft`` reflects about the crop's own
last sample and gives ``lens[b] // hop + 1`` frames); the three sums -- ``(M(y) - M(x))^2``, ``M(y)^2`` and
``|log M(y) - log M(x)|`` -- run over all crops, and the last is divided by the summed element count ``K sum_b F_b``.
Differentiable in ``x``; the samples behind a length are never read, so their gradient is exactly 0.
"""
import functools

import torch

from test_stft_loss_cpu import DEFAULT_RES, audio, power_stft64, power_unfold

# (resolutions, N, lens): see tests/test_ragged_losses_cpu.py for what each exercises
CASES = [
  (DEFAULT_RES, 4099, (1025, 2500, 4099)),
  (((64, 7, 33),), 1000, (33, 450, 1000)),
  (((2048, 2048, 2048),), 6200, (1025, 4096, 6200)),
]
CASE_IDS = ["default", "fft64-hop7", "hop-is-fft"]


def inputs(N, lens, silent):
  B = len(lens)
  return audio(B, N, 100 + N, silent), audio(B, N, 150 + N, False)


def _ragged(power_fn, x, y, lens, resolutions, eps, factor_sc, factor_mag):
  assert x.shape == y.shape and len(lens) == x.shape[0]
  sc = mag = 0.0
  for n_fft, hop, win in resolutions:
    s0 = s1 = s2 = 0.0
    count = 0
    for b, n in enumerate(lens):
      px, py = power_fn(x[b:b + 1, :n], n_fft, hop, win), power_fn(y[b:b + 1, :n], n_fft, hop, win)
      assert px.shape[-1] == n // hop + 1
      mx, my = torch.clamp(px, min=eps).sqrt(), torch.clamp(py, min=eps).sqrt()
      s0 = s0 + ((my - mx) ** 2).sum()
      s1 = s1 + (my ** 2).sum()
      s2 = s2 + (my.log() - mx.log()).abs().sum()
      count += px.numel()
    sc = sc + s0.sqrt() / s1.sqrt()
    mag = mag + s2 / count
  sc, mag = sc / len(resolutions), mag / len(resolutions)
  return sc, mag, factor_sc * sc + factor_mag * mag


def ragged_ref64(x, y, lens, resolutions=DEFAULT_RES, eps=1e-7, factor_sc=1.0, factor_mag=1.0):
  """(sc, mag, loss) in float64 with torch.stft per crop; differentiable in x."""
  return _ragged(power_stft64, x.double(), y.double(), lens, resolutions, eps, factor_sc, factor_mag)


def ragged_unfold(x, y, lens, resolutions=DEFAULT_RES, eps=1e-7, factor_sc=1.0, factor_mag=1.0, dtype=torch.float64):
  """The same by pad + unfold + matmul with the library's fp32 basis per crop, computed in ``dtype``."""
  return _ragged(functools.partial(power_unfold, dtype=dtype), x, y, lens, resolutions, eps, factor_sc, factor_mag)


def ragged_grad64(x, y, lens, resolutions=DEFAULT_RES, eps=1e-7, factor_sc=1.0, factor_mag=1.0, fn=ragged_ref64):
  xg = x.detach().clone().requires_grad_(True)
  (g,) = torch.autograd.grad(fn(xg, y, lens, resolutions, eps, factor_sc, factor_mag)[2], xg)
  return g
