"""The torch fp64 restatement of steps 1 - 6 of the intelligibility metrics (include/waveglow_amd.h: wg_stoi) that CPU
autograd differentiates with respect to the processed signal ``y``: the yardstick of ``wg_stoi_backward``.  The conventions
at the points where the definition is not smooth are the header's: ``sqrt0`` has gradient 0 where its argument is exactly
0, the clip is ``torch.where(a <= c, a, c)`` (a tie goes to the ``alpha y`` branch, as ``torch.where`` routes it), ``alpha``
is differentiated, the gate and ``x`` are constants (the gate is taken from tests/_stoi_oracle.py itself).

Two DFT forms: ``torch.fft.rfft`` and a direct product with the 512-entry cos / sin table over bins 7 .. 218, which is what
the kernels compute; the distance of their gradients is the rounding yardstick of the device bar.

Also the numpy restatement of the transposed resampler (include/waveglow_amd.h: wg_resample_backward)."""
import functools

import numpy as np
import torch

import _resample_oracle
import _stoi_oracle as oracle

W, H, NFFT, N, BANDS = oracle.W, oracle.H, oracle.NFFT, oracle.N, oracle.BANDS
EPS = oracle.EPS
CLIP = 1.0 + 10.0 ** (-oracle.BETA / 20.0)


class _Sqrt0(torch.autograd.Function):
  @staticmethod
  def forward(ctx, v):
    r = torch.sqrt(v)
    ctx.save_for_backward(r)
    return r

  @staticmethod
  def backward(ctx, g):
    r, = ctx.saved_tensors
    return torch.where(r > 0, g / (2 * torch.where(r > 0, r, torch.ones_like(r))), torch.zeros_like(g))


sqrt0 = _Sqrt0.apply


@functools.lru_cache(maxsize=None)
def _tables():
  ang = 2.0 * np.pi * np.arange(NFFT, dtype=np.float64) / NFFT
  cos, sin = np.cos(ang), np.sin(ang)                                           # the 512 entries the device is handed
  k = np.arange(oracle.BIN_LO, oracle.BIN_HI)[:, None]
  j = np.arange(W)[None, :]
  idx = (k * j) % NFFT
  return torch.from_numpy(cos[idx]), torch.from_numpy(sin[idx])                 # [212, 256]


def _frames(s, count, w):
  idx = (torch.arange(count) * H)[:, None] + torch.arange(W)[None, :]
  return w * s[idx]


def _spectra(s, frames, w, dft):
  """X [15, frames] of the silence-free signal s."""
  f = _frames(s, frames, w)
  if dft == "rfft":
    z = torch.fft.rfft(f, n=NFFT, dim=1)
    p = z.real ** 2 + z.imag ** 2
    lo0 = 0
  else:
    cos, sin = _tables()
    re, im = f @ cos.T, f @ sin.T
    p = re * re + im * im
    lo0 = oracle.BIN_LO
  return torch.stack([sqrt0(p[:, lo - lo0:hi - lo0].sum(dim=1)) for lo, hi in oracle.band_table().tolist()])


def _normalise(a, dim):
  a = a - a.mean(dim=dim, keepdim=True)
  return a / (sqrt0((a * a).sum(dim=dim, keepdim=True)) + EPS)


def scores(x, y, dft="rfft"):
  """(stoi, estoi, info): fp64 0-dim tensors with a graph to ``y`` (a 1-D fp64 torch tensor); ``x`` is a constant (numpy or
  torch).  NaN twice without a segment.  info = {"frames", "frames_kept", "segments", "margin"} as _stoi_oracle.stoi, and "clipped",
  the number of (segment, band, frame) entries where the clip branch wins."""
  x = torch.as_tensor(np.asarray(x, dtype=np.float64))
  n = min(len(x), len(y))
  x, y = x[:n], y[:n]
  w_np = oracle.window()
  w = torch.from_numpy(w_np)
  F0 = oracle.frame_count(n)
  info = {"frames": F0, "frames_kept": 0, "segments": 0, "margin": float("inf")}
  nan = torch.tensor(float("nan"), dtype=torch.float64)
  if F0 == 0:
    return nan, nan, info
  xf_np = oracle._frames(x.numpy(), w_np)                                      # the gate, value for value the oracle's
  e = 20 * np.log10(np.sqrt(np.sum(xf_np * xf_np, axis=1)) + EPS)
  gap = (np.max(e) - oracle.DYN_RANGE) - e
  mask = torch.from_numpy(gap < 0)
  K = int(mask.sum())
  info.update(frames_kept=K, margin=float(np.min(np.abs(gap))))
  F = K - 1
  J = max(F - (N - 1), 0)
  info["segments"] = J
  if J == 0:
    return nan, nan, info

  def silence_free(s):
    kept = _frames(s, F0, w)[mask]                                              # [K, 256]
    idx = (torch.arange(K) * H)[:, None] + torch.arange(W)[None, :]
    return torch.zeros((K - 1) * H + W, dtype=torch.float64).index_add(0, idx.reshape(-1), kept.reshape(-1))

  X = _spectra(silence_free(x), F, w, dft)                                      # [15, F]
  Y = _spectra(silence_free(y), F, w, dft)
  xs = X.unfold(1, N, 1).permute(1, 0, 2)                                       # [J, 15, 30]
  ys = Y.unfold(1, N, 1).permute(1, 0, 2)
  norm = lambda a: sqrt0((a * a).sum(dim=2, keepdim=True))
  alpha = norm(xs) / (norm(ys) + EPS)
  a, c = alpha * ys, xs * CLIP
  yp = torch.where(a <= c, a, c)
  info["clipped"] = int((a > c).sum())
  d = (_normalise(xs, 2) * _normalise(yp, 2)).sum() / (BANDS * J)
  xn = _normalise(_normalise(xs, 2), 1)
  yn = _normalise(_normalise(ys, 2), 1)
  est = (xn * yn / N).sum() / J
  return d, est, info


def gradient(x, y, g_stoi=1.0, g_estoi=0.0, dft="rfft"):
  """(d_y fp64 numpy [len(y)], stoi, estoi, info): CPU autograd of g_stoi STOI + g_estoi ESTOI with respect to ``y``; all
  zeros without a segment."""
  yt = torch.tensor(np.asarray(y, dtype=np.float64), requires_grad=True)
  d, e, info = scores(x, yt, dft)
  if info["segments"] == 0:
    return np.zeros(len(yt)), float("nan"), float("nan"), info
  (g_stoi * d + g_estoi * e).backward()
  return yt.grad.numpy().copy(), d.item(), e.item(), info


# ------------------------------------------------------------------------------------------------ transposed resampler
def plan(up: int, down: int):
  """(half, h): scipy's default filter of the reduced ratio; (0, [1.0]) for the copy."""
  if up == down == 1:
    return 0, np.ones(1)
  return _resample_oracle.taps(up, down)


def resample_forward(x, up: int, down: int) -> np.ndarray:
  """fp64 closed form of the resampler for one utterance (the copy included)."""
  if up == down == 1:
    return np.asarray(x, dtype=np.float64).copy()
  return _resample_oracle.resample(x, up, down)


def resample_backward(g, n_in: int, up: int, down: int) -> np.ndarray:
  """fp64 [n_in]: d_in[m] = sum_n g[n] h[half + n down - m up] over 0 <= n < out_len(n_in) with the tap index inside
  [0, 2 half]; ``g`` holds at least out_len(n_in) values and nothing behind them is read."""
  half, h = plan(up, down)
  olen = _resample_oracle.out_len(n_in, up, down)
  g = np.asarray(g, dtype=np.float64)
  d = np.zeros(n_in)
  for m in range(n_in):
    c = half - m * up
    n_lo = max(0, -(c // down))                                                # ceil(-c / down)
    n_hi = min(olen - 1, (2 * half - c) // down)
    if n_hi >= n_lo:
      n = np.arange(n_lo, n_hi + 1)
      d[m] = np.dot(g[n], h[c + n * down])
  return d
