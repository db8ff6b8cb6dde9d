"""Soft dynamic time warping as a training loss (``wg_softdtw_forward`` / ``wg_softdtw_backward``): the warped distance that
``validate`` reports as "MFCC DTW MCD" (``metrics.dtw_distance``), smoothed so that it has a gradient (Cuturi and Blondel,
"Soft-DTW: a differentiable loss function for time-series", ICML 2017).  It compares a generated mel of ``Ta`` frames with a
recording of ``Tb`` frames, which the frame-by-frame losses (``MultiResolutionSTFTLoss``, ``STOILoss``, a mel L1) cannot.

One forward is one launch, a wavefront over the anti-diagonals that keeps the accumulated-cost matrix R; one backward is a
second wavefront that gives the expected alignment E and one launch per feature gradient.  The definition is stated in
include/waveglow_amd.h and DESIGN.md section 7.  No torch / CPU fallback.

  loss = mean_b value_b / ((Ta_b + Tb_b) / 2)          over the utterances with valid frame counts
"""
from __future__ import annotations

import math

import torch

from . import _args, _lib, metrics
from ._args import ptr

COSTS = {"l2": _lib.WG_SDTW_L2, "sq": _lib.WG_SDTW_SQ}
FEATURES = ("mfcc", "mel")


def _gamma(gamma) -> float:
  try:
    g = float(gamma)
  except (TypeError, ValueError):
    raise _lib.WgError(f"soft_dtw: gamma must be a number, got {gamma!r}")
  if not (g > 0.0 and math.isfinite(g)):
    raise _lib.WgError(f"soft_dtw: gamma must be positive and finite, got {gamma!r}")
  return g


def _cost(cost) -> int:
  if cost not in COSTS:
    raise _lib.WgError(f"soft_dtw: cost must be one of {sorted(COSTS)}, got {cost!r}")
  return COSTS[cost]


def _check(feat_a, frames_a, feat_b, frames_b, gamma, cost):
  """Every refusal, before any launch: (a, fa, b, fb, gamma, cost id) with contiguous features and device counts."""
  g, c = _gamma(gamma), _cost(cost)
  a = metrics._features("soft_dtw: feat_a", feat_a)
  b = metrics._features("soft_dtw: feat_b", feat_b, a.device)
  if a.shape[0] != b.shape[0] or a.shape[1] != b.shape[1]:
    raise _lib.WgError(f"soft_dtw: batch and feature sizes differ, {tuple(a.shape)} against {tuple(b.shape)}")
  fa = metrics._frames("soft_dtw: frames_a", frames_a, a, upload=False)
  fb = metrics._frames("soft_dtw: frames_b", frames_b, b, upload=False)
  return a, fa.to(a.device), b, fb.to(b.device), g, c


def r_bytes(B: int, Ta: int, Tb: int) -> int:
  """Bytes of the accumulated-cost matrix one forward with a graph keeps (``wg_softdtw_bytes``; 0 outside the limits)."""
  return int(_lib.load().wg_softdtw_bytes(int(B), int(Ta), int(Tb)))


def _forward(a, fa, b, fb, gamma, cost, keep_r):
  B, K, Ta = a.shape
  Tb = b.shape[2]
  lib = _lib.load()
  with torch.cuda.device(a.device):
    value = torch.empty(B, dtype=torch.float64, device=a.device)
    r = torch.empty(lib.wg_softdtw_bytes(B, Ta, Tb) // 8, dtype=torch.float64, device=a.device) if keep_r else None
    _lib.check(lib.wg_softdtw_forward(ptr(a), ptr(fa), ptr(b), ptr(fb), gamma, cost, ptr(value), ptr(r), B, K, Ta, Tb,
                                      _args.stream(a.device)))
  return value, r


def _backward(a, fa, b, fb, gamma, cost, r, g_value, want_e, want_a, want_b):
  """(E or None, g_a or None, g_b or None).  The gradients need E: it is a temporary here when the caller does not want it."""
  B, K, Ta = a.shape
  Tb = b.shape[2]
  lib = _lib.load()
  with torch.cuda.device(a.device):
    e = torch.empty((B, Ta, Tb), dtype=torch.float64, device=a.device)
    g_a = torch.empty((B, K, Ta), dtype=torch.float32, device=a.device) if want_a else None
    g_b = torch.empty((B, K, Tb), dtype=torch.float32, device=a.device) if want_b else None
    _lib.check(lib.wg_softdtw_backward(ptr(a), ptr(fa), ptr(b), ptr(fb), gamma, cost, ptr(r), ptr(g_value), ptr(e),
                                       ptr(g_a), ptr(g_b), B, K, Ta, Tb, _args.stream(a.device)))
  return (e if want_e else None), g_a, g_b


class _SoftDtwFn(torch.autograd.Function):
  """(feat_a, frames_a, feat_b, frames_b, gamma, cost id) -> fp64 [B].  The forward keeps the features as the kernels read
  them, the counts and R; the backward allocates its own outputs, so a second backward under retain_graph gives the same
  bits."""

  @staticmethod
  def forward(ctx, feat_a, fa, feat_b, fb, gamma, cost):
    a, b = feat_a.detach().contiguous(), feat_b.detach().contiguous()
    value, r = _forward(a, fa, b, fb, gamma, cost, True)
    ctx.state = (a, fa, b, fb, gamma, cost, r)
    return value

  @staticmethod
  @torch.autograd.function.once_differentiable
  def backward(ctx, g):
    a, fa, b, fb, gamma, cost, r = ctx.state
    want_a, want_b = ctx.needs_input_grad[0], ctx.needs_input_grad[2]
    _, g_a, g_b = _backward(a, fa, b, fb, gamma, cost, r, g.to(torch.float64).contiguous(), False, want_a, want_b)
    return g_a, None, g_b, None, None, None


def soft_dtw(feat_a: torch.Tensor, frames_a, feat_b: torch.Tensor, frames_b, gamma: float = 1.0,
             cost: str = "l2") -> torch.Tensor:
  """fp64 ``[B]`` on the device: the soft-DTW value of the columns of ``feat_a`` [B, K, Ta] against those of ``feat_b``
  [B, K, Tb] (fp32 on one GPU, K <= 128, T <= 4096) with ``frames_a[b]`` / ``frames_b[b]`` frames each, and a graph to
  whichever of the two requires grad; the same tensor may stand on both sides.  ``cost``: "l2", the Euclidean frame
  distance of ``metrics.dtw_distance`` (the value tends to its cost as gamma -> 0), or "sq", its square.  Frame counts:
  None (all), or B integers as ``_args.counts`` takes them (a list, a tuple or a 1-D CPU tensor of an integer dtype; a
  float or a bool entry raises WgError), each in ``[1, T]`` (checked before any launch), or an int32 tensor ``[B]`` on
  the device, which is trusted and never read on the host: a count outside the limits there gives a NaN value and zero
  gradients for that utterance. Nothing behind a count is read.  Gradients are computed in fp64 and rounded to fp32
  once.  Without grad mode, or when nothing requires grad, only the values are computed: no R is kept and nothing is
  saved.  Enqueue-only; bit-reproducible; no double backward."""
  a, fa, b, fb, g, c = _check(feat_a, frames_a, feat_b, frames_b, gamma, cost)
  if torch.is_grad_enabled() and (feat_a.requires_grad or feat_b.requires_grad):
    return _SoftDtwFn.apply(feat_a, fa, feat_b, fb, g, c)
  return _forward(a, fa, b, fb, g, c, False)[0]


def soft_dtw_alignment(feat_a: torch.Tensor, frames_a, feat_b: torch.Tensor, frames_b, gamma: float = 1.0,
                       cost: str = "l2"):
  """``(values fp64 [B], E fp64 [B, Ta, Tb])`` without a graph: E(i, j) is the expected alignment, the weight of cell (i, j)
  over all warping paths under the Gibbs distribution of temperature gamma; E(0, 0) = E(Ta-1, Tb-1) = 1, exact zeros behind
  an utterance's frames.  Arguments as ``soft_dtw``."""
  a, fa, b, fb, g, c = _check(feat_a, frames_a, feat_b, frames_b, gamma, cost)
  a, b = a.detach(), b.detach()
  value, r = _forward(a, fa, b, fb, g, c, True)
  e, _, _ = _backward(a, fa, b, fb, g, c, r, None, True, False, False)
  return value, e


def dct_basis(n_mel: int, n_mfcc: int) -> torch.Tensor:
  """fp64 ``[n_mfcc, n_mel]`` on the host: row k-1 = sqrt(2/N) cos(pi k (2n+1) / (2N)), k = 1..n_mfcc -- coefficients
  1 .. n_mfcc of the orthonormal DCT-II, the basis of ``wg_metrics_mfcc``."""
  k = torch.arange(1, n_mfcc + 1, dtype=torch.float64)[:, None]
  n = torch.arange(n_mel, dtype=torch.float64)[None, :]
  return math.sqrt(2.0 / n_mel) * torch.cos(math.pi * k * (2 * n + 1) / (2 * n_mel))


class SoftDTWLoss(torch.nn.Module):
  """``crit(mel_hat, frames_hat, mel_ref, frames_ref)`` -> 0-dim fp32 loss on the device with a graph to whichever mel
  requires grad: ``mean_b value_b / ((Ta_b + Tb_b) / 2)`` over the utterances with valid counts, 0 with zero gradients when
  there is none.  ``crit.values(...)`` -> the per-utterance fp64 values with a graph.

  ``mel_hat`` [B, n_mel, Ta] and ``mel_ref`` [B, n_mel, Tb]: fp32 on the module's device; the two lengths are independent.
  ``features="mfcc"`` compares coefficients 1 .. ``n_mfcc`` of the orthonormal DCT-II over the mel axis (the features of
  ``validate``'s DTW-MCD), applied as one fp64 matmul under autograd with the basis made on the host and rounded to fp32
  once; ``features="mel"`` compares the mels themselves (n_mel <= 128).  Frame counts, ``gamma`` and ``cost`` as
  ``soft_dtw``.  Mask, division and mean are small tensor operations on the device; nothing is read back.  CPU tensors,
  other dtypes or ranks, mismatching B or n_mel, more than 128 feature rows or 4096 frames, and a count outside ``[1, T]`` in a
  host list raise WgError before any launch."""

  def __init__(self, gamma: float = 1.0, features: str = "mfcc", n_mfcc: int = 16, cost: str = "l2", device="cuda"):
    super().__init__()
    device = torch.device(device)
    if device.type != "cuda":
      raise _lib.WgError("SoftDTWLoss runs on the GPU library only")
    if features not in FEATURES:
      raise _lib.WgError(f"SoftDTWLoss: features must be one of {FEATURES}, got {features!r}")
    if features == "mfcc" and not (isinstance(n_mfcc, int) and 1 <= n_mfcc <= metrics.MAX_FEATURES):
      raise _lib.WgError(f"SoftDTWLoss: 1 <= n_mfcc <= {metrics.MAX_FEATURES} expected, got {n_mfcc!r}")
    self.gamma, self.cost = _gamma(gamma), cost
    _cost(cost)
    self.features, self.n_mfcc, self.device = features, int(n_mfcc), device
    self._basis = {}                 # n_mel -> fp64 [n_mfcc, n_mel] on the device

  def _k(self, n_mel: int) -> int:
    return self.n_mfcc if self.features == "mfcc" else n_mel

  def workspace_bytes(self, B: int, Ta: int, Tb: int, n_mel: int = 80) -> int:
    """Bytes one forward with a graph keeps until its backward: the accumulated-cost matrix R (``wg_softdtw_bytes``), the
    fp32 features of both sides and, with "mfcc", the fp64 copies of both mels that the matmul keeps; 0 for a shape the
    kernels refuse.  E and the gradients live only while the backward runs."""
    r = r_bytes(B, Ta, Tb)
    if not r or not 1 <= self._k(n_mel) <= metrics.MAX_FEATURES:
      return 0
    kept = 4 * int(B) * self._k(n_mel) * (int(Ta) + int(Tb))
    if self.features == "mfcc":
      kept += 8 * int(B) * int(n_mel) * (int(Ta) + int(Tb))
    return r + kept

  def _check(self, mel_hat, mel_ref):
    for name, t in (("mel_hat", mel_hat), ("mel_ref", mel_ref)):
      _args.tensor(f"SoftDTWLoss: {name}", t, device=self.device, ndim=3)
      if t.shape[0] < 1 or t.shape[1] < 1 or not 1 <= t.shape[2] <= metrics.MAX_FRAMES:
        raise _lib.WgError(f"SoftDTWLoss takes {name} [B, n_mel, T] with 1 <= T <= {metrics.MAX_FRAMES}, got shape "
                           f"{tuple(t.shape)}")
    if mel_hat.shape[0] != mel_ref.shape[0] or mel_hat.shape[1] != mel_ref.shape[1]:
      raise _lib.WgError(f"SoftDTWLoss: batch and channel sizes differ, {tuple(mel_hat.shape)} against {tuple(mel_ref.shape)}")
    n_mel = mel_hat.shape[1]
    if self.features == "mfcc" and not self.n_mfcc < n_mel:
      raise _lib.WgError(f"SoftDTWLoss: n_mfcc < n_mel expected, got {self.n_mfcc} of {n_mel}")
    if self._k(n_mel) > metrics.MAX_FEATURES:
      raise _lib.WgError(f"SoftDTWLoss: at most {metrics.MAX_FEATURES} feature rows, got {self._k(n_mel)}")

  def feats(self, mel: torch.Tensor) -> torch.Tensor:
    """The feature rows the warping compares, fp32 [B, K, T], under autograd."""
    if self.features == "mel":
      return mel
    n_mel = mel.shape[1]
    basis = self._basis.get(n_mel)
    if basis is None:
      basis = self._basis[n_mel] = dct_basis(n_mel, self.n_mfcc).to(mel.device)
    return torch.matmul(basis, mel.to(torch.float64)).to(torch.float32)

  def _run(self, mel_hat, frames_hat, mel_ref, frames_ref):
    self._check(mel_hat, mel_ref)
    fa = metrics._frames("SoftDTWLoss: frames_hat", frames_hat, mel_hat, upload=False)
    fb = metrics._frames("SoftDTWLoss: frames_ref", frames_ref, mel_ref, upload=False)
    with torch.cuda.device(mel_hat.device):
      fa, fb = fa.to(mel_hat.device), fb.to(mel_ref.device)
      return soft_dtw(self.feats(mel_hat), fa, self.feats(mel_ref), fb, self.gamma, self.cost), fa, fb

  def values(self, mel_hat: torch.Tensor, frames_hat, mel_ref: torch.Tensor, frames_ref) -> torch.Tensor:
    """fp64 ``[B]``: the soft-DTW value of every utterance (NaN for a refused device count), with a graph in grad mode."""
    return self._run(mel_hat, frames_hat, mel_ref, frames_ref)[0]

  def forward(self, mel_hat: torch.Tensor, frames_hat, mel_ref: torch.Tensor, frames_ref) -> torch.Tensor:
    v, fa, fb = self._run(mel_hat, frames_hat, mel_ref, frames_ref)
    Ta, Tb = mel_hat.shape[2], mel_ref.shape[2]
    valid = (fa >= 1) & (fa <= Ta) & (fb >= 1) & (fb <= Tb)
    half = torch.where(valid, fa + fb, torch.full_like(fa, 2)).to(torch.float64) / 2.0
    count = valid.sum().clamp(min=1).to(torch.float64)
    return (torch.where(valid, v, torch.zeros_like(v)) / half).sum().div(count).to(torch.float32)
