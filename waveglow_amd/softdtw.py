"""Soft dynamic time warping as a training loss (``wg_softdtw_forward`` / ``wg_softdtw_backward``): the warped distance that
``validate`` reports as "MFCC DTW MCD" (``metrics.dtw_distance``), smoothed so that it has a gradient (Cuturi and Blondel,
"Soft-DTW: a differentiable loss function for time-series", ICML 2017).  It compares a generated mel of ``Ta`` frames with a
recording of ``Tb`` frames, which the frame-by-frame losses (``MultiResolutionSTFTLoss``, ``STOILoss``, a mel L1) cannot.

One forward is one launch, a wavefront over the anti-diagonals that keeps the accumulated-cost matrix R; one backward is a
second wavefront that gives the expected alignment E and one launch per feature gradient.  The definition is stated in
include/waveglow_amd.h and DESIGN.md section 7.  No torch / CPU fallback.  ``band=w`` restricts the warping to a Sakoe-Chiba
band (``wg_softdtw_banded_*``: R and E shrink to the band); ``soft_dtw_divergence`` and ``SoftDTWLoss(divergence=True)``
subtract the two self-terms, so that the minimum lies at equal sequences.

  loss = mean_b value_b / ((Ta_b + Tb_b) / 2)          over the utterances with valid frame counts
"""
from __future__ import annotations

import math

import torch

from . import _args, _lib, metrics
from ._args import ptr

COSTS = {"l2": _lib.WG_SDTW_L2, "sq": _lib.WG_SDTW_SQ}
FEATURES = ("mfcc", "mel")
MAX_BAND = 511


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


def _band(band):
  """None (the whole matrix) or the Sakoe-Chiba half-width, an int in [1, MAX_BAND]."""
  if band is None:
    return None
  if isinstance(band, bool) or not isinstance(band, int) or not 1 <= band <= MAX_BAND:
    raise _lib.WgError(f"soft_dtw: band must be None or an int in [1, {MAX_BAND}], got {band!r}")
  return band


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


def r_bytes(B: int, Ta: int, Tb: int, band=None) -> int:
  """Bytes of the accumulated-cost matrix one forward with a graph keeps (``wg_softdtw_bytes``, or
  ``wg_softdtw_banded_bytes`` with a band; 0 outside the limits)."""
  if _band(band) is None:
    return int(_lib.load().wg_softdtw_bytes(int(B), int(Ta), int(Tb)))
  return int(_lib.load().wg_softdtw_banded_bytes(int(B), int(Ta), int(Tb), band))


def _forward(a, fa, b, fb, gamma, cost, keep_r, band=None):
  B, K, Ta = a.shape
  Tb = b.shape[2]
  lib = _lib.load()
  with torch.cuda.device(a.device):
    value = torch.empty(B, dtype=torch.float64, device=a.device)
    r = torch.empty(r_bytes(B, Ta, Tb, band) // 8, dtype=torch.float64, device=a.device) if keep_r else None
    if band is None:
      _lib.check(lib.wg_softdtw_forward(ptr(a), ptr(fa), ptr(b), ptr(fb), gamma, cost, ptr(value), ptr(r), B, K, Ta, Tb,
                                        _args.stream(a.device)))
    else:
      _lib.check(lib.wg_softdtw_banded_forward(ptr(a), ptr(fa), ptr(b), ptr(fb), gamma, cost, ptr(value), ptr(r), B, K,
                                               Ta, Tb, band, _args.stream(a.device)))
  return value, r


def _backward(a, fa, b, fb, gamma, cost, r, g_value, want_e, want_a, want_b, band=None):
  """(E or None, g_a or None, g_b or None).  The gradients need E: the dense call gets it as a temporary here when the
  caller does not want it, the banded call takes its own in the band layout and fills the dense E only when asked."""
  B, K, Ta = a.shape
  Tb = b.shape[2]
  lib = _lib.load()
  with torch.cuda.device(a.device):
    e = torch.empty((B, Ta, Tb), dtype=torch.float64, device=a.device) if band is None or want_e else None
    g_a = torch.empty((B, K, Ta), dtype=torch.float32, device=a.device) if want_a else None
    g_b = torch.empty((B, K, Tb), dtype=torch.float32, device=a.device) if want_b else None
    if band is None:
      _lib.check(lib.wg_softdtw_backward(ptr(a), ptr(fa), ptr(b), ptr(fb), gamma, cost, ptr(r), ptr(g_value), ptr(e),
                                         ptr(g_a), ptr(g_b), B, K, Ta, Tb, _args.stream(a.device)))
    else:
      _lib.check(lib.wg_softdtw_banded_backward(ptr(a), ptr(fa), ptr(b), ptr(fb), gamma, cost, ptr(r), ptr(g_value),
                                                ptr(e), ptr(g_a), ptr(g_b), B, K, Ta, Tb, band, _args.stream(a.device)))
  return (e if want_e else None), g_a, g_b


class _SoftDtwFn(torch.autograd.Function):
  """(feat_a, frames_a, feat_b, frames_b, gamma, cost id, band) -> fp64 [B].  The forward keeps the features as the kernels
  read them, the counts and R; the backward allocates its own outputs, so a second backward under retain_graph gives the
  same bits."""

  @staticmethod
  def forward(ctx, feat_a, fa, feat_b, fb, gamma, cost, band=None):
    a, b = feat_a.detach().contiguous(), feat_b.detach().contiguous()
    value, r = _forward(a, fa, b, fb, gamma, cost, True, band)
    ctx.state = (a, fa, b, fb, gamma, cost, r, band)
    return value

  @staticmethod
  @torch.autograd.function.once_differentiable
  def backward(ctx, g):
    a, fa, b, fb, gamma, cost, r, band = ctx.state
    want_a, want_b = ctx.needs_input_grad[0], ctx.needs_input_grad[2]
    _, g_a, g_b = _backward(a, fa, b, fb, gamma, cost, r, g.to(torch.float64).contiguous(), False, want_a, want_b, band)
    return g_a, None, g_b, None, None, None, None


def soft_dtw(feat_a: torch.Tensor, frames_a, feat_b: torch.Tensor, frames_b, gamma: float = 1.0,
             cost: str = "l2", *, band=None) -> torch.Tensor:
  """fp64 ``[B]`` on the device: the soft-DTW value of the columns of ``feat_a`` [B, K, Ta] against those of ``feat_b``
  [B, K, Tb] (fp32 on one GPU, K <= 128, T <= 4096) with ``frames_a[b]`` / ``frames_b[b]`` frames each, and a graph to
  whichever of the two requires grad; the same tensor may stand on both sides.  ``cost``: "l2", the Euclidean frame
  distance of ``metrics.dtw_distance`` (the value tends to its cost as gamma -> 0), or "sq", its square.  Frame counts:
  None (all), or B integers as ``_args.counts`` takes them (a list, a tuple or a 1-D CPU tensor of an integer dtype; a
  float or a bool entry raises WgError), each in ``[1, T]`` (checked before any launch), or an int32 tensor ``[B]`` on
  the device, which is trusted and never read on the host: a count outside the limits there gives a NaN value and zero
  gradients for that utterance. Nothing behind a count is read.  Gradients are computed in fp64 and rounded to fp32
  once.  Without grad mode, or when nothing requires grad, only the values are computed: no R is kept and nothing is
  saved.  Enqueue-only; bit-reproducible; no double backward.

  ``band``: None, the whole matrix, or the half-width w of a Sakoe-Chiba band, an int in [1, 511] (anything else raises
  WgError before the tensor checks): with n = Ta - 1, m = Tb - 1, cell (i, j) takes part iff |i m - j n| <= w max(n, m),
  and the kept R shrinks to ``r_bytes(B, Ta, Tb, band)``.  A band that covers the matrix gives the bits of ``band=None``."""
  w = _band(band)
  a, fa, b, fb, g, c = _check(feat_a, frames_a, feat_b, frames_b, gamma, cost)
  if torch.is_grad_enabled() and (feat_a.requires_grad or feat_b.requires_grad):
    return _SoftDtwFn.apply(feat_a, fa, feat_b, fb, g, c, w)
  return _forward(a, fa, b, fb, g, c, False, w)[0]


def soft_dtw_alignment(feat_a: torch.Tensor, frames_a, feat_b: torch.Tensor, frames_b, gamma: float = 1.0,
                       cost: str = "l2", *, band=None):
  """``(values fp64 [B], E fp64 [B, Ta, Tb])`` without a graph: E(i, j) is the expected alignment, the weight of cell (i, j)
  over all warping paths under the Gibbs distribution of temperature gamma; E(0, 0) = E(Ta-1, Tb-1) = 1, exact zeros behind
  an utterance's frames and, with a ``band``, outside it.  Arguments as ``soft_dtw``."""
  w = _band(band)
  a, fa, b, fb, g, c = _check(feat_a, frames_a, feat_b, frames_b, gamma, cost)
  a, b = a.detach(), b.detach()
  value, r = _forward(a, fa, b, fb, g, c, True, w)
  e, _, _ = _backward(a, fa, b, fb, g, c, r, None, True, False, False, w)
  return value, e


def _triple(a, fa, b, fb):
  """The 3 B pairs of the divergence at the common length T = max(Ta, Tb): left operands [a; a; b], right operands
  [b; a; b], the counts alike.  Small device copies; where either count lies outside its own side's [1, T] both become 0, so
  the padding is never taken for frames."""
  Ta, Tb = a.shape[2], b.shape[2]
  T = max(Ta, Tb)
  pa = torch.nn.functional.pad(a, (0, T - Ta)) if Ta < T else a
  pb = torch.nn.functional.pad(b, (0, T - Tb)) if Tb < T else b
  valid = (fa >= 1) & (fa <= Ta) & (fb >= 1) & (fb <= Tb)      # else all three pairs of the utterance are refused
  fa, fb = torch.where(valid, fa, torch.zeros_like(fa)), torch.where(valid, fb, torch.zeros_like(fb))
  return torch.cat([pa, pa, pb]), torch.cat([fa, fa, fb]), torch.cat([pb, pa, pb]), torch.cat([fb, fa, fb])


def _combine(v, B):
  return v[:B] - 0.5 * (v[B:2 * B] + v[2 * B:])


class _DivergenceFn(torch.autograd.Function):
  """(feat_a, frames_a, feat_b, frames_b, gamma, cost id, band) -> fp64 [B]: one forward and one backward call over the
  3 B pairs of ``_triple``, which are what the forward keeps beside R.  A side's gradient has three terms, from the cross
  pair and from both operands of its self pair, each rounded to fp32 by the kernels; they are summed in fp64 and rounded
  once."""

  @staticmethod
  def forward(ctx, feat_a, fa, feat_b, fb, gamma, cost, band):
    a3, fa3, b3, fb3 = _triple(feat_a.detach(), fa, feat_b.detach(), fb)
    value, r = _forward(a3, fa3, b3, fb3, gamma, cost, True, band)
    ctx.state = (a3, fa3, b3, fb3, gamma, cost, r, band, feat_a.shape[2], feat_b.shape[2])
    return _combine(value, feat_a.shape[0])

  @staticmethod
  @torch.autograd.function.once_differentiable
  def backward(ctx, g):
    a3, fa3, b3, fb3, gamma, cost, r, band, Ta, Tb = ctx.state
    B = a3.shape[0] // 3
    g = g.to(torch.float64)
    g3 = torch.cat([g, -0.5 * g, -0.5 * g])
    _, l, rt = _backward(a3, fa3, b3, fb3, gamma, cost, r, g3, False, True, True, band)
    l, rt = l.to(torch.float64), rt.to(torch.float64)
    g_a = g_b = None
    if ctx.needs_input_grad[0]:
      g_a = ((l[:B] + l[B:2 * B]) + rt[B:2 * B])[:, :, :Ta].to(torch.float32)
    if ctx.needs_input_grad[2]:
      g_b = ((rt[:B] + l[2 * B:]) + rt[2 * B:])[:, :, :Tb].to(torch.float32)
    return g_a, None, g_b, None, None, None, None


def soft_dtw_divergence(feat_a: torch.Tensor, frames_a, feat_b: torch.Tensor, frames_b, gamma: float = 1.0,
                        cost: str = "l2", *, band=None) -> torch.Tensor:
  """fp64 ``[B]`` on the device: the soft-DTW divergence ``D = sdtw(a, b) - 0.5 (sdtw(a, a) + sdtw(b, b))`` (Blondel, Mensch
  and Vert, AISTATS 2021), each term the ``soft_dtw`` value of that pair under the same ``gamma``, ``cost`` and ``band``,
  with a graph to whichever side requires grad.  Unlike the plain value it is 0 at a = b, and for ``cost="sq"`` without a
  band non-negative.  One forward and one backward call over 3 B pairs at the common length max(Ta, Tb): left operands
  [a; a; b], right operands [b; a; b].  As an utterance's bits depend on neither its batch nor its pitch, D has the bits
  of that combination of three ``soft_dtw`` calls, and a gradient is the fp64 sum of their three fp32 gradient terms
  rounded to fp32 once.  NaN where any of the three values is.  Arguments and refusals as ``soft_dtw``; a device count
  outside ``[1, T]`` of its own side gives NaN and zero gradients for that utterance."""
  w = _band(band)
  a, fa, b, fb, g, c = _check(feat_a, frames_a, feat_b, frames_b, gamma, cost)
  with torch.cuda.device(a.device):
    if torch.is_grad_enabled() and (feat_a.requires_grad or feat_b.requires_grad):
      return _DivergenceFn.apply(feat_a, fa, feat_b, fb, g, c, w)
    a3, fa3, b3, fb3 = _triple(a.detach(), fa, b.detach(), fb)
    return _combine(_forward(a3, fa3, b3, fb3, g, c, False, w)[0], a.shape[0])


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
  ``soft_dtw``.  ``band``: None or the Sakoe-Chiba half-width of ``soft_dtw``.  ``divergence=True`` puts the soft-DTW
  divergence (``soft_dtw_divergence``: 0 at mel_hat = mel_ref) in the place of the value, in ``values`` and in the loss.
  Mask, division and mean are small tensor operations on the device; nothing is read back.  CPU tensors,
  other dtypes or ranks, mismatching B or n_mel, more than 128 feature rows or 4096 frames, and a count outside ``[1, T]`` in a
  host list raise WgError before any launch."""

  def __init__(self, gamma: float = 1.0, features: str = "mfcc", n_mfcc: int = 16, cost: str = "l2", device="cuda", *,
               band=None, divergence: bool = False):
    super().__init__()
    self.band, self.divergence = _band(band), bool(divergence)
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
    """Bytes one forward with a graph keeps until its backward: the accumulated-cost matrix R (``r_bytes`` with the
    module's band), the fp32 features of both sides as the kernels read them and, with "mfcc", the fp64 copies of both mels
    that the matmul keeps; 0 for a shape the kernels refuse.  With the divergence R and the features are those of 3 B
    pairs at the common length max(Ta, Tb).  E and the gradients live only while the backward runs."""
    pairs, la, lb = int(B), int(Ta), int(Tb)
    if self.divergence and r_bytes(B, Ta, Tb, self.band):        # three pairs per utterance at the common length
      pairs, la, lb = 3 * pairs, max(la, lb), max(la, lb)
    r = r_bytes(pairs, la, lb, self.band)
    if not r or not 1 <= self._k(n_mel) <= metrics.MAX_FEATURES:
      return 0
    kept = 4 * pairs * self._k(n_mel) * (la + lb)
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
      fn = soft_dtw_divergence if self.divergence else soft_dtw
      return fn(self.feats(mel_hat), fa, self.feats(mel_ref), fb, self.gamma, self.cost, band=self.band), fa, fb

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
