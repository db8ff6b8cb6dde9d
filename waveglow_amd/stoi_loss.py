"""STOI / ESTOI as a training loss (``wg_stoi_forward``, ``wg_stoi_backward``, ``wg_resample_backward``): the metric
``validate --intelligibility-metrics`` reports, differentiated through the exact definition it uses.

The energy gate of the definition depends on the clean side alone, so with the target held constant both values are
differentiable in the processed audio (as ``torch_stoi``'s ``NegSTOILoss`` exploits).  One forward resamples both sides to
10 kHz with the project's resampler (skipped at 10 000 Hz), runs the five kernels of ``wg_stoi`` and keeps the band spectra;
one backward runs the reverses of those kernels in fp64 and the transposed polyphase filter, which takes the fp64 gradient
as it is and rounds to fp32 once.  No torch / CPU fallback.

  loss = -(factor_stoi * mean_b STOI_b + factor_estoi * mean_b ESTOI_b)      over the utterances that have a segment
"""
from __future__ import annotations

import torch

from . import _args, _lib, metrics, resample


class _ScoresFn(torch.autograd.Function):
  """Inputs: the module, audio and target [B, N] and the device lengths at the audio's rate.  Output: fp64 [B, 2].  The
  forward keeps the processed signal at 10 kHz and the library's saved buffer; the backward allocates its own scratch, so
  a second backward under retain_graph gives the same bits."""

  @staticmethod
  def forward(ctx, crit, audio, target, lens):
    x10, y10, n10 = crit._to_10k(audio.detach(), target, lens)
    rows, ctx.state = metrics.stoi_forward_saved(x10, n10, y10, n10)
    ctx.crit, ctx.lens, ctx.n_in = crit, lens, audio.shape[1]
    return rows[:, :2].clone()

  @staticmethod
  def backward(ctx, g):
    crit = ctx.crit
    d_y = metrics.stoi_backward_enqueue(ctx.state, g.to(torch.float64))
    if crit.sampling_rate == metrics.STOI_RATE:
      return None, d_y.to(torch.float32), None, None
    with torch.cuda.device(d_y.device):
      return None, resample.resample_backward_enqueue(d_y, ctx.lens, crit.sampling_rate, metrics.STOI_RATE, ctx.n_in), \
        None, None


class STOILoss(torch.nn.Module):
  """``crit(audio, target, lengths=None)`` -> 0-dim fp32 loss on the device with a graph back to ``audio``;
  ``crit.scores(audio, target, lengths=None)`` -> fp64 ``[B, 2]`` (STOI, ESTOI), NaN where an utterance has no segment.

  ``audio`` (processed) and ``target`` (clean): fp32 ``[B, N]`` on the module's device at ``sampling_rate``, same shape.
  Only ``audio`` gets a gradient (a ``target`` that requires grad raises WgError).  ``lengths``: None (all N), or B
  integers as ``_args.counts`` takes them (a list, a tuple or a 1-D CPU tensor of an integer dtype; a float or a bool
  entry raises WgError), each in ``[0, N]``; samples behind a length are never read and their gradient is exactly 0.
  The scores are the bits of ``metrics.intelligibility_metrics_enqueue(target, lengths, audio, lengths,
  sampling_rate)``.  The loss averages over the utterances that have a segment -- the mask and the means are small
  tensor ops on the device, nothing is read back -- and is 0 with zero gradients when none has.  CPU tensors, other
  dtypes or ranks, a shape mismatch and a rate the resampler refuses raise WgError before any launch.  Forward and
  backward enqueue on the current stream and never synchronise; values and gradients are bit-reproducible.  No double
  backward."""

  def __init__(self, sampling_rate=22050, factor_stoi=1.0, factor_estoi=0.0, device="cuda"):
    super().__init__()
    device = torch.device(device)
    if device.type != "cuda":
      raise _lib.WgError("STOILoss runs on the GPU library only")
    up, down, _, _ = resample.resample_plan(sampling_rate, metrics.STOI_RATE)      # refuses a rate before any device work
    self.sampling_rate, self._ratio = int(sampling_rate), (up, down)
    self.factor_stoi, self.factor_estoi = float(factor_stoi), float(factor_estoi)
    self.device = device

  def _n10(self, N: int) -> int:
    return resample.out_len(N, *self._ratio)

  def workspace_bytes(self, B: int, N: int) -> int:
    """Bytes one forward with a graph keeps until its backward for ``[B, N]`` audio: the processed signal at 10 kHz (fp32)
    and the saved buffer of ``wg_stoi_forward`` (counts, kept-frame lists, band spectra of both sides); 0 for a shape the
    kernels refuse.  The backward's own scratch lives only while it runs."""
    n10 = self._n10(int(N))
    saved = metrics.stoi_saved_bytes(int(B), n10) if 1 <= n10 <= metrics.STOI_MAX_PITCH else 0
    return saved + 4 * int(B) * n10 if saved else 0

  def _check(self, audio, target):
    for name, t in (("audio", audio), ("target", target)):
      _args.tensor(f"STOILoss: {name}", t, device=self.device, ndim=2)
      if t.shape[0] < 1 or t.shape[0] > 65535 or t.shape[1] < 1:
        raise _lib.WgError(f"STOILoss takes {name} [B, N] with 1 <= B <= 65535 and N >= 1, got shape {tuple(t.shape)}")
    if audio.shape != target.shape:
      raise _lib.WgError(f"audio {tuple(audio.shape)} and target {tuple(target.shape)} differ in shape")
    if target.requires_grad:
      raise _lib.WgError("STOILoss: only audio gets a gradient (the gate runs on the target); detach the target")
    if audio.shape[1] > resample.MAX_SAMPLES or self._n10(audio.shape[1]) > metrics.STOI_MAX_PITCH:
      raise _lib.WgError(f"STOILoss: rows of {audio.shape[1]} samples are beyond {metrics.STOI_MAX_PITCH} at 10 kHz")

  def _to_10k(self, audio, target, lens):
    """(x10k, y10k, lengths at 10 kHz) of contiguous rows: the clean side first."""
    if self.sampling_rate == metrics.STOI_RATE:
      return target.contiguous(), audio.contiguous(), lens
    up, down = self._ratio
    x10 = resample.resample_enqueue(target, lens, self.sampling_rate, metrics.STOI_RATE)
    y10 = resample.resample_enqueue(audio, lens, self.sampling_rate, metrics.STOI_RATE)
    n10 = (lens.to(torch.int64) * up + (down - 1)).div(down, rounding_mode="floor").to(torch.int32)
    return x10, y10, n10

  def scores(self, audio: torch.Tensor, target: torch.Tensor, lengths=None) -> torch.Tensor:
    """fp64 ``[B, 2]``: STOI and ESTOI of every utterance, with a graph back to ``audio`` in grad mode."""
    self._check(audio, target)
    B, N = audio.shape
    with torch.cuda.device(audio.device):
      lens = _args.counts("STOILoss: lengths", [N] * B if lengths is None else lengths, B, 0, N, device=audio.device)[0]
      if torch.is_grad_enabled() and audio.requires_grad:
        return _ScoresFn.apply(self, audio, target, lens)
      x10, y10, n10 = self._to_10k(audio.detach(), target, lens)
      return metrics.stoi_enqueue(x10, n10, y10, n10)[:, :2].clone()

  def forward(self, audio: torch.Tensor, target: torch.Tensor, lengths=None) -> torch.Tensor:
    s = self.scores(audio, target, lengths)
    scored = ~torch.isnan(s[:, 0])                                  # both values are NaN together: no segment
    count = scored.sum().clamp(min=1).to(torch.float64)
    mean = torch.where(scored[:, None], s, torch.zeros_like(s)).sum(dim=0) / count
    return (0.0 - (self.factor_stoi * mean[0] + self.factor_estoi * mean[1])).to(torch.float32)
