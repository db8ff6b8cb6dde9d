"""Timing of ``WaveGlow.infer_differentiable`` forward + backward with per-utterance frame counts beside the dense call.
Shape: 32 x 63 frames (BASELINE.json configs[3]), 256 channels, frozen vocoder, gradients for mel and the noise.

  dense          (a) the call without ``frames``: this leg uses nothing of the feature, so ``--legs a`` runs unmodified on a
                 checkout without it -- the regression check against the parent commit
  full_counts    (b) the same call with ``frames=[63] * 32``: what the keyword itself costs (the planes are cleared on every
                 ragged call)
  ragged         (c) counts spread over 20 .. 63, the longest neither first nor last
  ragged_wgrads  (d) (c) with ``weight_grads=True``: the vocoder's own parameters trainable

The loss is ``(audio * r).sum()`` with ``r`` zero behind the counts in every leg that has them; ``model.grad_scale`` is the
automatic one.  The counts are a device tensor, uploaded once.  The legs alternate in one process, repetition by
repetition, after a warm-up of all of them; every time is a host clock around work that ends in a device synchronise.  One
JSON line with the median, the 10th and 90th percentile and the extremes of every leg, and the ratios to (a).

  python tools/bench_infer_ragged.py [--reps 20] [--warmup 3] [--batch 32] [--frames 63] [--min-frames 20] [--legs abcd]
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
sys.path.insert(0, ROOT)
from waveglow_amd import synthetic  # noqa: E402
from waveglow_amd.hparams import HParams  # noqa: E402
from waveglow_amd.model import WaveGlow  # noqa: E402


def spread(ms):
  a = np.sort(np.asarray(ms))
  return {"median": float(np.median(a)), "p10": float(np.percentile(a, 10)), "p90": float(np.percentile(a, 90)),
          "min": float(a[0]), "max": float(a[-1]), "n": int(a.size)}


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument("--reps", type=int, default=20)
  ap.add_argument("--warmup", type=int, default=3)
  ap.add_argument("--batch", type=int, default=32)
  ap.add_argument("--frames", type=int, default=63)
  ap.add_argument("--min-frames", type=int, default=20)
  ap.add_argument("--channels", type=int, default=256)
  ap.add_argument("--sigma", type=float, default=0.6)
  ap.add_argument("--legs", type=str, default="abcd")
  a = ap.parse_args()
  if a.reps < 1:
    ap.error("--reps must be at least 1")
  dev = torch.device("cuda:0")
  hp = HParams(n_channels=a.channels)
  B, T = a.batch, a.frames
  L = 32 * T

  def make_model(trainable):
    model = WaveGlow(hp)
    model.load_state_dict(synthetic.to_weightnorm_form(synthetic.make_state_dict(hp, seed=0)))
    return model.to(dev).train().requires_grad_(trainable)

  frozen = make_model(False)
  gen = torch.Generator().manual_seed(17)
  mel = synthetic.make_mel(B, T, seed=5).to(dev).requires_grad_(True)
  zi = torch.randn(B, frozen.n_remaining_channels, L, generator=gen).to(dev).requires_grad_(True)
  ze = [torch.randn(B, hp.n_early_size, L, generator=gen).to(dev).requires_grad_(True) for _ in range(frozen.n_early_flows())]
  r = torch.randn(B, 256 * T, generator=gen) / (B * 256 * T)
  ragged = [int(round(v)) for v in np.linspace(a.min_frames, T, B)]
  ragged = ragged[1::2] + ragged[0::2]                                   # the longest is neither first nor last
  r_ragged = r.clone()
  for b, f in enumerate(ragged):
    r_ragged[b, 256 * f:] = 0.0
  r, r_ragged = r.to(dev), r_ragged.to(dev)

  def step(model, cot, **kw):
    def run():
      for t in [mel, zi] + ze:
        t.grad = None
      model.zero_grad(set_to_none=True)
      audio = model.infer_differentiable(mel, a.sigma, z_init=zi, z_early=ze, **kw)
      (audio * cot).sum().backward()
    torch.cuda.synchronize(dev)
    t0 = time.perf_counter()
    run()
    torch.cuda.synchronize(dev)
    return (time.perf_counter() - t0) * 1e3

  legs = {}
  if "a" in a.legs:
    legs["dense"] = lambda: step(frozen, r)
  if "b" in a.legs:
    full_dev = torch.tensor([T] * B, dtype=torch.int32).to(dev)
    legs["full_counts"] = lambda: step(frozen, r, frames=full_dev)
  if "c" in a.legs or "d" in a.legs:
    ragged_dev = torch.tensor(ragged, dtype=torch.int32).to(dev)
  if "c" in a.legs:
    legs["ragged"] = lambda: step(frozen, r_ragged, frames=ragged_dev)
  if "d" in a.legs:
    trainable = make_model(True)
    legs["ragged_wgrads"] = lambda: step(trainable, r_ragged, frames=ragged_dev, weight_grads=True)
  times = {k: [] for k in legs}
  for it in range(a.warmup + a.reps):
    for k, fn in legs.items():
      ms = fn()
      if it >= a.warmup:
        times[k].append(ms)
  out = {"batch": B, "frames": T, "ragged_frames": ragged, "ragged_share_of_frames": sum(ragged) / (B * T),
         "channels": a.channels, "sigma": a.sigma, "ms": {k: spread(v) for k, v in times.items()}}
  if "dense" in legs:
    for k in legs:
      if k != "dense":
        out[f"{k}_over_dense"] = out["ms"][k]["median"] / out["ms"]["dense"]["median"]
  print(json.dumps(out), flush=True)


if __name__ == "__main__":
  main()
