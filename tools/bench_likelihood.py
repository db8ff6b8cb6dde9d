"""Timing of the per-utterance likelihood (``WaveGlow.log_likelihood``) beside the dense no-grad forward it rests on.
Two shapes: 16 x 864 frames (BASELINE.json configs[1]) and a ragged batch of 16 utterances of 200 .. 864 frames.

  forward_loss  (a) dense ``model((mel, audio))`` + ``WaveGlowLoss``: what a training log line costs; this leg uses nothing
                of the likelihood, so ``--legs a`` runs unmodified on a checkout without it
  ll_dense      (b) ``log_likelihood_enqueue(mel, audio)`` on the same dense batch
  ll_ragged     (c) ``log_likelihood_enqueue(mel, audio, frames)`` on the ragged batch (padded to 864 frames)
  nll_dense     (d) ``wg_nll`` alone on the z and log_s of the dense batch, between device events
  nll_ragged    (d) the same on the ragged batch

The legs alternate in one process, repetition by repetition, after a warm-up of all of them.  One JSON line with the
median, the 10th and 90th percentile and the extremes of every leg, (b) - (a), and (d) as a share of the forward.

  python tools/bench_likelihood.py [--reps 20] [--warmup 3] [--batch 16] [--frames 864] [--legs abcd]
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
from waveglow_amd.model import WaveGlow, WaveGlowLoss  # noqa: E402


def spread(ms):
  a = np.sort(np.asarray(ms))
  return {"median": float(np.median(a)), "p10": float(np.percentile(a, 10)), "p90": float(np.percentile(a, 90)),
          "min": float(a[0]), "max": float(a[-1]), "n": int(a.size)}


def timed(fn, dev):
  torch.cuda.synchronize(dev)
  t0 = time.perf_counter()
  out = fn()
  torch.cuda.synchronize(dev)
  return (time.perf_counter() - t0) * 1e3, out


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument("--reps", type=int, default=20)
  ap.add_argument("--warmup", type=int, default=3)
  ap.add_argument("--batch", type=int, default=16)
  ap.add_argument("--frames", type=int, default=864)
  ap.add_argument("--min-frames", type=int, default=200)
  ap.add_argument("--channels", type=int, default=256)
  ap.add_argument("--sigma", type=float, default=1.0)
  ap.add_argument("--legs", type=str, default="abcd")
  a = ap.parse_args()
  if a.reps < 1:
    ap.error("--reps must be at least 1")
  dev = torch.device("cuda:0")
  hp = HParams(n_channels=a.channels)
  model = WaveGlow.remove_weightnorm(WaveGlow(hp))
  model.load_state_dict(synthetic.make_state_dict(hp, seed=0))
  model = model.to(dev).eval()
  loss_fn = WaveGlowLoss(a.sigma)
  B, T = a.batch, a.frames
  mel = synthetic.make_mel(B, T, seed=5).to(dev)
  g = torch.Generator().manual_seed(17)
  audio = (torch.rand(B, 256 * T, generator=g) * 0.6 - 0.3).to(dev)
  ragged = [int(round(v)) for v in np.linspace(a.min_frames, T, B)]
  ragged = ragged[1::2] + ragged[0::2]                                   # the longest is neither first nor last
  frames_dev = torch.tensor(ragged, dtype=torch.int32).to(dev)
  state = {}

  def leg_a():
    def run():
      with torch.no_grad():
        state["loss"] = loss_fn(model((mel, audio)))
    return timed(run, dev)[0]

  def leg_b():
    return timed(lambda: state.update(rows=model.log_likelihood_enqueue(mel, audio, sigma=a.sigma)), dev)[0]

  def leg_c():
    return timed(lambda: state.update(rows_ragged=model.log_likelihood_enqueue(mel, audio, frames_dev, sigma=a.sigma)),
                 dev)[0]

  def leg_d(frames):
    from waveglow_amd import likelihood
    eng, z, log_s, fr = likelihood._forward(model, mel, audio, frames)
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    ev[0].record()
    likelihood.nll_enqueue(eng, z, log_s, fr, a.sigma)
    ev[1].record()
    torch.cuda.synchronize(dev)
    return ev[0].elapsed_time(ev[1])

  legs = {}
  if "a" in a.legs:
    legs["forward_loss"] = leg_a
  if "b" in a.legs:
    legs["ll_dense"] = leg_b
  if "c" in a.legs:
    legs["ll_ragged"] = leg_c
  if "d" in a.legs:
    legs["nll_dense"] = lambda: leg_d(None)
    legs["nll_ragged"] = lambda: leg_d(frames_dev)
  times = {k: [] for k in legs}
  for it in range(a.warmup + a.reps):
    for k, fn in legs.items():
      ms = fn()
      if it >= a.warmup:
        times[k].append(ms)
  out = {"batch": B, "frames": T, "ragged_frames": ragged, "channels": a.channels, "sigma": a.sigma,
         "ms": {k: spread(v) for k, v in times.items()}}
  med = lambda k: out["ms"][k]["median"]     # noqa: E731
  if "forward_loss" in legs and "ll_dense" in legs:
    out["ll_dense_minus_forward_loss_ms"] = med("ll_dense") - med("forward_loss")
    rows = state["rows"].cpu()
    out["batch_mean_nll"] = float((rows[:, 5] * rows[:, 0]).sum() / rows[:, 5].sum())
    out["forward_loss_value"] = float(state["loss"])
  if "nll_dense" in legs and "ll_dense" in legs:
    out["nll_share_of_ll_dense"] = med("nll_dense") / med("ll_dense")
  if "nll_ragged" in legs and "ll_ragged" in legs:
    out["nll_share_of_ll_ragged"] = med("nll_ragged") / med("ll_ragged")
  print(json.dumps(out), flush=True)


if __name__ == "__main__":
  main()
