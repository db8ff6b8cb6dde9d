"""Timing of the device work of ``waveglow-cli validate`` per batch, leg by leg.  Two shapes, one JSON line each: 16 pairs
of 864 / 865 frames (BASELINE.json configs[1]) and a ragged batch of 16 pairs with 200 .. 864 frames.

  metrics   metrics.mel_metrics_enqueue on the original and the inferred mels (wg_metrics_mel: two MFCC launches, the DTW
            wavefront, the padded MCD and cosine kernel)
  mel       TacotronSTFT.mel_spectrogram_ragged_device of the synthesised audio (the inferred mel)
  flow      Synthesizer._infer_batch_device of the same batch: flow + denoiser between its own device events, so the
            per-utterance noise draws before the flow are not in it
  host      the numpy restatement of the metrics (tests/_metrics_oracle.py) on the host, pair by pair; the reference's
            own implementation (mel_cepstral_distance with fastdtw) is not installed here and cannot be a leg

The legs alternate in one process, repetition by repetition, after a warm-up of all of them; the host leg, seconds per
batch, runs in the first ``--host-reps`` repetitions only.  Each line gives the median, the 10th and 90th percentile and
the extremes; ``metrics_share_of_flow`` is the ratio of the two medians of the same run.

  python tools/bench_validate.py [--reps 20] [--warmup 3] [--host-reps 2] [--batch 16] [--frames 864]
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
sys.path.insert(0, os.path.join(ROOT, "tests"))
import _metrics_oracle as oracle  # noqa: E402
from waveglow_amd import metrics, synthetic  # noqa: E402
from waveglow_amd.checkpoint import CheckpointWaveglow  # noqa: E402
from waveglow_amd.hparams import HParams  # noqa: E402
from waveglow_amd.model import WaveGlow  # noqa: E402
from waveglow_amd.synthesizer import Synthesizer  # noqa: E402
from waveglow_amd.taco_stft import TacotronSTFT  # noqa: E402


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
  ap.add_argument("--host-reps", type=int, default=2)
  ap.add_argument("--batch", type=int, default=16)
  ap.add_argument("--frames", type=int, default=864)
  ap.add_argument("--min-frames", type=int, default=200)
  ap.add_argument("--channels", type=int, default=256)
  ap.add_argument("--strength", type=float, default=0.0005)
  ap.add_argument("--sigma", type=float, default=0.6)
  ap.add_argument("--seed", type=int, default=1)
  a = ap.parse_args()
  if a.reps < 1:
    ap.error("--reps must be at least 1")
  dev = torch.device("cuda:0")
  hp = HParams(n_channels=a.channels)
  model = WaveGlow(hp)
  model.load_state_dict(synthetic.to_weightnorm_form(synthetic.make_state_dict(hp, seed=0)))
  synth = Synthesizer(CheckpointWaveglow.from_instances(model, None, hp, 1), device=dev)
  taco = TacotronSTFT(hp, dev)
  ragged = [int(round(v)) for v in np.linspace(a.min_frames, a.frames, a.batch)]
  ragged = ragged[1::2] + ragged[0::2]                                   # the longest is neither first nor last
  for name, frames in (("uniform", [a.frames] * a.batch), ("ragged", ragged)):
    mels = [synthetic.make_mel(1, T, seed=100 + i).to(dev) for i, T in enumerate(frames)]
    mel_orig = torch.zeros((a.batch, hp.n_mel_channels, max(frames)), device=dev)
    for b, m in enumerate(mels):
      mel_orig[b, :, :frames[b]] = m[0]
    frames_dev = torch.tensor(frames, dtype=torch.int32).to(dev)
    samples = [256 * t for t in frames]
    state = {}

    def leg_flow():
      audio, den, _, _, ev = synth._infer_batch_device(mels, a.sigma, a.strength, a.seed)
      state["den"], state["ev"] = den, ev

    def leg_mel():
      den = state["den"]
      normed = den / den.abs().amax(dim=1, keepdim=True)
      state["normed"] = normed
      return timed(lambda: state.update(inf=taco.mel_spectrogram_ragged_device(normed, samples)), dev)[0]

    def leg_metrics():
      mel_inf, _, frames_inf_dev = state["inf"]
      return timed(lambda: state.update(rows=metrics.mel_metrics_enqueue(mel_orig, frames_dev, mel_inf, frames_inf_dev)),
                   dev)[0]

    def leg_host():
      mel_inf, frames_inf, _ = state["inf"]
      o, i = mel_orig.cpu().numpy(), mel_inf.cpu().numpy()
      t0 = time.perf_counter()
      ref = [oracle.mel_metrics(o[b, :, :frames[b]], i[b, :, :frames_inf[b]]) for b in range(a.batch)]
      state["ref"] = ref
      return (time.perf_counter() - t0) * 1e3

    times = {k: [] for k in ("flow", "mel", "metrics", "host")}
    for it in range(a.warmup + a.reps):
      leg_flow()
      torch.cuda.synchronize(dev)
      ms = {"flow": state["ev"][0].elapsed_time(state["ev"][2]), "mel": leg_mel(), "metrics": leg_metrics()}
      if a.warmup <= it < a.warmup + a.host_reps:
        ms["host"] = leg_host()
      if it >= a.warmup:
        for k, v in ms.items():
          times[k].append(v)
    rows = state["rows"].cpu().numpy()
    out = {"shape": name, "batch": a.batch, "frames": frames if name == "ragged" else a.frames, "channels": a.channels,
           "ms": {k: spread(v) for k, v in times.items() if v}}
    out["metrics_share_of_flow"] = out["ms"]["metrics"]["median"] / out["ms"]["flow"]["median"]
    if "ref" in state:
      ref = state["ref"]
      out["frames_dtw_equal_host"] = bool(all(int(rows[b, metrics.FRAMES_DTW]) == ref[b]["frames_dtw"] for b in range(a.batch)))
      out["mcd_dtw_max_rel_diff"] = float(max(abs(rows[b, metrics.MCD_DTW] - ref[b]["mcd_dtw"]) / ref[b]["mcd_dtw"]
                                              for b in range(a.batch)))
      out["host_min_margin"] = float(min(r["margin"] for r in ref))
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
  main()
