"""Timing of the intelligibility metrics of ``waveglow-cli validate --intelligibility-metrics`` per batch beside the work
the batch does anyway.  Two shapes, one JSON line each: 16 pairs of 864 frames' worth of audio (BASELINE.json configs[1])
and a ragged batch of 16 pairs with 200 .. 864 frames.  The original side of a pair is a harmonic tone under a 1.3 Hz
envelope (real pauses, so the energy gate removes frames), the other side the denoised synthesis of the batch,
peak-normalised as ``validate`` does it.

  resample  the two ``resample.resample_enqueue`` calls that bring both sides from the model's rate to 10 kHz
  stoi      ``metrics.stoi_enqueue`` on the two 10 kHz batches (wg_stoi alone: five launches)
  intel     ``metrics.intelligibility_metrics_enqueue``: what the flag adds to a validate batch (the two above and the
            small tensor operations for the common length)
  pitch     ``metrics.pitch_metrics_enqueue`` on the same two audio batches
  metrics   ``metrics.mel_metrics_enqueue`` on the original and the inferred mels
  flow      ``Synthesizer._infer_batch_device`` of the same batch: flow + denoiser between its own device events
  host      the numpy restatement (tests/_stoi_oracle.py) on the device resampler's output, per pair, over the first
            ``--host-pairs`` pairs; pystoi is not installed here and cannot be a leg

The legs alternate in one process, repetition by repetition, after a warm-up of all of them; the host leg runs in the first
``--host-reps`` repetitions only.  Each line gives the median, the 10th and 90th percentile and the extremes.

  python tools/bench_stoi.py [--reps 20] [--warmup 3] [--host-reps 1] [--batch 16] [--frames 864]
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
import _stoi_oracle as oracle  # noqa: E402
from waveglow_amd import metrics, resample, synthetic  # noqa: E402
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


def original(n, sr, seed):
  """n samples: 29 harmonics of a gliding tone under a squared, clipped 1.3 Hz envelope, plus a noise floor."""
  rng = np.random.default_rng(seed)
  t = np.arange(n) / sr
  f = rng.uniform(90, 140) + 10 * np.sin(2 * np.pi * 0.4 * t)
  phi = np.cumsum(2 * np.pi * f / sr)
  x = sum(np.sin(k * phi) / k for k in range(1, 30)) * np.clip(np.sin(2 * np.pi * 1.3 * t + rng.uniform(0, 6)), 0, 1) ** 2
  return (0.5 * x / np.max(np.abs(x)) + 1e-4 * rng.standard_normal(n)).astype(np.float32)


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument("--reps", type=int, default=20)
  ap.add_argument("--warmup", type=int, default=3)
  ap.add_argument("--host-reps", type=int, default=1)
  ap.add_argument("--host-pairs", type=int, default=2, help="pairs of the batch the host leg computes")
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
  sr = hp.sampling_rate
  model = WaveGlow(hp)
  model.load_state_dict(synthetic.to_weightnorm_form(synthetic.make_state_dict(hp, seed=0)))
  synth = Synthesizer(CheckpointWaveglow.from_instances(model, None, hp, 1), device=dev)
  taco = TacotronSTFT(hp, dev)
  ragged = [int(round(v)) for v in np.linspace(a.min_frames, a.frames, a.batch)]
  ragged = ragged[1::2] + ragged[0::2]                                   # the longest is neither first nor last
  for name, frames in (("uniform", [a.frames] * a.batch), ("ragged", ragged)):
    samples = [256 * t for t in frames]
    wavs = [original(n, sr, 200 + i) for i, n in enumerate(samples)]
    orig = torch.zeros((a.batch, max(samples)))
    for b, w in enumerate(wavs):
      orig[b, :samples[b]] = torch.from_numpy(w)
    orig = orig.to(dev)
    samples_dev = torch.tensor(samples, dtype=torch.int32).to(dev)
    up, down, _, _ = resample.resample_plan(sr, metrics.STOI_RATE)
    samples10 = [resample.out_len(n, up, down) for n in samples]
    samples10_dev = torch.tensor(samples10, dtype=torch.int32).to(dev)
    mel_orig, frames_orig, frames_orig_dev = taco.mel_spectrogram_ragged_device(orig, samples)
    mels = [mel_orig[b, :, :frames[b]].contiguous() for b in range(a.batch)]
    state = {}
    n_host = max(1, min(a.host_pairs, a.batch))

    def leg_flow():
      audio, den, _, _, ev = synth._infer_batch_device(mels, a.sigma, a.strength, a.seed)
      normed = den / den.abs().amax(dim=1, keepdim=True)
      state["normed"], state["ev"] = normed, ev
      state["inf"] = taco.mel_spectrogram_ragged_device(normed, samples)

    def leg_metrics():
      mel_inf, _, frames_inf_dev = state["inf"]
      return timed(lambda: metrics.mel_metrics_enqueue(mel_orig, frames_orig_dev, mel_inf, frames_inf_dev), dev)[0]

    def leg_pitch():
      return timed(lambda: metrics.pitch_metrics_enqueue(orig, samples_dev, state["normed"], samples_dev, sampling_rate=sr),
                   dev)[0]

    def leg_resample():
      def both():
        state["x10"] = resample.resample_enqueue(orig, samples_dev, sr, metrics.STOI_RATE)
        state["y10"] = resample.resample_enqueue(state["normed"], samples_dev, sr, metrics.STOI_RATE)
      return timed(both, dev)[0]

    def leg_stoi():
      return timed(lambda: state.update(rows_alone=metrics.stoi_enqueue(state["x10"], samples10_dev, state["y10"],
                                                                        samples10_dev)), dev)[0]

    def leg_intel():
      return timed(lambda: state.update(rows=metrics.intelligibility_metrics_enqueue(
        orig, samples_dev, state["normed"], samples_dev, sampling_rate=sr)), dev)[0]

    def leg_host():
      x10, y10 = state["x10"].cpu().numpy(), state["y10"].cpu().numpy()
      t0 = time.perf_counter()
      state["ref"] = [oracle.stoi(x10[b, :samples10[b]], y10[b, :samples10[b]]) for b in range(n_host)]
      return (time.perf_counter() - t0) * 1e3 / n_host

    times = {k: [] for k in ("flow", "metrics", "pitch", "resample", "stoi", "intel", "host")}
    for it in range(a.warmup + a.reps):
      leg_flow()
      torch.cuda.synchronize(dev)
      ms = {"flow": state["ev"][0].elapsed_time(state["ev"][2]), "metrics": leg_metrics(), "pitch": leg_pitch(),
            "resample": leg_resample(), "stoi": leg_stoi(), "intel": leg_intel()}
      if a.warmup <= it < a.warmup + a.host_reps:
        ms["host"] = leg_host()
      if it >= a.warmup:
        for k, v in ms.items():
          times[k].append(v)
    rows = state["rows"].cpu().numpy()
    out = {"shape": name, "batch": a.batch, "frames": frames if name == "ragged" else a.frames, "channels": a.channels,
           "stoi_frames": [int(v) for v in rows[:, metrics.STOI_FRAMES]],
           "stoi_frames_kept": [int(v) for v in rows[:, metrics.STOI_FRAMES_KEPT]],
           "fused_equals_parts": bool(rows.tobytes() == state["rows_alone"].cpu().numpy().tobytes()),
           "ms": {k: spread(v) for k, v in times.items() if v}}
    out["intel_share_of_flow"] = out["ms"]["intel"]["median"] / out["ms"]["flow"]["median"]
    out["stoi_over_pitch"] = out["ms"]["stoi"]["median"] / out["ms"]["pitch"]["median"]
    if "ref" in state:
      ref = state["ref"]
      out["host_pairs"] = n_host                                        # ms["host"] is per pair
      out["counts_equal_host"] = bool(all(
        (int(rows[b, 2]), int(rows[b, 3]), int(rows[b, 4])) == (ref[b]["frames"], ref[b]["frames_kept"], ref[b]["segments"])
        for b in range(n_host)))
      out["largest_distance_to_host"] = float(max(max(abs(rows[b, 0] - ref[b]["stoi"]), abs(rows[b, 1] - ref[b]["estoi"]))
                                                  for b in range(n_host)))
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
  main()
