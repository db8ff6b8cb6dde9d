"""Timing of one batched synthesis from mel-spectrograms on the device to int16 samples on the host: what
``waveglow-cli synthesize --batch-size N`` does per batch, without the file reads and writes.  Two shapes, one JSON line
each: 16 x 864 frames (BASELINE.json configs[1]) and a ragged batch of 16 with 200 .. 864 frames.

  legacy  Synthesizer.infer_batch, then convert_wav(normalize_wav(wav_denoised), int16) per utterance on the host
  pcm     Synthesizer.infer_batch_pcm (denoiser and int16 finishing as one launch sequence, one int16 copy back)

The legs alternate in one process, repetition by repetition, after a warm-up of both; each line gives the median, the
10th and 90th percentile and the extremes of the host clock around the call (both legs end with the arrays on the host,
so the clock covers all device work).  The legacy leg uses only what older checkouts have: on a tree without
``infer_batch_pcm`` the script runs that leg alone, which is how the baseline of a comparison is taken.  The last
repetition's arrays of the two legs are compared: they must be equal.

Two parts of the remaining time are measured on their own: ``noise_ms`` (the per-utterance seed resets and normal draws
that both legs make before the flow) and ``write_ms`` (scipy writing the batch's int16 wav files to a temporary folder).

  python tools/bench_synthesize.py [--reps 20] [--warmup 3] [--batch 16] [--frames 864] [--strength 0.0005]
"""
import argparse
import json
import os
import sys
import tempfile
import time

import numpy as np
import torch

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
sys.path.insert(0, ROOT)
from waveglow_amd import synthetic  # noqa: E402
from waveglow_amd.audio import convert_wav, normalize_wav  # noqa: E402
from waveglow_amd.checkpoint import CheckpointWaveglow  # noqa: E402
from waveglow_amd.hparams import HParams  # noqa: E402
from waveglow_amd.model import WaveGlow  # noqa: E402
from waveglow_amd.synthesizer import Synthesizer, init_global_seeds  # noqa: E402


def spread(ms):
  a = np.sort(np.asarray(ms))
  return {"median": float(np.median(a)), "p10": float(np.percentile(a, 10)), "p90": float(np.percentile(a, 90)),
          "min": float(a[0]), "max": float(a[-1]), "n": int(a.size)}


def leg_legacy(synth, mels, a):
  res = synth.infer_batch(mels, sigma=a.sigma, denoiser_strength=a.strength, seed=a.seed)
  return [convert_wav(normalize_wav(r.wav_denoised), np.int16) for r in res]


def leg_pcm(synth, mels, a):
  return [r.pcm for r in synth.infer_batch_pcm(mels, sigma=a.sigma, denoiser_strength=a.strength, seed=a.seed)]


def draw_noise(synth, frames, seed):
  """The draws both legs make before the flow (Synthesizer.infer_batch): seed reset, then the tensors of one utterance."""
  m, dev = synth.model, synth.device
  n_early = len([k for k in range(m.n_flows) if k % m.n_early_every == 0 and k > 0])
  for T in frames:
    L = T * 256 // m.n_group
    init_global_seeds(seed)
    torch.empty((1, m.n_remaining_channels, L), device=dev).normal_()
    for _ in range(n_early):
      torch.empty((1, m.n_early_size, L), device=dev).normal_()


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
  legs = {"legacy": leg_legacy}
  if hasattr(synth, "infer_batch_pcm"):
    legs["pcm"] = leg_pcm
  ragged = [int(round(v)) for v in np.linspace(a.min_frames, a.frames, a.batch)]
  ragged = ragged[1::2] + ragged[0::2]                                   # the longest is neither first nor last
  for name, frames in (("uniform", [a.frames] * a.batch), ("ragged", ragged)):
    mels = [synthetic.make_mel(1, T, seed=100 + i).to(dev) for i, T in enumerate(frames)]
    times = {k: [] for k in legs}
    last = {}
    for it in range(a.warmup + a.reps):
      for k, fn in legs.items():
        ms, last[k] = timed(lambda: fn(synth, mels, a), dev)
        if it >= a.warmup:
          times[k].append(ms)
    noise = [timed(lambda: draw_noise(synth, frames, a.seed), dev)[0] for _ in range(a.warmup + a.reps)][a.warmup:]
    with tempfile.TemporaryDirectory() as tmp:
      from scipy.io.wavfile import write
      def write_all():
        for i, x in enumerate(last["legacy"]):
          write(os.path.join(tmp, f"u{i}.wav"), hp.sampling_rate, x)
      writes = [timed(write_all, dev)[0] for _ in range(a.warmup + a.reps)][a.warmup:]
    out = {"shape": name, "batch": a.batch, "frames": frames if name == "ragged" else a.frames,
           "samples": 256 * sum(frames), "channels": a.channels, "denoiser_strength": a.strength,
           "ms": {k: spread(v) for k, v in times.items()}, "noise_ms": spread(noise), "write_ms": spread(writes)}
    if "pcm" in legs:
      out["legs_equal"] = bool(all(np.array_equal(x, y) for x, y in zip(last["legacy"], last["pcm"])))
    print(json.dumps(out), flush=True)
    if "pcm" in legs and not out["legs_equal"]:
      sys.exit("the two legs returned different samples")


if __name__ == "__main__":
  main()
