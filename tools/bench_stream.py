"""Timing of streaming synthesis (``Synthesizer.open_stream`` / ``stream_step``) beside whole-utterance synthesis.
256 channels, the default depth (12 flows x 8 layers), utterances of 864 frames, denoiser on; 1 and 16 sessions at
``chunk_frames`` 32 and 64.

  first_chunk   from ``open_stream(total_frames=864)`` (the noise draw of the whole utterance included) over the push of
                the first ``C + Hr`` frames (already on the device) to the first chunk's int16 samples on the host
  step          one steady-state step (a chunk whose window has the whole halo on both sides), int16 samples on the host
  slicing       the same step with the windows formed and the chunks cropped by torch slicing instead of
                ``wg_stream_gather`` / ``wg_stream_emit``, the fp32 interiors (raw and denoised) copied back: what the two
                kernels buy
  whole         ``infer_batch_pcm`` on the whole utterances

The legs alternate in one process, repetition by repetition, after a warm-up of all of them; every time is a host clock
around work that ends in a device synchronise.  One JSON line per configuration with the median, the 10th and 90th
percentile and the extremes of every leg.

  python tools/bench_stream.py [--reps 10] [--warmup 3] [--frames 864] [--channels 256] [--sessions 1,16] [--chunks 32,64]
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
from waveglow_amd.checkpoint import CheckpointWaveglow  # noqa: E402
from waveglow_amd.hparams import HParams  # noqa: E402
from waveglow_amd.model import WaveGlow  # noqa: E402
from waveglow_amd.synthesizer import Synthesizer  # noqa: E402

STRENGTH = 0.01


def spread(ms):
  a = np.sort(np.asarray(ms))
  return {"median": float(np.median(a)), "p10": float(np.percentile(a, 10)), "p90": float(np.percentile(a, 90)),
          "min": float(a[0]), "max": float(a[-1]), "n": int(a.size)}


def slicing_step(synth, sessions):
  """What ``stream_step`` does for these sessions, with torch slicing in place of the two kernels and fp32 interiors
  copied back.  Does not advance the sessions."""
  model, dev = synth.model, synth.device
  plans = [s.next_plan() for s in sessions]
  B = len(sessions)
  w_max = max(s.chunk_frames + s.Hl + s.Hr for s in sessions)
  mel = torch.zeros((B, sessions[0].n_mel, w_max), device=dev)
  zi = torch.zeros((B, sessions[0].n_rem, 32 * w_max), device=dev)
  ze = [torch.zeros((B, sessions[0].n_early_size, 32 * w_max), device=dev) for _ in range(sessions[0].n_early)]
  for b, (s, p) in enumerate(zip(sessions, plans)):
    n = p.w1 - p.w0
    mel[b, :, :n] = s._mel[:, p.w0:p.w1]
    zi[b, :, :32 * n] = s._z_init[0, :, 32 * p.w0:32 * p.w1]
    for dst, src in zip(ze, s._z_early):
      dst[b, :, :32 * n] = src[0, :, 32 * p.w0:32 * p.w1]
  frames = [p.w1 - p.w0 for p in plans]
  lengths = [256 * f for f in frames]
  with torch.no_grad():
    audio = model.infer_with_noise(mel, zi, ze, sessions[0].sigma, frames=torch.tensor(frames, dtype=torch.int32))
    den = torch.empty_like(audio)
    synth.denoiser.run_ragged(audio, lengths, torch.tensor(lengths, dtype=torch.int32).to(dev), STRENGTH, den)
  out = []
  for b, p in enumerate(plans):
    out.append((audio[b, p.offset:p.offset + p.count].cpu(), den[b, p.offset:p.offset + p.count].cpu()))
  return out


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument("--reps", type=int, default=10)
  ap.add_argument("--warmup", type=int, default=3)
  ap.add_argument("--frames", type=int, default=864)
  ap.add_argument("--channels", type=int, default=256)
  ap.add_argument("--sessions", type=str, default="1,16")
  ap.add_argument("--chunks", type=str, default="32,64")
  a = ap.parse_args()
  dev = torch.device("cuda:0")
  hp = HParams(n_channels=a.channels)
  m = WaveGlow(hp)
  m.load_state_dict(synthetic.to_weightnorm_form(synthetic.make_state_dict(hp, seed=0)))
  synth = Synthesizer(CheckpointWaveglow.from_instances(m, None, hp, 1), device=dev)
  T = a.frames

  def timed(fn):
    torch.cuda.synchronize(dev)
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize(dev)
    return (time.perf_counter() - t0) * 1e3

  for n in [int(x) for x in a.sessions.split(",")]:
    mels = [synthetic.make_mel(1, T, seed=5 + i)[0].to(dev) for i in range(n)]
    for C in [int(x) for x in a.chunks.split(",")]:
      def open_all(upto):
        ss = [synth.open_stream(denoiser_strength=STRENGTH, chunk_frames=C, seed=i, total_frames=T) for i in range(n)]
        for s, mel in zip(ss, mels):
          s.push(mel[:, :upto])
        return ss
      full = open_all(T)
      for s in full:
        s.close()
      Hl, Hr = full[0].Hl, full[0].Hr
      j = -(-Hl // C)                                      # the first chunk with the whole halo on its left
      assert (j + 1) * C + Hr <= T

      def at_j():
        for s in full:
          s.next_chunk = j

      def first_chunk():
        ss = open_all(C + Hr)
        res = synth.stream_step(ss)
        assert all(r is not None and r.start_sample == 0 for r in res)

      def step():
        at_j()
        res = synth.stream_step(full)
        assert all(r.pcm.size == 256 * C for r in res)

      def slicing():
        at_j()
        slicing_step(synth, full)

      legs = {"first_chunk": first_chunk, "step": step, "slicing": slicing,
              "whole": lambda: synth.infer_batch_pcm([x[None] for x in mels], denoiser_strength=STRENGTH)}
      times = {k: [] for k in legs}
      for it in range(a.warmup + a.reps):
        for k, fn in legs.items():
          ms = timed(fn)
          if it >= a.warmup:
            times[k].append(ms)
      print(json.dumps({"sessions": n, "chunk_frames": C, "frames": T, "channels": a.channels, "window_frames": C + Hl + Hr,
                        "ms": {k: spread(v) for k, v in times.items()}}), flush=True)


if __name__ == "__main__":
  main()
