"""Timing of the device resampler beside the host's: 16 utterances of 10 s from 48 000 to 22 050 Hz and from 22 050 to
48 000 Hz, int16 as a wav file holds them.  One JSON line per direction.

  device    upload of the int16 batch + resample.resample on the device (wg_resample), synchronised: what
            ``--resample-inputs`` does with a batch of files
  host      scipy.signal.resample_poly of every utterance on the host, on at most 16 threads, + the upload of its fp32
            result: what a preprocessing pass over the corpus does
  kernel    the wg_resample launch alone, between two device events (audio and lengths already on the device)

The legs alternate in one process, repetition by repetition, after a warm-up of all of them.  Each line gives the median,
the 10th and 90th percentile and the extremes, and the largest distance between the two results in units of the bound of
tests/test_gpu_resample.py.

  python tools/bench_resample.py [--reps 20] [--warmup 3] [--batch 16] [--seconds 10] [--threads 16]
"""
import argparse
import json
import os
import sys
import time
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import torch

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
sys.path.insert(0, ROOT)
from waveglow_amd import resample as rs  # noqa: E402


def spread(ms):
  a = np.sort(np.asarray(ms))
  return {"median": float(np.median(a)), "p10": float(np.percentile(a, 10)), "p90": float(np.percentile(a, 90)),
          "min": float(a[0]), "max": float(a[-1]), "n": int(a.size)}


def main():
  from scipy.signal import resample_poly
  ap = argparse.ArgumentParser()
  ap.add_argument("--reps", type=int, default=20)
  ap.add_argument("--warmup", type=int, default=3)
  ap.add_argument("--batch", type=int, default=16)
  ap.add_argument("--seconds", type=float, default=10.0)
  ap.add_argument("--threads", type=int, default=16)
  a = ap.parse_args()
  if a.reps < 1:
    ap.error("--reps must be at least 1")
  dev = torch.device("cuda:0")
  threads = max(1, min(a.threads, 16))
  pool = ThreadPoolExecutor(max_workers=threads)
  for sr_in, sr_out in ((48000, 22050), (22050, 48000)):
    up, down, half, taps = rs.resample_plan(sr_in, sr_out)
    n = int(round(a.seconds * sr_in))
    pcm = np.random.default_rng(sr_in).integers(-29000, 29001, (a.batch, n)).astype(np.int16)
    lens = [n] * a.batch
    state = {}

    def leg_device():
      torch.cuda.synchronize(dev)
      t0 = time.perf_counter()
      state["dev"], _ = rs.resample(torch.from_numpy(pcm).to(dev), lens, sr_in, sr_out)
      torch.cuda.synchronize(dev)
      return (time.perf_counter() - t0) * 1e3

    def leg_host():
      torch.cuda.synchronize(dev)
      t0 = time.perf_counter()
      rows = list(pool.map(lambda row: resample_poly(row.astype(np.float64) / 32768.0, up, down), pcm))
      state["ref"] = np.stack(rows)
      state["host"] = torch.from_numpy(state["ref"].astype(np.float32)).to(dev)
      torch.cuda.synchronize(dev)
      return (time.perf_counter() - t0) * 1e3

    audio_dev = torch.from_numpy(pcm).to(dev)
    lens_dev = torch.tensor(lens, dtype=torch.int32).to(dev)
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]

    def leg_kernel():
      stream = torch.cuda.current_stream(dev)
      ev[0].record(stream)
      rs.resample_enqueue(audio_dev, lens_dev, sr_in, sr_out)
      ev[1].record(stream)
      torch.cuda.synchronize(dev)
      return ev[0].elapsed_time(ev[1])

    times = {k: [] for k in ("device", "host", "kernel")}
    for it in range(a.warmup + a.reps):
      ms = {"device": leg_device(), "host": leg_host(), "kernel": leg_kernel()}
      if it >= a.warmup:
        for k, v in ms.items():
          times[k].append(v)
    got, ref = state["dev"].cpu().numpy().astype(np.float64), state["ref"]
    L = max(float(np.abs(taps[p::up]).sum()) for p in range(up))
    tol = 2.0 ** -24 * np.abs(ref) + 1e-12 * float(np.abs(pcm).max() / 32768.0) * L
    out = {"sr_in": sr_in, "sr_out": sr_out, "up": up, "down": down, "batch": a.batch, "n_in": n, "n_out": int(got.shape[1]),
           "host_threads": threads, "ms": {k: spread(v) for k, v in times.items()},
           "largest_distance_over_bound": float(np.max(np.abs(got - ref) / tol))}
    out["host_over_device"] = out["ms"]["host"]["median"] / out["ms"]["device"]["median"]
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
  main()
