"""What the data loader adds to a training step: the legacy path (``DataLoader(MelLoader)``, one utterance at a time)
against the device-resident path (``train(..., device_dataset=True)``, waveglow_amd/device_data.py), on a seeded folder of
int16 wavs written here: 64 files of 1 - 3 s and one shorter than the segment.  Default model (256 channels), batch 32 x
16 000 samples.

  (a) batch-ready time: host clock from just after a device synchronise to the point where the next ``(mel, audio)`` is
      complete on the device (a synchronise at the end).  Legs: legacy with ``cache_wavs`` off and on, device loader
      without prefetch, and device loader with the batch prefetched before the first synchronise (what is left on the
      critical path) together with the host time of that ``prefetch()`` call.  The legs alternate batch by batch.
  (b) wall time per optimiser step of ``train()`` itself: the time between the per-step log records of one ``train(...,
      max_iterations=warmup + block)`` call, the first ``warmup`` steps dropped.  The legs alternate call by call until
      each has ``--steps`` timed steps.  No checkpoint or validation falls into the timed steps.

Each line gives the median and the 10th - 90th percentile range.  On a tree without waveglow_amd/device_data.py only the
legacy legs run.

  python tools/bench_train_loop.py [--steps 40] [--block 10] [--warmup 3] [--ready-reps 30] [--out FILE]
"""
import argparse
import logging
import os
import shutil
import sys
import tempfile
import time
from pathlib import Path

import numpy as np
import torch
from scipy.io.wavfile import write as write_wav

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
sys.path.insert(0, ROOT)
from waveglow_amd.hparams import HParams  # noqa: E402
from waveglow_amd.training import load_dataset, prepare_trainloader, train  # noqa: E402

try:
  from waveglow_amd.device_data import DeviceBatchLoader  # noqa: E402
except ImportError:
  DeviceBatchLoader = None

SR = 22050


def write_folder(folder: Path, n: int, seed: int, segment: int, short: bool):
  folder.mkdir(parents=True)
  rng = np.random.default_rng(seed)
  lens = [int(rng.integers(SR, 3 * SR + 1)) for _ in range(n)] + ([segment // 2] if short else [])
  for i, m in enumerate(lens):
    write_wav(folder / f"utt_{i:03d}.wav", SR, np.int16(rng.uniform(-0.3, 0.3, size=m) * 32767))


def spread(ms):
  a = np.asarray(ms)
  return f"median {np.median(a):8.3f}  p10 {np.percentile(a, 10):8.3f}  p90 {np.percentile(a, 90):8.3f}  n {a.size}"


def endless(loader):
  while True:
    for batch in loader:
      yield batch


def ready_times(entries, hp, dev, reps, warmup):
  """(a): milliseconds per leg, the legs taking turns batch by batch."""
  import dataclasses
  legs = {"legacy": endless(prepare_trainloader(hp, entries, dev)),
          "legacy cache_wavs": endless(prepare_trainloader(dataclasses.replace(hp, cache_wavs=True), entries, dev))}
  pre = None
  if DeviceBatchLoader is not None:
    legs["device"] = endless(DeviceBatchLoader(entries, hp, dev, drop_last=True))
    pre = DeviceBatchLoader(entries, hp, dev, drop_last=True)
    legs["device prefetched"] = endless(pre)
  times = {k: [] for k in legs}
  times_pre = []
  for it in range(warmup + reps):
    for name, gen in legs.items():
      if name == "device prefetched":
        t0 = time.perf_counter()
        pre.prefetch()
        t_pre = (time.perf_counter() - t0) * 1e3
      torch.cuda.synchronize(dev)
      t0 = time.perf_counter()
      batch = next(gen)
      torch.cuda.synchronize(dev)
      ms = (time.perf_counter() - t0) * 1e3
      del batch
      if it >= warmup:
        times[name].append(ms)
        if name == "device prefetched":
          times_pre.append(t_pre)
  if times_pre:
    times["  its prefetch() call, host"] = times_pre
  return times


class StepClock(logging.Handler):
  """perf_counter at every per-step record of train()."""

  def __init__(self):
    super().__init__(level=logging.INFO)
    self.stamps = []

  def emit(self, record):
    if "Total iteration" in record.getMessage():
      self.stamps.append(time.perf_counter())


def step_times(trn, val, custom, dev, steps, block, warmup, ckp_root: Path):
  """(b): milliseconds per optimiser step of train(), per leg."""
  legs = [("legacy", {}, {}), ("legacy cache_wavs", {"cache_wavs": "True"}, {})]
  if DeviceBatchLoader is not None:
    legs.append(("device_dataset", {}, {"device_dataset": True}))
  times = {name: [] for name, _, _ in legs}
  log = logging.getLogger("waveglow_amd.training")
  old = log.level
  log.setLevel(logging.INFO)
  call = 0
  try:
    while any(len(v) < steps for v in times.values()):
      for name, extra, kw in legs:
        clock = StepClock()
        log.addHandler(clock)
        try:
          call += 1
          train(dict(custom, **extra), None, trn, val, ckp_root / f"ckp_{call}", None, None, dev,
                max_iterations=warmup + block, **kw)
        finally:
          log.removeHandler(clock)
          shutil.rmtree(ckp_root / f"ckp_{call}", ignore_errors=True)      # the checkpoint of iteration 1
        d = np.diff(clock.stamps) * 1e3                  # d[i]: step i + 2 of the call
        times[name].extend(d[warmup - 1:].tolist())
  finally:
    log.setLevel(old)
  return {k: v[:steps] for k, v in times.items()}


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument("--steps", type=int, default=40)
  ap.add_argument("--block", type=int, default=10)
  ap.add_argument("--warmup", type=int, default=3)
  ap.add_argument("--ready-reps", type=int, default=30)
  ap.add_argument("--batch", type=int, default=32)
  ap.add_argument("--segment", type=int, default=16000)
  ap.add_argument("--channels", type=int, default=256)
  ap.add_argument("--files", type=int, default=64)
  ap.add_argument("--out", type=Path, default=None, help="also write the table to this file")
  a = ap.parse_args()
  if a.warmup < 2:
    ap.error("--warmup must be at least 2 (step 2 waits for the checkpoint and the validation of iteration 1)")
  dev = torch.device("cuda:0")
  lines = []

  def say(s=""):
    print(s, flush=True)
    lines.append(s)

  with tempfile.TemporaryDirectory() as tmp:
    tmp = Path(tmp)
    write_folder(tmp / "trn", a.files, 1, a.segment, short=True)
    write_folder(tmp / "val", 2, 2, a.segment, short=False)
    trn, val = load_dataset(tmp / "trn"), load_dataset(tmp / "val")
    hp = HParams(batch_size=a.batch, segment_length=a.segment, n_channels=a.channels)
    say(f"train loader A/B on {torch.cuda.get_device_name(dev)}: {len(trn)} int16 wavs, batch {a.batch} x {a.segment}, "
        f"{a.channels} channels" + ("" if DeviceBatchLoader is not None else "  (no device loader in this tree)"))
    say()
    say(f"(a) batch-ready time, ms (host clock, synchronise .. next (mel, audio) complete), {a.ready_reps} batches per leg")
    for name, ms in ready_times(trn, hp, dev, a.ready_reps, a.warmup).items():
      say(f"  {name:30s} {spread(ms)}")
    say()
    say(f"(b) wall time per optimiser step of train(), ms; blocks of {a.block} steps behind {a.warmup} warm-up steps")
    custom = {"batch_size": str(a.batch), "segment_length": str(a.segment), "n_channels": str(a.channels),
              "epochs": "100000", "iters_per_checkpoint": "0", "epochs_per_checkpoint": "0"}
    res = step_times(trn, val, custom, dev, a.steps, a.block, a.warmup, tmp)
    for name, ms in res.items():
      say(f"  {name:30s} {spread(ms)}")
    if "device_dataset" in res:
      new, legacy = np.asarray(res["device_dataset"]), np.asarray(res["legacy"])
      faster = np.percentile(new, 90) < np.percentile(legacy, 10)
      say(f"  device_dataset p90 below legacy p10: {bool(faster)}")
  if a.out is not None:
    a.out.parent.mkdir(parents=True, exist_ok=True)
    a.out.write_text("\n".join(lines) + "\n")


if __name__ == "__main__":
  main()
