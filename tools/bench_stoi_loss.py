"""Timing of ``waveglow_amd.STOILoss`` (STOI / ESTOI as a training loss at 22 050 Hz: both sides resampled to 10 kHz, the five
kernels of wg_stoi, and in the backward the five of wg_stoi_backward and the transposed resampler).  Two shapes: 16 utterances
of 221 184 samples (864 mel frames, BASELINE.json configs[1]) and 32 of 16 128 (63 frames, the training segment).  The
target is white noise under a slow envelope that stays above the gate, the processed side the target plus noise.

  forward   ``crit.scores`` without grad mode: no graph, nothing saved
  saved     ``crit(audio, target)`` in grad mode: the forward that keeps the 10 kHz signal and the band spectra
  backward  ``loss.backward()`` of that forward
  torch     the STOI part of the same loss restated with torch fp64 operations on the device (torch.fft.rfft, boolean
            indexing for the gate, index_add for the overlap-add), forward + backward with respect to the 10 kHz signal the
            project's resampler made, utterance by utterance; the resampler's own gradient is not part of this leg
  infer     for scale: ``infer_differentiable(..., weight_grads=True)`` forward + backward at 32 x 63 frames, 256 channels

The legs alternate in one process, repetition by repetition, after warm-ups of all of them; each line gives the median and
the 10th and 90th percentile in ms (host clock around the call and a device synchronise).

  python tools/bench_stoi_loss.py [--reps 10] [--warmup 3] [--out profiles/stoi_loss_ab.txt]
"""
import argparse
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import _stoi_loss_oracle as lo  # noqa: E402
from waveglow_amd import STOILoss, metrics, resample, synthetic  # noqa: E402
from waveglow_amd.hparams import HParams  # noqa: E402
from waveglow_amd.model import WaveGlow  # noqa: E402

SHAPES = ((16, 221184), (32, 16128))


def timed(fn, dev):
  torch.cuda.synchronize(dev)
  t0 = time.perf_counter()
  out = fn()
  torch.cuda.synchronize(dev)
  return (time.perf_counter() - t0) * 1e3, out


def line(name, ms):
  a = np.asarray(ms)
  return f"  {name:9s} {np.median(a):9.3f} [{np.percentile(a, 10):.3f} - {np.percentile(a, 90):.3f}]  n = {a.size}"


def torch_scores(x, y, w, band_matrix):
  """(stoi, estoi) of one pair of fp64 10 kHz signals on the device, with a graph to y: steps 1 - 6 of the definition."""
  W, H, N = lo.W, lo.H, lo.N
  F0 = len(range(0, len(x) - W, H))
  xf, yf = x.unfold(0, W, H)[:F0] * w, y.unfold(0, W, H)[:F0] * w
  e = 20 * torch.log10(xf.norm(dim=1) + lo.EPS)
  keep = (e.max() - 40.0 - e) < 0
  K = int(keep.sum())
  idx = ((torch.arange(K, device=x.device) * H)[:, None] + torch.arange(W, device=x.device)[None, :]).reshape(-1)

  def spectra(frames):
    s = torch.zeros((K - 1) * H + W, dtype=torch.float64, device=x.device).index_add(0, idx, frames[keep].reshape(-1))
    z = torch.fft.rfft(s.unfold(0, W, H)[:K - 1] * w, n=lo.NFFT, dim=1)
    return lo.sqrt0((z.real ** 2 + z.imag ** 2) @ band_matrix).T                # [15, F]

  xs = spectra(xf).unfold(1, N, 1).permute(1, 0, 2)
  ys = spectra(yf).unfold(1, N, 1).permute(1, 0, 2)
  J = xs.shape[0]
  norm = lambda a: lo.sqrt0((a * a).sum(dim=2, keepdim=True))
  a, c = norm(xs) / (norm(ys) + lo.EPS) * ys, xs * lo.CLIP
  d = (lo._normalise(xs, 2) * lo._normalise(torch.where(a <= c, a, c), 2)).sum() / (lo.BANDS * J)
  est = (lo._normalise(lo._normalise(xs, 2), 1) * lo._normalise(lo._normalise(ys, 2), 1) / N).sum() / J
  return d, est


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument("--reps", type=int, default=10)
  ap.add_argument("--warmup", type=int, default=3)
  ap.add_argument("--infer-batch", type=int, default=32)
  ap.add_argument("--infer-frames", type=int, default=63)
  ap.add_argument("--out", default=None, help="also write the report to this file")
  a = ap.parse_args()
  dev = torch.device("cuda:0")
  sr = 22050
  crit = STOILoss(sampling_rate=sr, factor_stoi=1.0, factor_estoi=1.0, device=dev)
  w = torch.from_numpy(metrics.stoi_window()).to(dev)
  table = metrics.stoi_band_table()
  band_matrix = torch.zeros((lo.NFFT // 2 + 1, lo.BANDS), dtype=torch.float64)
  for b, (lo_bin, hi_bin) in enumerate(table.tolist()):
    band_matrix[lo_bin:hi_bin, b] = 1.0
  band_matrix = band_matrix.to(dev)

  hp = HParams()
  model = WaveGlow(hp)
  model.load_state_dict(synthetic.to_weightnorm_form(synthetic.make_state_dict(hp, seed=0)))
  model = model.to(dev).train().requires_grad_(True)
  mel = synthetic.make_mel(a.infer_batch, a.infer_frames, seed=7).to(dev)

  def leg_infer():
    model.zero_grad(set_to_none=True)
    audio = model.infer_differentiable(mel, 0.6, weight_grads=True)
    audio.backward(torch.full_like(audio, 1.0 / audio.numel()))

  report = [f"STOILoss at {sr} Hz, factor_stoi = factor_estoi = 1; median [p10 - p90] ms, {a.reps} repetitions after {a.warmup} "
            f"warm-ups, the legs alternating in one process"]
  for B, N in SHAPES:
    gen = torch.Generator().manual_seed(B)
    t = torch.arange(N) / sr
    env = 0.55 + 0.45 * torch.sin(2 * np.pi * 1.3 * t)                          # never 40 dB below its peak
    target = (0.1 * env * torch.randn((B, N), generator=gen)).to(dev)
    audio = (target + 0.03 * torch.randn((B, N), generator=gen).to(dev)).requires_grad_(True)
    up, down, _, _ = resample.resample_plan(sr, metrics.STOI_RATE)
    n10 = resample.out_len(N, up, down)
    with torch.no_grad():
      x10 = resample.resample(target, None, sr, metrics.STOI_RATE)[0].double()
      y10 = resample.resample(audio.detach(), None, sr, metrics.STOI_RATE)[0].double()
    state = {}

    def leg_forward():
      with torch.no_grad():
        state["scores"] = crit.scores(audio, target)

    def leg_saved():
      state["loss"] = crit(audio, target)

    def leg_backward():
      audio.grad = None
      state["loss"].backward()

    def leg_torch():
      y = y10.clone().requires_grad_(True)
      total = 0.0
      for b in range(B):
        d, e = torch_scores(x10[b], y[b], w, band_matrix)
        total = total + d + e
      (-(total / B)).backward()
      state["torch_loss"] = -(total / B).detach()

    times = {k: [] for k in ("forward", "saved", "backward", "torch", "infer")}
    for it in range(a.warmup + a.reps):
      ms = {"forward": timed(leg_forward, dev)[0], "saved": timed(leg_saved, dev)[0], "backward": timed(leg_backward, dev)[0],
            "torch": timed(leg_torch, dev)[0], "infer": timed(leg_infer, dev)[0]}
      if it >= a.warmup:
        for k, v in ms.items():
          times[k].append(v)
    rows = metrics.intelligibility_metrics_enqueue(target, None, audio.detach(), None, sr).cpu().numpy()
    report.append("")
    report.append(f"{B} x {N} samples ({n10} at 10 kHz; {int(rows[0, 2])} STOI frames, {int(rows[:, 3].min())} .. "
                  f"{int(rows[:, 3].max())} kept); forward keeps {crit.workspace_bytes(B, N) / 2 ** 20:.1f} MiB")
    report += [line(k, v) for k, v in times.items()]
    report.append(f"  loss {float(state['loss'].detach()):.9f}, torch restatement {float(state['torch_loss']):.9f}; "
                  f"scores equal intelligibility_metrics_enqueue bit for bit: "
                  f"{state['scores'].cpu().numpy().tobytes() == rows[:, :2].tobytes()}")
    report.append(f"  infer: {a.infer_batch} x {a.infer_frames} frames, 256 channels, weight_grads=True, forward + backward")
  text = "\n".join(report)
  print(text, flush=True)
  if a.out:
    with open(a.out, "w") as f:
      f.write(text + "\n")


if __name__ == "__main__":
  main()
