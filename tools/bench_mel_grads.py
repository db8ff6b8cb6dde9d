"""Timing of ``TacotronSTFT.mel_spectrogram_differentiable`` (the mel front-end with an audio gradient).  One JSON line per
shape and mode; shapes B x N: 16 x 221 184 (the audio of configs[1]) and 32 x 16 128 by default.

  p  plain mel, no graph (wg_stft_mel)
  f  mel_spectrogram_differentiable forward only (saved state, no backward)
  b  mel_spectrogram_differentiable forward + backward (d audio)
  t  for comparison, forward + backward of a torch autograd composition on the GPU with the conv-STFT as framing +
     GEMM: reflect F.pad, unfold, matmul, sqrt, matmul, clamp, log
  c  the same composition with F.conv1d for the conv-STFT (tests/test_mel_grads_cpu.py: mel_ref64 at fp32), as the
     test of the vocoder cycle runs it.  Not in the default modes: its first forward + backward at 16 x 221 184 did
     not finish within 7 minutes on the MI355X; give it --shapes 32x16128 and few steps

  r  mel_spectrogram_differentiable(y, lengths) forward only  } added by --lengths: B utterances spread evenly from
  l  the same, forward + backward                             } 200/864 of the row pitch to all of it, in whole frames
     of 256 samples (16 x 221 184: 200 ... 864 frames); shapes whose N is no multiple of 256 skip them

  python tools/bench_mel_grads.py [--shapes 16x221184,32x16128] [--steps 20] [--warmup 3] [--modes pfbt] [--lengths]

The modes of a shape run interleaved, step by step, in one process.  Each line gives the mean of the forward and of the
backward part (hipEvent milliseconds) with median, p10 and p90 over the steps after the warm-up, the GEMM work of one
direction (2 x 1056 x 1024 x B x F flops on the padded 1056-row basis) and its rate over the mean time.
"""
import argparse
import json
import os
import statistics
import sys

import torch
import torch.nn.functional as Fn

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from test_mel_grads_cpu import constants64, mel_ref64  # noqa: E402
from waveglow_amd.taco_stft import TacotronSTFT, TSTFTHParams  # noqa: E402


def mel_unfold(y, fwd, basis):
  """mel_ref64 with the conv-STFT as frames x basis^T (one GEMM each way under autograd)."""
  frames = Fn.pad(y[:, None, :], (512, 512), mode="reflect")[:, 0].unfold(-1, 1024, 256)    # [B, F, 1024]
  X = torch.matmul(frames, fwd.t()).transpose(1, 2)                                    # [B, 1026, F]
  p = X[:, :513] ** 2 + X[:, 513:] ** 2
  nz = p > 0
  mag = torch.where(nz, torch.where(nz, p, torch.ones_like(p)).sqrt(), torch.zeros_like(p))
  return torch.log(torch.clamp(torch.matmul(basis, mag), min=1e-5))


def spread_lengths(B, N):
  """B lengths in whole frames of 256 samples, evenly from 200/864 of the pitch to the pitch; None if N % 256."""
  if N % 256 or B < 2:
    return None
  T = N // 256
  lo = round(T * 200 / 864)
  return [256 * round(lo + (T - lo) * b / (B - 1)) for b in range(B)]


def run_once(taco, consts, y, g, mode, lens, ev):
  """One iteration of one mode: (forward ms, backward ms)."""
  torch.cuda.synchronize()
  ev[0].record()
  if mode == "p":
    with torch.no_grad():
      taco.mel_spectrogram_differentiable(y)
    ev[1].record()
  else:
    yg = y.detach().requires_grad_(True)
    fn = {"t": lambda t: mel_unfold(t, *consts), "c": lambda t: mel_ref64(t, *consts),
          "r": lambda t: taco.mel_spectrogram_differentiable(t, lens),
          "l": lambda t: taco.mel_spectrogram_differentiable(t, lens)}.get(mode, taco.mel_spectrogram_differentiable)
    mel = fn(yg)
    ev[1].record()
    if mode not in "fr":
      mel.backward(g)
    del mel
  ev[2].record()
  torch.cuda.synchronize()
  return ev[0].elapsed_time(ev[1]), ev[1].elapsed_time(ev[2])


def spread(v):
  s = sorted(v)
  pct = lambda q: s[min(len(s) - 1, max(0, round(q * (len(s) - 1))))]
  return {"median": statistics.median(v), "p10": pct(0.1), "p90": pct(0.9)}


def run_modes(taco, consts, y, g, modes, lens, steps, warmup):
  """All modes interleaved, step by step: one result per mode."""
  ev = [torch.cuda.Event(enable_timing=True) for _ in range(3)]
  times = {m: ([], []) for m in modes}
  for it in range(warmup + steps):
    for m in modes:
      tf, tb = run_once(taco, consts, y, g, m, lens, ev)
      if it >= warmup:
        times[m][0].append(tf)
        times[m][1].append(tb)
    if it % 5 == 0:
      print(json.dumps({"step": it, "of": warmup + steps}), flush=True)
  out = []
  for m in modes:
    tf, tb = times[m]
    both = [a + b for a, b in zip(tf, tb)]
    out.append({"mode": m, "ms_forward": sum(tf) / steps, "ms_backward": sum(tb) / steps,
                "ms_fwd_plus_bwd": sum(both) / steps, "forward": spread(tf), "backward": spread(tb),
                "fwd_plus_bwd": spread(both)})
  return out


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument("--shapes", default="16x221184,32x16128")
  ap.add_argument("--steps", type=int, default=20)
  ap.add_argument("--warmup", type=int, default=3)
  ap.add_argument("--modes", default="pfbt")
  ap.add_argument("--lengths", action="store_true", help="add the modes r and l: per-utterance lengths")
  a = ap.parse_args()
  dev = "cuda:0"
  taco = TacotronSTFT(TSTFTHParams(), dev)
  fwd, basis = constants64()
  consts = (fwd.float().to(dev), basis.float().to(dev))
  for shape in a.shapes.split(","):
    B, N = (int(v) for v in shape.split("x"))
    F = N // 256 + 1
    gen = torch.Generator(device=dev).manual_seed(1)
    y = torch.rand(B, N, device=dev, generator=gen) * 1.6 - 0.8
    g = torch.randn(B, 80, F, device=dev, generator=gen) / (B * 80 * F)
    gflop = 2.0 * 1056 * 1024 * B * F / 1e9
    ws = int(taco.lib.wg_stft_mel_grad_workspace_bytes(taco._h, B, N))
    lens = spread_lengths(B, N) if a.lengths else None
    modes = a.modes + ("rl" if lens is not None else "")
    print(json.dumps({"starting": modes, "batch": B, "n_samples": N}), flush=True)
    for out in run_modes(taco, consts, y, g, modes, lens, a.steps, a.warmup):
      mode = out["mode"]
      out.update(batch=B, n_samples=N, frames=F, gemm_gflop=gflop, workspace_bytes=ws)
      if mode in "rl":
        out.update(lengths=lens, samples_of_dense=sum(lens) / (B * N))
      if mode in "pfb":
        out["fwd_tflops"] = gflop / out["ms_forward"]
      if mode == "b":
        out["bwd_tflops"] = gflop / out["ms_backward"]
      print(json.dumps(out), flush=True)


if __name__ == "__main__":
  main()
