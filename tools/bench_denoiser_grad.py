"""Timing of ``Denoiser.forward_differentiable`` (the denoiser with an audio gradient).  One JSON line per shape and leg;
shapes B x N: 16 x 221 184 (the audio of configs[1]) and 32 x 16 128 by default.

  p  Denoiser.forward, no graph (wg_stft_denoise)
  f  forward_differentiable forward only (wg_stft_denoise_forward_saved: the raw spectrum is kept)
  b  forward_differentiable forward + backward (d audio); the backward part is timed on its own
  t  for comparison, forward + backward of the same function as a torch autograd composition in fp32 on the device:
     reflect F.pad, F.conv1d with the forward basis, magnitude, subtract, clamp, recombine, F.conv_transpose1d with the
     inverse basis, window-sum-square, crop.  Skipped (reported as "not measured") for a shape with more than
     --torch-max-samples samples: tools/bench_mel_grads.py found that F.conv1d with this basis did not finish its first
     step at 16 x 221 184 within 7 minutes

  python tools/bench_denoiser_grad.py [--shapes 16x221184,32x16128] [--steps 10] [--warmup 3] [--legs pfbt]
                                      [--strength 0.1] [--torch-max-samples 1000000]

The legs of a shape run alternating, step by step, in one process.  Each line gives median, p10 and p90 (hipEvent
milliseconds) of the forward part, the backward part and their sum over the steps after the warm-up, and the GEMM work
of one transform (2 x 1056 x 1024 x B x F flops on the padded 1056-row basis; the forward runs two, the backward two more).
"""
import argparse
import json
import os
import statistics
import sys

import numpy as np
import torch
import torch.nn.functional as Fn

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
sys.path.insert(0, ROOT)
from waveglow_amd import Denoiser  # noqa: E402
from waveglow_amd.denoiser import stft_bases  # noqa: E402
from waveglow_amd.taco_stft import TSTFTHParams  # noqa: E402


class _Vocoder:
  """What ``Denoiser.__init__`` asks of a vocoder: the timing does not depend on the bias it yields."""

  def __init__(self, dev):
    self.upsample = type("Up", (), {"weight": torch.zeros(1, device=dev)})()
    self.dev = dev

  def infer(self, mel, sigma):
    gen = torch.Generator(device=self.dev).manual_seed(0)
    return torch.randn(1, 256 * mel.shape[2], device=self.dev, generator=gen) * 0.05


def denoise_torch(x, fwd, inv, wsq, bias, strength):
  """Denoiser.forward as torch ops with a graph to x (the true gradient: the phase is not detached)."""
  re_im = Fn.conv1d(Fn.pad(x[:, None, :], (512, 512), mode="reflect"), fwd, stride=256)
  re, im = re_im[:, :513], re_im[:, 513:]
  p = re * re + im * im
  nz = p > 0
  mag = torch.where(nz, torch.where(nz, p, torch.ones_like(p)).sqrt(), torch.zeros_like(p))
  safe = torch.where(nz, mag, torch.ones_like(mag))
  md = torch.clamp(mag - bias[None, :, None] * strength, min=0.0)
  rec = torch.cat([md * torch.where(nz, re / safe, torch.ones_like(re)), md * torch.where(nz, im / safe, torch.zeros_like(im))], 1)
  full = Fn.conv_transpose1d(rec, inv, stride=256)
  F = re.shape[2]
  ws = Fn.conv_transpose1d(torch.ones(1, 1, F, device=x.device), wsq[None, None, :], stride=256)[0, 0]
  tiny = float(np.finfo(np.float32).tiny)
  full = torch.where(ws > tiny, full / torch.where(ws > tiny, ws, torch.ones_like(ws)), full) * 4.0
  return full[:, :, 512:-512]


def run_once(den, consts, x, g, leg, strength, ev):
  """One iteration of one leg: (forward ms, backward ms)."""
  torch.cuda.synchronize()
  ev[0].record()
  if leg == "p":
    den(x, strength)
    ev[1].record()
  else:
    xg = x.detach().requires_grad_(True)
    out = denoise_torch(xg, *consts, strength) if leg == "t" else den.forward_differentiable(xg, strength)
    ev[1].record()
    if leg != "f":
      out.backward(g)
    del out
  ev[2].record()
  torch.cuda.synchronize()
  return ev[0].elapsed_time(ev[1]), ev[1].elapsed_time(ev[2])


def spread(v):
  s = sorted(v)
  pct = lambda q: s[min(len(s) - 1, max(0, round(q * (len(s) - 1))))]
  return {"median": statistics.median(v), "p10": pct(0.1), "p90": pct(0.9)}


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument("--shapes", default="16x221184,32x16128")
  ap.add_argument("--steps", type=int, default=10)
  ap.add_argument("--warmup", type=int, default=3)
  ap.add_argument("--legs", default="pfbt")
  ap.add_argument("--strength", type=float, default=0.1)
  ap.add_argument("--torch-max-samples", type=int, default=1000000)
  a = ap.parse_args()
  dev = "cuda:0"
  den = Denoiser(_Vocoder(dev), TSTFTHParams(), "zeros", dev)
  fwd, inv, wsq = (torch.from_numpy(v).to(dev) for v in stft_bases())
  consts = (fwd[:, None, :], inv[:, None, :], wsq, den.bias_spec.reshape(-1))
  ev = [torch.cuda.Event(enable_timing=True) for _ in range(3)]
  for shape in a.shapes.split(","):
    B, N = (int(v) for v in shape.split("x"))
    F = N // 256 + 1
    gen = torch.Generator(device=dev).manual_seed(1)
    x = torch.rand(B, N, device=dev, generator=gen) * 1.6 - 0.8
    g = torch.randn(B, 1, N, device=dev, generator=gen) / (B * N)
    legs = a.legs
    if "t" in legs and B * N > a.torch_max_samples:
      legs = legs.replace("t", "")
      print(json.dumps({"leg": "t", "batch": B, "n_samples": N, "result": "not measured",
                        "why": f"more than {a.torch_max_samples} samples (--torch-max-samples)"}), flush=True)
    print(json.dumps({"starting": legs, "batch": B, "n_samples": N}), flush=True)
    times = {m: ([], []) for m in legs}
    for it in range(a.warmup + a.steps):
      for m in legs:
        tf, tb = run_once(den, consts, x, g, m, a.strength, ev)
        if it >= a.warmup:
          times[m][0].append(tf)
          times[m][1].append(tb)
    for m in legs:
      tf, tb = times[m]
      out = {"leg": m, "batch": B, "n_samples": N, "frames": F, "steps": a.steps, "forward": spread(tf),
             "backward": spread(tb), "fwd_plus_bwd": spread([p + q for p, q in zip(tf, tb)]),
             "gemm_gflop_per_transform": 2.0 * 1056 * 1024 * B * F / 1e9,
             "grad_workspace_bytes": den.grad_workspace_bytes(B, N)}
      print(json.dumps(out), flush=True)


if __name__ == "__main__":
  main()
