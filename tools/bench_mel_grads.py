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

  python tools/bench_mel_grads.py [--shapes 16x221184,32x16128] [--steps 20] [--warmup 3] [--modes pfbt]

Each line also gives the GEMM work of one direction (2 x 1056 x 1024 x B x F flops on the padded 1056-row basis) and
its rate over the measured time of the forward / backward part.
"""
import argparse
import json
import os
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


def run_mode(taco, consts, y, g, mode, steps, warmup):
  ev = [torch.cuda.Event(enable_timing=True) for _ in range(3)]
  t_f = t_b = 0.0
  for it in range(warmup + steps):
    torch.cuda.synchronize()
    ev[0].record()
    if mode == "p":
      with torch.no_grad():
        taco.mel_spectrogram_differentiable(y)
      ev[1].record()
    else:
      yg = y.detach().requires_grad_(True)
      fn = {"t": lambda t: mel_unfold(t, *consts), "c": lambda t: mel_ref64(t, *consts)}.get(
          mode, taco.mel_spectrogram_differentiable)
      mel = fn(yg)
      ev[1].record()
      if mode != "f":
        mel.backward(g)
      del mel
    ev[2].record()
    torch.cuda.synchronize()
    if it >= warmup:
      t_f += ev[0].elapsed_time(ev[1])
      t_b += ev[1].elapsed_time(ev[2])
  return {"mode": mode, "ms_forward": t_f / steps, "ms_backward": t_b / steps, "ms_fwd_plus_bwd": (t_f + t_b) / steps}


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument("--shapes", default="16x221184,32x16128")
  ap.add_argument("--steps", type=int, default=20)
  ap.add_argument("--warmup", type=int, default=3)
  ap.add_argument("--modes", default="pfbt")
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
    for mode in a.modes:
      print(json.dumps({"starting": mode, "batch": B, "n_samples": N}), flush=True)
      out = run_mode(taco, consts, y, g, mode, a.steps, a.warmup)
      out.update(batch=B, n_samples=N, frames=F, gemm_gflop=gflop, workspace_bytes=ws)
      if mode in "pfb":
        out["fwd_tflops"] = gflop / out["ms_forward"]
      if mode == "b":
        out["bwd_tflops"] = gflop / out["ms_backward"]
      print(json.dumps(out), flush=True)


if __name__ == "__main__":
  main()
