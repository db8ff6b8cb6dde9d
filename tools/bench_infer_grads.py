"""Timing of ``WaveGlow.infer_differentiable`` (synthesis with gradients for mel and noise) at BASELINE config 4 shapes
(per GPU: batch 32 x 63 mel frames, 256 channels, fp32 I/O), synthetic data / random-init weights, frozen model.  One JSON
line per mode:

  p  plain infer_with_noise (fp32), no graph
  f  infer_differentiable, forward only (saved state, no backward)
  m  infer_differentiable forward + backward with d mel
  z  infer_differentiable forward + backward with d mel and d z (z_init and every z_early)
  c  for comparison: the frozen training direction, WaveGlow.forward + WaveGlowLoss + backward with d mel and d audio
     (tools/bench_input_grads.py mode c)

  python tools/bench_infer_grads.py [--batch 32] [--frames 63] [--steps 5] [--warmup 2] [--modes pfmzc] [--rounds 1] [--weights [--weights-modes w,wr,ws,fs]]

``--weights`` adds, after the modes above in every round, the weight-gradient path (``infer_differentiable(...,
weight_grads=True)``, gradients for all 686 parameters, no input gradient) on the same model made trainable for the
duration -- one model, one engine: a second engine's streams would share the process's hardware queues with the first's
and the weight-gradient stream would no longer run beside the chain:

  w   forward + backward, full save            wr  the same with activation recomputation
  ws  forward of the step after a weight change (the 1x1 inverses follow on the device, no engine re-finalisation)
  fs  for comparison: forward of the frozen path (mode f) after the same weight change (re-finalises the inference engine)

The first line also reports wg_train_workspace_bytes of the synthesis geometry.  ``--headroom`` adds one line on the fp16
gradient planes: for loss = mean(audio * r), r ~ N(0, 1), the automatic loss scale, the largest |d z| / |d mel| it gives,
and the smallest power-of-two scale at which the planes overflow (model.grad_finite false).
"""
import argparse
import json
import math
import os
import sys

import torch

sys.path.insert(0, os.path.abspath(os.path.join(os.path.dirname(__file__), "..")))
from waveglow_amd import synthetic  # noqa: E402
from waveglow_amd.hparams import HParams  # noqa: E402
from waveglow_amd.model import WaveGlow, WaveGlowLoss  # noqa: E402


def run_mode(model, mel, zi, ze, wav, mode, sigma, steps, warmup):
  ev = [torch.cuda.Event(enable_timing=True) for _ in range(3)]
  t_f = t_b = 0.0
  for it in range(warmup + steps):
    torch.cuda.synchronize()
    ev[0].record()
    if mode == "p":
      with torch.no_grad():
        model.infer_with_noise(mel, zi, ze, sigma)
      ev[1].record()
    elif mode == "c":
      m = mel.detach().requires_grad_(True)
      a = wav.detach().requires_grad_(True)
      loss = WaveGlowLoss(1.0)(model((m, a)), None)
      ev[1].record()
      loss.backward()
    else:
      m = mel.detach().requires_grad_(True)
      z_i = zi.detach().requires_grad_(mode == "z")
      z_e = [z.detach().requires_grad_(mode == "z") for z in ze]
      audio = model.infer_differentiable(m, sigma, z_init=z_i, z_early=z_e)
      ev[1].record()
      if mode != "f":
        audio.backward(torch.full_like(audio, 1.0 / audio.numel()))
      del audio
    ev[2].record()
    torch.cuda.synchronize()
    if it >= warmup:
      t_f += ev[0].elapsed_time(ev[1])
      t_b += ev[1].elapsed_time(ev[2])
  return {"mode": mode, "ms_forward": t_f / steps, "ms_backward": t_b / steps, "ms_fwd_plus_bwd": (t_f + t_b) / steps}


def run_weights(model, mel, zi, ze, mode, sigma, steps, warmup):
  """``--weights`` modes (see the module docstring): the model is trainable for w / wr / ws, frozen again afterwards."""
  ev = [torch.cuda.Event(enable_timing=True) for _ in range(3)]
  t_f = t_b = 0.0
  model.recompute_activations = mode == "wr"
  model.requires_grad_(mode != "fs")
  for it in range(warmup + steps):
    if mode in ("ws", "fs"):
      with torch.no_grad():
        model.upsample.bias.add_(0.0)           # what an optimiser step does to the parameter versions
    m = mel.detach().requires_grad_(mode == "fs")
    model.zero_grad(set_to_none=True)
    torch.cuda.synchronize()
    ev[0].record()
    audio = model.infer_differentiable(m, sigma, z_init=zi, z_early=ze, weight_grads=mode != "fs")
    ev[1].record()
    if mode in ("w", "wr"):
      audio.backward(torch.full_like(audio, 1.0 / audio.numel()))
    del audio
    ev[2].record()
    torch.cuda.synchronize()
    if it >= warmup:
      t_f += ev[0].elapsed_time(ev[1])
      t_b += ev[1].elapsed_time(ev[2])
  model.recompute_activations = False
  model.zero_grad(set_to_none=True)
  model.requires_grad_(False)
  out = {"mode": mode, "ms_forward": t_f / steps}
  if mode in ("w", "wr"):
    out.update(ms_backward=t_b / steps, ms_fwd_plus_bwd=(t_f + t_b) / steps)
  return out


def headroom(model, mel, zi, ze, sigma):
  r = torch.randn(mel.shape[0], 256 * mel.shape[2], device=mel.device, generator=torch.Generator(device=mel.device).manual_seed(1))

  def step(scale):
    if scale:
      model.grad_scale = float(scale)
    elif hasattr(model, "grad_scale"):
      del model.grad_scale
    m = mel.detach().requires_grad_(True)
    z_i = zi.detach().requires_grad_(True)
    z_e = [z.detach().requires_grad_(True) for z in ze]
    audio = model.infer_differentiable(m, sigma, z_init=z_i, z_early=z_e)
    (audio * r).mean().backward()
    return bool(model.grad_finite), m.grad, [z_i.grad] + [z.grad for z in z_e]

  ok, g_mel, g_z = step(0)
  auto = 2.0 ** round(math.log2(r.numel()))
  first_bad = None
  for e in range(int(math.log2(auto)) + 1, 64):
    if not step(2.0 ** e)[0]:
      first_bad = e
      break
  step(0)
  return {"headroom": True, "finite_at_auto_scale": ok, "auto_scale_log2": math.log2(auto),
          "max_abs_d_audio": 1.0 / r.numel() * float(r.abs().max()),
          "max_abs_d_z": max(float(g.abs().max()) for g in g_z), "max_abs_d_mel": float(g_mel.abs().max()),
          "first_overflow_scale_log2": first_bad}


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument("--batch", type=int, default=32)
  ap.add_argument("--frames", type=int, default=63)
  ap.add_argument("--sigma", type=float, default=0.6)
  ap.add_argument("--steps", type=int, default=5)
  ap.add_argument("--warmup", type=int, default=2)
  ap.add_argument("--modes", default="pfmzc")
  ap.add_argument("--rounds", type=int, default=1)
  ap.add_argument("--headroom", action="store_true")
  ap.add_argument("--weights", action="store_true")
  ap.add_argument("--weights-modes", default="w,wr,ws,fs", help="comma-separated subset of the --weights modes")
  a = ap.parse_args()
  hp = HParams()
  model = WaveGlow(hp)
  model.load_state_dict(synthetic.to_weightnorm_form(synthetic.make_state_dict(hp, seed=0)))
  model = model.to("cuda:0").eval().requires_grad_(False)
  B, T = a.batch, a.frames
  L = 32 * T
  mel = synthetic.make_mel(B, T, seed=7).cuda()
  gen = torch.Generator(device="cuda:0").manual_seed(5)
  zi = torch.randn(B, model.n_remaining_channels, L, device="cuda:0", generator=gen)
  n_early = sum(1 for k in range(hp.n_flows) if k % hp.n_early_every == 0 and k > 0)
  ze = [torch.randn(B, hp.n_early_size, L, device="cuda:0", generator=gen) for _ in range(n_early)]
  wav = (torch.rand(B, 256 * T - 128, generator=torch.Generator().manual_seed(3)) * 0.6 - 0.3).cuda()   # 16000 at T = 63
  eng = model._get_engine(mel.device, need_weights=bool(a.modes))      # --modes "": the frozen engine stays unfinalised
  ws = int(eng.lib.wg_train_workspace_bytes(eng.handle, B, T, 256 * T, 0))
  print(json.dumps({"workspace_bytes": ws, "bytes_per_output_sample": ws / (B * 256 * T), "batch": B, "frames": T}), flush=True)
  for r in range(a.rounds):
    for mode in a.modes:
      out = run_mode(model, mel, zi, ze, wav, mode, a.sigma, a.steps, a.warmup)
      out.update(round=r, batch=B, frames=T)
      print(json.dumps(out), flush=True)
    for mode in ([m for m in a.weights_modes.split(",") if m in ("w", "wr", "ws", "fs")] if a.weights else ()):
      out = run_weights(model, mel, zi, ze, mode, a.sigma, a.steps, a.warmup)
      out.update(round=r, batch=B, frames=T)
      print(json.dumps(out), flush=True)
  if a.headroom:
    print(json.dumps(headroom(model, mel, zi, ze, a.sigma)), flush=True)


if __name__ == "__main__":
  main()
