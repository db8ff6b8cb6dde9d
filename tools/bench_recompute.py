"""Activation recomputation (``WaveGlow.recompute_activations``, include/waveglow_amd.h: WG_TRAIN_RECOMPUTE) against the
default full-save mode, at BASELINE configs[3] shapes (per GPU: 256 channels, batch 32 x 63 mel frames, 16 000-sample
segments), synthetic data and weights.  One JSON line per (path, mode), modes measured in interleaved rounds on one box:

  t  training step: WaveGlow.forward + WaveGlowLoss + backward (every parameter gradient)
  l  frozen likelihood loss: the same with frozen weights, d mel + d audio
  i  infer_differentiable forward + backward with d mel and d z (z_init and every z_early)

Each line: forward and backward ms (means over --steps after --warmup, per round), the library's workspace GB of the
mode and torch.cuda.max_memory_allocated over the measured steps.  ``--full-utterance`` adds one line that full-save mode
cannot reasonably hold: infer_differentiable with recompute at batch 16 x 861 frames (16 utterances of 10 s, 3.5 M
samples; the full-save workspace would be about 135 GB there), with its peak memory and time.  Full-save mode is not run
at that size.

  python tools/bench_recompute.py [--batch 32] [--frames 63] [--samples 16000] [--steps 5] [--warmup 2] [--rounds 3]
                                  [--paths tli] [--modes fr] [--full-utterance]

--modes: f full save, r recompute (``--modes r --paths t --rounds 1``: the recompute training step alone, for a kernel trace).
"""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.abspath(os.path.join(os.path.dirname(__file__), "..")))
from waveglow_amd import synthetic  # noqa: E402
from waveglow_amd.hparams import HParams  # noqa: E402
from waveglow_amd.model import WaveGlow, WaveGlowLoss  # noqa: E402


def make_model(hp, sd, path, recompute):
  model = WaveGlow(hp)
  model.load_state_dict(sd)
  model = model.to("cuda:0")
  if path == "t":
    model.train()
  else:
    model.eval().requires_grad_(False)
  model.recompute_activations = recompute
  return model


def noise(model, B, T, gen):
  L = 256 * T // model.n_group
  zi = torch.randn(B, model.n_remaining_channels, L, generator=gen).cuda()
  n_early = sum(1 for k in range(model.n_flows) if k % model.n_early_every == 0 and k > 0)
  ze = [torch.randn(B, model.n_early_size, L, generator=gen).cuda() for _ in range(n_early)]
  return zi, ze


def one_step(model, path, mel, wav, zi, ze):
  """(forward ms, backward ms) of one step."""
  ev = [torch.cuda.Event(enable_timing=True) for _ in range(3)]
  torch.cuda.synchronize()
  ev[0].record()
  if path == "i":
    m = mel.detach().requires_grad_(True)
    z_i = zi.detach().requires_grad_(True)
    z_e = [z.detach().requires_grad_(True) for z in ze]
    out = model.infer_differentiable(m, 1.0, z_init=z_i, z_early=z_e)
    ev[1].record()
    out.backward(torch.full_like(out, 1.0 / out.numel()))
  else:
    if path == "t":
      model.zero_grad(set_to_none=True)
      m, a = mel, wav
    else:
      m, a = mel.detach().requires_grad_(True), wav.detach().requires_grad_(True)
    out = WaveGlowLoss(1.0)(model((m, a)), None)
    ev[1].record()
    out.backward()
  ev[2].record()
  torch.cuda.synchronize()
  del out
  return ev[0].elapsed_time(ev[1]), ev[1].elapsed_time(ev[2])


def measure(model, path, mel, wav, zi, ze, steps, warmup):
  for _ in range(warmup):
    one_step(model, path, mel, wav, zi, ze)
  torch.cuda.synchronize()
  torch.cuda.reset_peak_memory_stats()
  tf = tb = 0.0
  for _ in range(steps):
    f, b = one_step(model, path, mel, wav, zi, ze)
    tf += f
    tb += b
  return tf / steps, tb / steps, torch.cuda.max_memory_allocated()


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument("--batch", type=int, default=32)
  ap.add_argument("--frames", type=int, default=63)
  ap.add_argument("--samples", type=int, default=16000)
  ap.add_argument("--steps", type=int, default=5)
  ap.add_argument("--warmup", type=int, default=2)
  ap.add_argument("--rounds", type=int, default=3)
  ap.add_argument("--paths", default="tli")
  ap.add_argument("--modes", default="fr")
  ap.add_argument("--full-utterance", action="store_true")
  args = ap.parse_args()
  hp = HParams()
  sd = synthetic.to_weightnorm_form(synthetic.make_state_dict(hp, seed=7))
  B, T = args.batch, args.frames
  mel = synthetic.make_mel(B, T, seed=1).cuda()
  g = torch.Generator().manual_seed(3)
  wav = (torch.rand(B, args.samples, generator=g) * 0.6 - 0.3).cuda()
  for path in args.paths:
    zi, ze = noise(WaveGlow(hp), B, T, torch.Generator().manual_seed(5))
    modes = [m == "r" for m in args.modes]
    res = {m: [] for m in modes}
    for rnd in range(args.rounds):
      for recompute in modes:               # interleaved: one model per mode and round, nothing else alive
        model = make_model(hp, sd, path, recompute)
        S = 256 * T if path == "i" else args.samples
        ws = model.gradient_workspace_bytes(B, T, S)
        res[recompute].append(measure(model, path, mel, wav, zi, ze, args.steps, args.warmup) + (ws,))
        del model
        torch.cuda.empty_cache()
    for recompute in modes:
      r = res[recompute]
      print(json.dumps({
          "path": {"t": "train_step", "l": "frozen_dmel_daudio", "i": "infer_differentiable_dmel_dz"}[path],
          "recompute": recompute, "batch": B, "frames": T,
          "forward_ms": [round(x[0], 3) for x in r], "backward_ms": [round(x[1], 3) for x in r],
          "total_ms_min": round(min(x[0] + x[1] for x in r), 3),
          "workspace_gb": round(r[0][3] / 1e9, 3), "max_allocated_gb": round(max(x[2] for x in r) / 1e9, 3)}), flush=True)
  if args.full_utterance:
    Bu, Tu = 16, 861
    model = make_model(hp, sd, "i", True)
    full_ws = model.gradient_workspace_bytes(Bu, Tu, recompute=False)
    ws = model.gradient_workspace_bytes(Bu, Tu)
    melu = synthetic.make_mel(Bu, Tu, seed=2).cuda()
    zi, ze = noise(model, Bu, Tu, torch.Generator().manual_seed(6))
    f, b, peak = measure(model, "i", melu, None, zi, ze, max(1, args.steps // 2), 1)
    print(json.dumps({"path": "infer_differentiable_dmel_dz_full_utterance", "recompute": True, "batch": Bu, "frames": Tu,
                      "samples": Bu * 256 * Tu, "forward_ms": round(f, 3), "backward_ms": round(b, 3),
                      "workspace_gb": round(ws / 1e9, 3), "full_save_workspace_gb_not_run": round(full_ws / 1e9, 3),
                      "max_allocated_gb": round(peak / 1e9, 3)}), flush=True)


if __name__ == "__main__":
  main()
