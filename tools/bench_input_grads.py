"""Forward + backward timing of ``WaveGlow.forward`` with input gradients, at BASELINE config 4 shapes (per GPU: batch 32 x
16000 samples, 63 mel frames, fp32 I/O), synthetic data / random-init weights.  One JSON line per mode:

  a  today's training step: trainable weights, inputs without gradient
  b  trainable weights plus d mel and d audio
  c  frozen weights (model.requires_grad_(False)), d mel and d audio: the data-gradient chain alone
  d  frozen weights, d audio only (no d spect GEMM, no d mel)

  python tools/bench_input_grads.py [--batch 32] [--steps 5] [--warmup 2] [--modes abcd] [--rounds 1]

--rounds > 1 runs the modes round-robin that many times (same-box A/B: drift shows up as spread between rounds).
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

MODES = {"a": (False, False, False), "b": (False, True, True), "c": (True, True, True), "d": (True, False, True)}


def run_mode(model, mel, wav, mode, steps, warmup):
  frozen, want_mel, want_audio = MODES[mode]
  model.requires_grad_(not frozen)
  crit = WaveGlowLoss(1.0)
  ev = [torch.cuda.Event(enable_timing=True) for _ in range(3)]
  t_f = t_b = 0.0
  for it in range(warmup + steps):
    model.zero_grad(set_to_none=True)
    m = mel.detach().requires_grad_(want_mel)
    a = wav.detach().requires_grad_(want_audio)
    torch.cuda.synchronize()
    ev[0].record()
    loss = crit(model((m, a)), None)
    ev[1].record()
    loss.backward()
    ev[2].record()
    torch.cuda.synchronize()
    if it >= warmup:
      t_f += ev[0].elapsed_time(ev[1])
      t_b += ev[1].elapsed_time(ev[2])
  return {"mode": mode, "frozen": frozen, "d_mel": want_mel, "d_audio": want_audio, "ms_forward": t_f / steps,
          "ms_backward": t_b / steps, "ms_fwd_plus_bwd": (t_f + t_b) / steps, "loss": float(loss.detach())}


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument("--batch", type=int, default=32)
  ap.add_argument("--segment", type=int, default=16000)
  ap.add_argument("--steps", type=int, default=5)
  ap.add_argument("--warmup", type=int, default=2)
  ap.add_argument("--modes", default="abcd")
  ap.add_argument("--rounds", type=int, default=1)
  a = ap.parse_args()
  hp = HParams()
  sd = synthetic.to_weightnorm_form(synthetic.make_state_dict(hp, seed=0))
  model = WaveGlow(hp)
  model.load_state_dict(sd)
  model = model.to("cuda:0").train()
  mel = synthetic.make_mel(a.batch, 1 + a.segment // 256, seed=7).cuda()
  wav = (torch.rand(a.batch, a.segment, generator=torch.Generator().manual_seed(3)) * 0.6 - 0.3).cuda()
  for r in range(a.rounds):
    for mode in a.modes:
      out = run_mode(model, mel, wav, mode, a.steps, a.warmup)
      out.update(round=r, batch=a.batch, segment=a.segment)
      print(json.dumps(out), flush=True)


if __name__ == "__main__":
  main()
