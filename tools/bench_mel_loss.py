"""Timing of ``MultiScaleMelLoss`` (HIP forward and backward) with the default (DAC) scales.  Shapes B x N: 16 x 221 184
(the audio of configs[1]) and 32 x 16 128 by default.  All legs of a shape alternate, repetition by repetition, in one
process; times are hipEvent milliseconds, reported as median [p10 - p90] over the repetitions after the warm-ups.

  values    forward without a graph
  saved     forward with saved state
  backward  the backward of that forward
  torch     the same loss written with torch.stft and a matmul on the device, forward + backward under autograd
  infer     WaveGlow.infer_differentiable forward + backward (d mel) at --vocoder-batch x --vocoder-frames, the step the
            loss is attached to

  python tools/bench_mel_loss.py [--shapes 16x221184,32x16128] [--reps 10] [--warmup 3] [--no-vocoder] [--no-torch]
      [--out FILE]

Every shape also prints the tap products per sample and signal that the transforms execute, the saved bytes, and how far
the torch leg's value and gradient lie from the library's.
"""
import argparse
import os
import statistics
import sys

import torch

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
sys.path.insert(0, ROOT)
from waveglow_amd.mel_loss import MultiScaleMelLoss  # noqa: E402

DEV = "cuda:0"


def torch_mel_loss(x, y, scales, banks, windows, clamp):
  log = 0.0
  for (n_fft, hop, win, _), W, w in zip(scales, banks, windows):
    def mel(t):
      X = torch.stft(t, n_fft, hop, win, w, center=True, pad_mode="reflect", return_complex=True)
      return torch.matmul(W, X.abs())
    log = log + (torch.clamp(mel(x), min=clamp).log() - torch.clamp(mel(y), min=clamp).log()).abs().mean()
  return log / len(scales)


class Timer:
  def __init__(self):
    self.t = {}

  def run(self, key, fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    out = fn()
    b.record()
    torch.cuda.synchronize()
    self.t.setdefault(key, []).append(a.elapsed_time(b))
    return out

  def line(self, key, warmup):
    s = sorted(self.t[key][warmup:])
    pct = lambda q: s[min(len(s) - 1, max(0, round(q * (len(s) - 1))))]
    return f"  {key:<9} {statistics.median(s):9.3f} [{pct(0.1):.3f} - {pct(0.9):.3f}]  n = {len(s)}"

  def median(self, key, warmup):
    return statistics.median(self.t[key][warmup:])


def vocoder_step(a):
  from waveglow_amd import synthetic
  from waveglow_amd.hparams import HParams
  from waveglow_amd.model import WaveGlow
  hp = HParams()
  model = WaveGlow(hp)
  model.load_state_dict(synthetic.to_weightnorm_form(synthetic.make_state_dict(hp, seed=0)))
  model = model.to(DEV).eval().requires_grad_(False)
  B, T = a.vocoder_batch, a.vocoder_frames
  mel = synthetic.make_mel(B, T, seed=7).to(DEV)
  gen = torch.Generator(device=DEV).manual_seed(5)
  zi = torch.randn(B, model.n_remaining_channels, 32 * T, device=DEV, generator=gen)
  n_early = sum(1 for k in range(hp.n_flows) if k % hp.n_early_every == 0 and k > 0)
  ze = [torch.randn(B, hp.n_early_size, 32 * T, device=DEV, generator=gen) for _ in range(n_early)]

  def step():
    m = mel.detach().requires_grad_(True)
    audio = model.infer_differentiable(m, 0.6, z_init=zi, z_early=ze)
    audio.backward(torch.full_like(audio, 1.0 / audio.numel()))
  return step


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument("--shapes", default="16x221184,32x16128")
  ap.add_argument("--reps", type=int, default=10)
  ap.add_argument("--warmup", type=int, default=3)
  ap.add_argument("--no-vocoder", action="store_true")
  ap.add_argument("--no-torch", action="store_true")
  ap.add_argument("--vocoder-batch", type=int, default=32)
  ap.add_argument("--vocoder-frames", type=int, default=63)
  ap.add_argument("--out", help="also append the report to this file")
  a = ap.parse_args()
  lines = []

  def say(s):
    print(s, flush=True)
    lines.append(s)

  crit = MultiScaleMelLoss(device=DEV)
  scales = crit.scales
  banks = [torch.from_numpy(w).to(DEV) for w in crit.mel_bases]
  windows = [torch.hann_window(s[2], device=DEV) for s in scales]
  taps = sum(s[0] * s[2] / s[1] for s in scales)
  say(f"MultiScaleMelLoss, default scales {scales}; median [p10 - p90] ms, {a.reps} repetitions after {a.warmup} "
      f"warm-ups, the legs alternating in one process; {taps:.0f} tap products per sample and signal in the transforms")
  voc = None if a.no_vocoder else vocoder_step(a)
  for shape in a.shapes.split(","):
    B, N = (int(v) for v in shape.split("x"))
    gen = torch.Generator(device=DEV).manual_seed(1)
    x = torch.rand(B, N, device=DEV, generator=gen) * 1.6 - 0.8
    y = torch.rand(B, N, device=DEV, generator=gen) * 1.6 - 0.8
    tm = Timer()
    g_lib = g_torch = v_lib = v_torch = None
    for _ in range(a.warmup + a.reps):
      with torch.no_grad():
        tm.run("values", lambda: crit(x, y))
      xg = x.detach().requires_grad_(True)
      loss = tm.run("saved", lambda: crit(xg, y))
      tm.run("backward", loss.backward)
      g_lib, v_lib = xg.grad, loss.detach()
      del loss, xg
      if not a.no_torch:
        xg = x.detach().requires_grad_(True)

        def both():
          out = torch_mel_loss(xg, y, scales, banks, windows, crit.clamp)
          out.backward()
          return out.detach()
        v_torch = tm.run("torch", both)
        g_torch = xg.grad
        del xg
      if voc is not None:
        tm.run("infer", voc)
    say(f"{B} x {N} (saved state {crit.workspace_bytes(B, N) / 2 ** 20:.1f} MiB)")
    for key in ("values", "saved", "backward", "torch", "infer"):
      if key in tm.t:
        say(tm.line(key, a.warmup))
    both = tm.median("saved", a.warmup) + tm.median("backward", a.warmup)
    tail = f"  forward + backward {both:.3f} ms"
    if "torch" in tm.t:
      tail += (f"; the torch leg takes {tm.median('torch', a.warmup) / both:.2f} times that; value against torch: relative "
               f"difference {abs(float(v_lib) - float(v_torch)) / abs(float(v_torch)):.2e}, gradient "
               f"{float((g_lib - g_torch).abs().max() / g_torch.abs().max()):.2e} of max|g|")
    if "infer" in tm.t:
      tail += f"; {100 * both / tm.median('infer', a.warmup):.1f} % of the infer leg"
    say(tail)
  if a.out:
    with open(a.out, "a") as f:
      f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
  main()
