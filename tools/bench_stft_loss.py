"""Timing of ``MultiResolutionSTFTLoss`` (HIP forward and backward).  One JSON line per shape and leg; shapes B x N:
16 x 221 184 (the audio of configs[1]) and 32 x 16 128 by default.  All legs of a shape run interleaved, step by step,
in one process; times are hipEvent milliseconds, mean / median / min / p10 / p90 over the steps after the warm-up.

  all      the default three resolutions: forward without a graph, forward with saved state, backward
  r<i>     the same for a module with resolution i alone
  torch    the same loss written with torch.stft on the GPU (pad + unfold + matmul if torch.stft fails), forward +
           backward under autograd
  vocoder  WaveGlow.infer_differentiable forward + backward (d mel) at --vocoder-batch x --vocoder-frames, the step this
           loss is attached to
  --lengths  beside every library leg, the same module called with ``lengths=``: B utterances spread evenly from
           200/864 of the row pitch to all of it, in whole frames of 256 samples (16 x 221 184: 200 ... 864 frames),
           reported as leg "<name>.lengths" with the sum of the lengths; shapes whose N is no multiple of 256 skip it

  python tools/bench_stft_loss.py [--shapes 16x221184,32x16128] [--steps 20] [--warmup 3] [--legs all,r0,r1,r2]
      [--no-vocoder] [--no-torch] [--lengths]

GEMM work per line: ``gflop_window`` counts the products the kernels execute (only the taps under the window),
``gflop_full`` the full n_fft x (n_fft + 2) basis; the rates are over the measured time.
"""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from test_stft_loss_cpu import DEFAULT_RES, loss_unfold, terms_from_power  # noqa: E402
from waveglow_amd.stft_loss import MultiResolutionSTFTLoss  # noqa: E402

DEV = "cuda:0"


def torch_stft_loss(x, y, windows, eps=1e-7):
  sc = mag = 0.0
  for (n_fft, hop, win), w in zip(DEFAULT_RES, windows):
    def power(t):
      X = torch.stft(t, n_fft, hop, win, w, center=True, pad_mode="reflect", return_complex=True)
      return X.real ** 2 + X.imag ** 2
    s, m = terms_from_power(power(x), power(y), eps)
    sc, mag = sc + s, mag + m
  return (sc + mag) / len(DEFAULT_RES)


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

  def stats(self, key, warmup):
    v = self.t[key][warmup:]
    s = sorted(v)
    pct = lambda q: s[min(len(s) - 1, max(0, round(q * (len(s) - 1))))]
    return {"mean": sum(v) / len(v), "median": statistics.median(v), "min": min(v), "p10": pct(0.1), "p90": pct(0.9)}


def spread_lengths(B, N):
  """B lengths in whole frames of 256 samples, evenly from 200/864 of the pitch to the pitch; None if N % 256."""
  if N % 256 or B < 2:
    return None
  T = N // 256
  lo = round(T * 200 / 864)
  return [256 * round(lo + (T - lo) * b / (B - 1)) for b in range(B)]


def gflops(res, B, N):
  win_f = win_b = full = 0.0
  for n_fft, hop, win in res:
    F = N // hop + 1
    win_f += 2.0 * n_fft * ((win + 63) // 64 * 64) * B * F
    win_b += 2.0 * n_fft * ((win + 31) // 32 * 32) * B * F
    full += 2.0 * n_fft * (n_fft + 2) * B * F
  return win_f / 1e9, win_b / 1e9, full / 1e9


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
  ap.add_argument("--steps", type=int, default=20)
  ap.add_argument("--warmup", type=int, default=3)
  ap.add_argument("--legs", default="all,r0,r1,r2", help="which library modules to time")
  ap.add_argument("--no-vocoder", action="store_true")
  ap.add_argument("--no-torch", action="store_true")
  ap.add_argument("--lengths", action="store_true", help="also time every library leg with per-utterance lengths")
  ap.add_argument("--vocoder-batch", type=int, default=32)
  ap.add_argument("--vocoder-frames", type=int, default=63)
  a = ap.parse_args()
  mods = {"all": MultiResolutionSTFTLoss(device=DEV)}
  for i, r in enumerate(DEFAULT_RES):
    mods[f"r{i}"] = MultiResolutionSTFTLoss((r[0],), (r[1],), (r[2],), device=DEV)
  mods = {k: v for k, v in mods.items() if k in a.legs.split(",")}
  windows = [torch.hann_window(w, device=DEV) for _, _, w in DEFAULT_RES]
  voc = None if a.no_vocoder else vocoder_step(a)
  for shape in a.shapes.split(","):
    B, N = (int(v) for v in shape.split("x"))
    gen = torch.Generator(device=DEV).manual_seed(1)
    x = torch.rand(B, N, device=DEV, generator=gen) * 1.6 - 0.8
    y = torch.rand(B, N, device=DEV, generator=gen) * 1.6 - 0.8
    torch_fn = None
    if not a.no_torch:
      torch_fn = lambda t: torch_stft_loss(t, y, windows)
      try:
        torch_fn(x.detach().requires_grad_(True)).backward()
        torch_name = "torch.stft"
      except Exception as e:   # noqa: BLE001
        print(json.dumps({"torch_stft_failed": repr(e)[:200]}), flush=True)
        torch_fn = lambda t: loss_unfold(t, y, DEFAULT_RES, 1e-7, 1.0, 1.0, dtype=torch.float32)[2]
        torch_name = "pad + unfold + matmul"
    tm = Timer()
    lens = spread_lengths(B, N) if a.lengths else None
    for _ in range(a.warmup + a.steps):
      for key, crit in mods.items():
        with torch.no_grad():
          tm.run(key + ".forward", lambda: crit(x, y))
        xg = x.detach().requires_grad_(True)
        loss = tm.run(key + ".forward_saved", lambda: crit(xg, y))
        tm.run(key + ".backward", loss.backward)
        del loss, xg
        if lens is not None:
          with torch.no_grad():
            tm.run(key + ".lengths.forward", lambda: crit(x, y, lens))
          xg = x.detach().requires_grad_(True)
          loss = tm.run(key + ".lengths.forward_saved", lambda: crit(xg, y, lens))
          tm.run(key + ".lengths.backward", loss.backward)
          del loss, xg
      if torch_fn is not None:
        xg = x.detach().requires_grad_(True)
        loss = tm.run("torch.forward", lambda: torch_fn(xg))
        tm.run("torch.backward", loss.backward)
        del loss, xg
      if voc is not None:
        tm.run("vocoder.fwd_plus_bwd", voc)
    for key, crit in mods.items():
      res = crit.resolutions
      gf, gb, full = gflops(res, B, N)
      f, s, b = (tm.stats(f"{key}.{leg}", a.warmup) for leg in ("forward", "forward_saved", "backward"))
      print(json.dumps({
        "leg": key, "batch": B, "n_samples": N, "resolutions": res, "ms_forward": f, "ms_forward_saved": s,
        "ms_backward": b, "ms_fwd_saved_plus_bwd_median": s["median"] + b["median"],
        "workspace_bytes": crit.workspace_bytes(B, N),
        "gflop_window": {"forward_two_signals": 2 * gf, "backward": gb}, "gflop_full_one_signal": full,
        "tflops_window": {"forward_saved": 2 * gf / s["median"], "backward": gb / b["median"]},
        "tflops_full_basis": {"forward_saved": 2 * full / s["median"], "backward": full / b["median"]}}), flush=True)
      if lens is not None:
        f, s, b = (tm.stats(f"{key}.lengths.{leg}", a.warmup) for leg in ("forward", "forward_saved", "backward"))
        print(json.dumps({
          "leg": key + ".lengths", "batch": B, "n_samples": N, "resolutions": res, "lengths": lens,
          "samples_of_dense": sum(lens) / (B * N), "ms_forward": f, "ms_forward_saved": s, "ms_backward": b,
          "ms_fwd_saved_plus_bwd_median": s["median"] + b["median"]}), flush=True)
    if torch_fn is not None:
      f, b = tm.stats("torch.forward", a.warmup), tm.stats("torch.backward", a.warmup)
      print(json.dumps({"leg": "torch", "what": torch_name, "batch": B, "n_samples": N, "ms_forward": f,
                        "ms_backward": b, "ms_fwd_plus_bwd_median": f["median"] + b["median"]}), flush=True)
    if voc is not None:
      print(json.dumps({"leg": "vocoder", "batch": a.vocoder_batch, "frames": a.vocoder_frames,
                        "ms_fwd_plus_bwd": tm.stats("vocoder.fwd_plus_bwd", a.warmup)}), flush=True)


if __name__ == "__main__":
  main()
