"""Timing of the soft-DTW loss (waveglow_amd/softdtw.py: wg_softdtw_forward / wg_softdtw_backward), leg by leg, at two
shapes: 16 pairs of 864 / 865 frames and a ragged batch of 16 pairs with 200 .. 864 frames, K = 16 feature rows, L2 cost.

  values    ``soft_dtw`` without a graph: the forward wavefront alone, no R kept
  saved     ``soft_dtw`` with a graph: the same wavefront storing R
  backward  ``.backward()`` of that forward: memset of E, the backward wavefront, one launch per feature gradient
  torch     the same loss written with torch fp64 operations on the device, one anti-diagonal per step (shifted views of the
            last two diagonals, ``logsumexp``), forward + backward under autograd
  dtw       for scale: ``metrics.dtw_distance`` (wg_metrics_dtw), the exact warping of the same pairs
  infer     for scale: ``infer_differentiable(..., weight_grads=True)`` forward + backward at 32 x 63 frames, 256 channels

With ``--band W`` and / or ``--divergence`` further legs run beside these, with the same alternation and repetitions:

  b-values, b-saved, b-backward   the three soft-DTW legs inside a Sakoe-Chiba band of half-width W (wg_softdtw_banded_*)
  div, b-div                      ``soft_dtw_divergence`` forward + backward, dense and (with ``--band``) banded

and the report gives the bytes every form keeps between forward and backward.

The legs alternate in one process, repetition by repetition, after warm-ups of all of them; each line gives the median and
the 10th and 90th percentile in ms (host clock around the call and a device synchronise).

  python tools/bench_softdtw.py [--reps 10] [--warmup 3] [--gamma 1.0] [--band W] [--divergence] [--skip-scale]
                                [--out profiles/softdtw_ab.txt]
"""
import argparse
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
sys.path.insert(0, ROOT)
from waveglow_amd import metrics, softdtw, synthetic  # noqa: E402
from waveglow_amd.hparams import HParams  # noqa: E402
from waveglow_amd.model import WaveGlow  # noqa: E402

BIG = 1e30      # stands for +infinity in the torch leg: exp(-BIG / gamma) is an exact 0 and no inf - inf can form


def timed(fn, dev):
  torch.cuda.synchronize(dev)
  t0 = time.perf_counter()
  out = fn()
  torch.cuda.synchronize(dev)
  return (time.perf_counter() - t0) * 1e3, out


def line(name, ms):
  a = np.asarray(ms)
  return f"  {name:10s} {np.median(a):9.3f} [{np.percentile(a, 10):.3f} - {np.percentile(a, 90):.3f}]  n = {a.size}"


def torch_soft_dtw(fa, na, fb, nb, gamma):
  """fp64 [B]: the values of ``soft_dtw(fa, na, fb, nb, gamma, "l2")`` with a graph to fa and fb, one anti-diagonal per step."""
  B, _, Ta = fa.shape
  Tb = fb.shape[2]
  dev = fa.device
  D = torch.cdist(fa.double().transpose(1, 2), fb.double().transpose(1, 2))                  # [B, Ta, Tb]
  nd = Ta + Tb - 1
  i = torch.arange(Ta, device=dev)[None, :]
  j = torch.arange(nd, device=dev)[:, None] - i                                                # [nd, Ta]
  inside = ((j >= 0) & (j < Tb))[None] & (i[None] < na[:, None, None]) & (j[None] < nb[:, None, None])
  skew = D[:, i.expand(nd, Ta), j.clamp(0, Tb - 1)]                                             # [B, nd, Ta]: D(i, d - i)
  big = torch.full((B, Ta), BIG, dtype=torch.float64, device=dev)
  col = big[:, :1]
  last = (na + nb - 2).to(torch.int64)
  row = (na - 1).to(torch.int64)[:, None]
  prev1 = prev2 = big
  value = torch.zeros(B, dtype=torch.float64, device=dev)
  for d in range(nd):
    if d == 0:
      r = torch.where(inside[:, 0], skew[:, 0], big)
    else:
      x = torch.stack([torch.cat([col, prev1[:, :-1]], 1), prev1, torch.cat([col, prev2[:, :-1]], 1)])
      r = torch.where(inside[:, d], skew[:, d] - gamma * torch.logsumexp(-x / gamma, dim=0), big)
    value = torch.where(last == d, r.gather(1, row)[:, 0], value)
    prev2, prev1 = prev1, r
  return value


def features(B, K, T, seed, dev):
  """fp32 [B, K, T]: a random walk per feature row, so that neighbouring frames are close as speech features are."""
  gen = torch.Generator().manual_seed(seed)
  return (torch.cumsum(torch.randn((B, K, T), generator=gen) * 0.4, dim=2) + torch.randn((B, K, 1), generator=gen)).to(dev)


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument("--reps", type=int, default=10)
  ap.add_argument("--warmup", type=int, default=3)
  ap.add_argument("--gamma", type=float, default=1.0)
  ap.add_argument("--batch", type=int, default=16)
  ap.add_argument("--frames", type=int, default=864)
  ap.add_argument("--min-frames", type=int, default=200)
  ap.add_argument("--features", type=int, default=16)
  ap.add_argument("--infer-batch", type=int, default=32)
  ap.add_argument("--infer-frames", type=int, default=63)
  ap.add_argument("--band", type=int, default=0, help="also time the banded legs at this half-width")
  ap.add_argument("--divergence", action="store_true", help="also time soft_dtw_divergence forward + backward")
  ap.add_argument("--skip-scale", action="store_true", help="leave out the torch, dtw and infer legs")
  ap.add_argument("--out", default=None, help="also write the report to this file")
  a = ap.parse_args()
  dev = torch.device("cuda:0")
  B, T, K, gamma = a.batch, a.frames, a.features, a.gamma

  hp = HParams()
  model = WaveGlow(hp)
  model.load_state_dict(synthetic.to_weightnorm_form(synthetic.make_state_dict(hp, seed=0)))
  model = model.to(dev).train().requires_grad_(True)
  mel = synthetic.make_mel(a.infer_batch, a.infer_frames, seed=7).to(dev)

  def leg_infer():
    model.zero_grad(set_to_none=True)
    audio = model.infer_differentiable(mel, 0.6, weight_grads=True)
    audio.backward(torch.full_like(audio, 1.0 / audio.numel()))

  report = [f"soft_dtw, K = {K}, gamma = {gamma:g}, cost l2; median [p10 - p90] ms, {a.reps} repetitions after {a.warmup} warm-ups, "
            f"the legs alternating in one process"]
  ragged = [a.min_frames + (T - a.min_frames) * u // max(1, B - 1) for u in range(B)]
  for name, counts_a, counts_b in ((f"{B} pairs of {T} / {T + 1} frames", [T] * B, [T + 1] * B),
                                   (f"{B} pairs of {a.min_frames} .. {T} frames", ragged, ragged[::-1])):
    fa = features(B, K, T, 1, dev).requires_grad_(True)
    fb = features(B, K, T + 1, 2, dev)
    na = torch.tensor(counts_a, dtype=torch.int32, device=dev)
    nb = torch.tensor(counts_b, dtype=torch.int32, device=dev)
    state = {}
    fb_leaf = fa.detach().requires_grad_(True)        # the banded legs' own leaf: fa.grad stays the dense gradient

    def leg_values():
      with torch.no_grad():
        state["values"] = softdtw.soft_dtw(fa, na, fb, nb, gamma)

    def leg_saved():
      state["graph"] = softdtw.soft_dtw(fa, na, fb, nb, gamma)

    def leg_backward():
      fa.grad = None
      state["graph"].sum().backward()

    def leg_torch():
      x = fa.detach().clone().requires_grad_(True)
      v = torch_soft_dtw(x, na, fb, nb, gamma)
      v.sum().backward()
      state["torch_values"], state["torch_grad"] = v.detach(), x.grad

    def leg_dtw():
      state["dtw"] = metrics.dtw_distance(fa.detach(), na, fb, nb)[0]

    def leg_band_values():
      with torch.no_grad():
        state["band_values"] = softdtw.soft_dtw(fa, na, fb, nb, gamma, band=a.band)

    def leg_band_saved():
      state["band_graph"] = softdtw.soft_dtw(fb_leaf, na, fb, nb, gamma, band=a.band)

    def leg_band_backward():
      fb_leaf.grad = None
      state["band_graph"].sum().backward()

    def leg_div(band):
      def run():
        x = fa.detach().requires_grad_(True)
        v = softdtw.soft_dtw_divergence(x, na, fb, nb, gamma, band=band)
        v.sum().backward()
        state["div", band] = v.detach()
      return run

    legs = {"values": leg_values, "saved": leg_saved, "backward": leg_backward}
    if not a.skip_scale:
      legs.update({"torch": leg_torch, "dtw": leg_dtw, "infer": leg_infer})
    if a.band:
      legs.update({"b-values": leg_band_values, "b-saved": leg_band_saved, "b-backward": leg_band_backward})
    if a.divergence:
      legs["div"] = leg_div(None)
      if a.band:
        legs["b-div"] = leg_div(a.band)
    times = {k: [] for k in legs}
    for it in range(a.warmup + a.reps):
      ms = {k: timed(fn, dev)[0] for k, fn in legs.items()}
      if it >= a.warmup:
        for k, v in ms.items():
          times[k].append(v)
    med = {k: float(np.median(t)) for k, t in times.items()}
    report.append(f"{name} (cells {sum(x * y for x, y in zip(counts_a, counts_b))}, R buffer "
                  f"{softdtw.r_bytes(B, T, T + 1) / 2 ** 20:.0f} MiB)")
    report += [line(k, t) for k, t in times.items()]
    plain = med["saved"] + med["backward"]
    if a.band:
      banded = med["b-saved"] + med["b-backward"]
      report.append(f"  band {a.band}: R buffer {softdtw.r_bytes(B, T, T + 1, a.band) / 2 ** 20:.1f} MiB; forward + backward "
                    f"{banded:.3f} ms against {plain:.3f} ms dense; banded - dense values in "
                    f"[{float((state['band_values'] - state['values']).min()):.3f}, "
                    f"{float((state['band_values'] - state['values']).max()):.3f}]")
    if a.divergence:
      for k, band in (("div", None), ("b-div", a.band or None)):
        if k in med:
          ref = med["b-saved"] + med["b-backward"] if band else plain
          report.append(f"  divergence{f' band {band}' if band else ''}: R buffer "
                        f"{softdtw.r_bytes(3 * B, T + 1, T + 1, band) / 2 ** 20:.1f} MiB; forward + backward {med[k]:.3f} ms = "
                        f"{med[k] / ref:.2f}x the plain loss; D in [{float(state['div', band].min()):.3f}, "
                        f"{float(state['div', band].max()):.3f}]")
    if a.skip_scale:
      continue
    v, tv = state["values"], state["torch_values"]
    g, tg = fa.grad.double(), state["torch_grad"].double()
    report.append(f"  forward + backward {med['saved'] + med['backward']:.3f} ms = {med['torch'] / (med['saved'] + med['backward']):.1f}x "
                  f"faster than the torch leg, {100 * (med['saved'] + med['backward']) / med['infer']:.1f} % of the infer leg; "
                  f"values against torch: max relative difference {float(((v - tv).abs() / tv.abs()).max()):.2e}, gradient "
                  f"{float((g - tg).abs().max() / tg.abs().max()):.2e} of max|g|; soft - dtw in "
                  f"[{float((v - state['dtw']).min()):.3f}, {float((v - state['dtw']).max()):.3f}]")
  text = "\n".join(report)
  print(text)
  if a.out:
    with open(a.out, "w") as f:
      f.write(text + "\n")


if __name__ == "__main__":
  main()
