"""Golden TRAJECTORIES from the reference's own training loop (build container only; imports the reference).

  python tests/golden/make_golden_trajectory.py [c64] [c256]

K = 10 optimiser steps of the reference's loop (train.py:190-199: zero_grad -> forward -> WaveGlowLoss -> backward ->
optimizer.step) on CPU fp32, on the reference's own WaveGlow with the synthetic weights, two alternating batches.  Legs:
c64 with Adam (lr 1e-4, the HParams default), c64 with plain SGD (lr 1e-2; Adam is blind to the scale of a gradient,
SGD's update is the sum of the gradients), c256 (default HParams) with Adam.

Per leg (keys ``LEG/...``; the per-parameter records are PACKED in the order of ``LEG/names``, because one zip member
per parameter and record would put 686 x 4 members into the c256 file and that alone exceeds the size of the largest
committed fixture -- tests/_cases.py: Trajectory gives them back by name):

  loss[K+1]      the loss read before each step + the loss of batch 0 after the last one
  dglobal        ||theta_K - theta_0|| over all parameters
  dnorm, dsum    [P]   norm and sum of every parameter's update
  dhead          [P,8] its first 8 values (zero-padded for smaller tensors)
  dsub           kept values of every update, concatenated: the WHOLE update of a tensor of at most sub_full elements
                 (c64: 4096, c256: 64), of a larger one an evenly strided sample (one value per 2048 elements, at
                 least sub_min, at most 4096 -- tests/_cases.py: sub_count, sub_index).  The whole updates of the large
                 tensors (6.5 M elements in ``upsample``) cannot be committed; the sample lets a test measure
                 ||D - D_ref|| there too, and over all parameters, each kept value standing for numel / kept elements.

Yardsticks -- what a path may do whose every gradient sits at the edge of the single-step bound the project already
states (GRAD_TOL = 5e-3): the same loop with every p.grad replaced by g + n * (GRAD_TOL * ||g|| / ||n||), n Gaussian,
fresh per step and tensor (seeds 1, 2, 3; c256: seed 1) and once with ONE n per tensor for all steps:

  yard_loss[K+1]                          max over those runs of |loss - loss_ref|
  yard_global_random, yard_global_fixed   ||D - D_ref|| / ||D_ref|| over all parameters (max over the random seeds),
                                          measured over the kept values exactly as the tests measure (_cases.sub_errors);
                                          the figure over whole tensors is printed beside it
  yard           [P]   max over the runs of every tensor's ||D - D_ref|| / ||D_ref||, the larger of whole tensor and
                       kept values

Fault records (c64): the loop with the update of step 5 skipped, and with step 5 run on step 4's weights (a stale packed
copy: forward and backward both see them, the update goes to the current parameters): fault_skip_loss / _global,
fault_stale_loss / _global = max |loss - loss_ref| and the global update error (over the kept values).  tests/test_trajectory_cpu.py holds the
GPU tests' bounds to at most half of these.
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.abspath(os.path.join(HERE, "..")))
sys.path.insert(0, os.path.abspath(os.path.join(HERE, "..", "..")))
from _ref_import import import_reference  # noqa: E402
from _cases import GRAD_TOL, sub_errors, sub_take, trajectory_batches  # noqa: E402
from waveglow_amd.hparams import HParams  # noqa: E402
from waveglow_amd import synthetic  # noqa: E402

ref_model, ref_hparams, ref_train = import_reference()

K = 10                # GRAD_TOL (5e-3) is the single-step bound per gradient tensor
FAULT_STEP = 5
FIXED_SEED = 4

# name: (hparam overrides, B, mel frames T, weight seed, crop (S = 256*T - crop), legs, random yardstick seeds, faults,
#        (sub_full, sub_min): tensors kept whole up to sub_full elements, at least sub_min values of the others)
CASES = {"c64": (dict(n_channels=64, n_layers=4, n_flows=6, n_early_every=2), 2, 12, 5, 96,
                 (("adam", 1e-4), ("sgd", 1e-2)), (1, 2, 3), True, (4096, 256)),
         "c256": (dict(), 2, 9, 3, 40, (("adam", 1e-4),), (1,), False, (64, 64))}
if len(sys.argv) > 1:
  CASES = {k: v for k, v in CASES.items() if k in sys.argv[1:]}


def run(over, sd, data, kind, lr, perturb=None, fault=None):
  """perturb: None | ("random", seed) | ("fixed", seed);  fault: None | "skip" | "stale".
  Returns (loss[K+1] float64, {name: theta_K - theta_0})."""
  model = ref_model.WaveGlow(ref_hparams.HParams(**over))
  model.load_state_dict(sd)
  model.train()
  crit = ref_train.WaveGlowLoss(sigma=1.0)
  params = dict(model.named_parameters())
  theta0 = {n: p.detach().clone() for n, p in params.items()}
  opt = (torch.optim.Adam(model.parameters(), lr=lr) if kind == "adam" else torch.optim.SGD(model.parameters(), lr=lr))
  gen = torch.Generator().manual_seed(perturb[1]) if perturb else None
  fixed = ({n: torch.randn(p.shape, generator=gen) for n, p in params.items()}
           if perturb and perturb[0] == "fixed" else None)
  losses = []
  before_prev = None
  for k in range(K):
    before = [p.detach().clone() for p in params.values()]
    stale = fault == "stale" and k == FAULT_STEP
    if stale:
      with torch.no_grad():
        for p, old in zip(params.values(), before_prev):
          p.copy_(old)
    model.zero_grad()
    loss = crit(model(data[k % 2]), None)
    losses.append(float(loss.detach()))
    loss.backward()
    if stale:
      with torch.no_grad():
        for p, cur in zip(params.values(), before):
          p.copy_(cur)
    if perturb:
      for n, p in params.items():
        noise = fixed[n] if fixed is not None else torch.randn(p.shape, generator=gen)
        p.grad = p.grad + noise * (GRAD_TOL * float(p.grad.norm()) / float(noise.norm()))
    if not (fault == "skip" and k == FAULT_STEP):
      opt.step()
    before_prev = before
  with torch.no_grad():
    losses.append(float(crit(model(data[0]), None)))
  return np.array(losses, dtype=np.float64), {n: (p.detach() - theta0[n]) for n, p in params.items()}


def true_errors(d, d_ref):
  """Over whole tensors: ([relative update error per tensor], global relative update error)."""
  e2 = np.array([float((d[n].double() - d_ref[n].double()).pow(2).sum()) for n in d_ref])
  r2 = np.array([float(d_ref[n].double().pow(2).sum()) for n in d_ref])
  return np.sqrt(e2 / np.maximum(r2, 1e-60)), float(np.sqrt(e2.sum() / r2.sum()))


def measure(d, d_ref, ref_sub, full, nmin):
  """([per-tensor relative update error: the larger of the whole-tensor figure and the one over the kept values],
  global error over the kept values -- what the tests can compute --, global error over whole tensors)."""
  t_true, g_true = true_errors(d, d_ref)
  per, g_sub = sub_errors(d, ref_sub, full, nmin)
  t_sub = np.array([per[n][0] / max(per[n][1], 1e-30) for n in d_ref])
  return np.maximum(t_true, t_sub), g_sub, g_true


for name, (over, B, T, wseed, crop, legs, seeds, faults, (full, nmin)) in CASES.items():
  hp = HParams(**over)
  sd = synthetic.to_weightnorm_form(synthetic.make_state_dict(hp, seed=wseed))
  data = trajectory_batches(B, T, crop)
  out = {"hp_json": np.array(str(over)), "K": np.array(K), "weight_seed": np.array(wseed), "B": np.array(B),
         "T": np.array(T), "crop": np.array(crop), "grad_tol": np.array(GRAD_TOL), "fault_step": np.array(FAULT_STEP),
         "sub_full": np.array(full), "sub_min": np.array(nmin), "legs": np.array([leg for leg, _ in legs])}
  for leg, lr in legs:
    loss, d_ref = run(over, sd, data, leg, lr)
    print(f"{name}/{leg}: loss", " ".join(f"{v:.5f}" for v in loss), flush=True)
    if name == "c64":
      fx = np.load(os.path.join(HERE, "c64_grads.npz"))
      assert np.float32(loss[0]) == fx["loss"], (loss[0], float(fx["loss"]))
    names = list(d_ref)
    ref_sub = {n: sub_take(d_ref[n], full, nmin).clone() for n in names}
    dglobal = sum(float(d.double().pow(2).sum()) for d in d_ref.values()) ** 0.5
    head = np.zeros((len(names), 8), dtype=np.float32)
    for i, n in enumerate(names):
      h = d_ref[n].flatten()[:8].numpy()
      head[i, :h.size] = h
    rec = {"lr": np.array(lr), "loss": loss.astype(np.float32), "names": np.array(names),
           "numel": np.array([d_ref[n].numel() for n in names], dtype=np.int64),
           "dglobal": np.array(dglobal, dtype=np.float32),
           "dnorm": np.array([float(d_ref[n].double().norm()) for n in names], dtype=np.float32),
           "dsum": np.array([float(d_ref[n].double().sum()) for n in names], dtype=np.float32), "dhead": head,
           "dsub": np.concatenate([ref_sub[n].numpy() for n in names]).astype(np.float32)}
    yard_loss = np.zeros(K + 1)
    yard = np.zeros(len(names))
    g_random = 0.0
    for what, seed in [("random", s) for s in seeds] + [("fixed", FIXED_SEED)]:
      l, d = run(over, sd, data, leg, lr, perturb=(what, seed))
      t, g_sub, g_true = measure(d, d_ref, ref_sub, full, nmin)
      print(f"{name}/{leg}: {what} seed {seed}: max |dloss| {np.abs(l - loss).max():.3e}  global {g_sub:.4e} "
            f"(whole tensors {g_true:.4e})  worst tensor {t.max():.3e} ({names[int(t.argmax())]})", flush=True)
      yard_loss = np.maximum(yard_loss, np.abs(l - loss))
      yard = np.maximum(yard, t)
      if what == "random":
        g_random = max(g_random, g_sub)
      else:
        g_fixed = g_sub
    rec.update(yard_loss=yard_loss.astype(np.float32), yard=yard.astype(np.float32),
               yard_global_random=np.array(g_random, dtype=np.float32),
               yard_global_fixed=np.array(g_fixed, dtype=np.float32), yard_seeds=np.array(list(seeds) + [FIXED_SEED]))
    print(f"{name}/{leg}: yard_loss", " ".join(f"{v:.2e}" for v in yard_loss), flush=True)
    if faults:
      for fault in ("skip", "stale"):
        l, d = run(over, sd, data, leg, lr, fault=fault)
        _, g_sub, g_true = measure(d, d_ref, ref_sub, full, nmin)
        rec[f"fault_{fault}_loss"] = np.array(np.abs(l - loss).max(), dtype=np.float32)
        rec[f"fault_{fault}_global"] = np.array(g_sub, dtype=np.float32)
        print(f"{name}/{leg}: fault {fault}: max |dloss| {float(rec[f'fault_{fault}_loss']):.3e}  "
              f"global {g_sub:.4e} (whole tensors {g_true:.4e})", flush=True)
    out.update({f"{leg}/{k}": v for k, v in rec.items()})
  path = os.path.join(HERE, f"{name}_trajectory.npz")
  np.savez_compressed(path, **out)
  print(name, "written", os.path.getsize(path), "bytes")
