"""Shared helpers: rebuild the inputs of a golden case from its fixture + the weight generator."""
import ast
import os
import zlib

import numpy as np
import torch

from waveglow_amd.hparams import HParams
from waveglow_amd import synthetic

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


class Case:
  def __init__(self, name):
    self.name = name
    self.npz = np.load(os.path.join(GOLDEN, f"{name}.npz"), allow_pickle=False)
    over = dict(ast.literal_eval(str(self.npz["hp_json"])))
    self.hp = HParams(**over)
    self.sigma = float(self.npz["sigma"])
    self.sd = synthetic.make_state_dict(self.hp, seed=int(self.npz["weight_seed"]))
    self.mel = torch.from_numpy(self.npz["mel"])
    self.z_init = torch.from_numpy(self.npz["z_init"])
    self.z_early = {int(k.split("_")[-1]): torch.from_numpy(self.npz[k])
                    for k in self.npz.files if k.startswith("z_early_")}
    self.audio = torch.from_numpy(self.npz["audio"])

  def weights_crc(self):
    crc = 0
    for key in sorted(self.sd):
      crc = zlib.crc32(self.sd[key].numpy().tobytes(), crc)
    return crc

  def oracle_cfg(self):
    from oracle.torch_oracle import OracleConfig
    hp = self.hp
    return OracleConfig(n_mel_channels=hp.n_mel_channels, n_flows=hp.n_flows, n_group=hp.n_group,
                        n_early_every=hp.n_early_every, n_early_size=hp.n_early_size,
                        n_layers=hp.n_layers, n_channels=hp.n_channels, kernel_size=hp.kernel_size)


def oracle_cfg_from_hp(hp):
  from oracle.torch_oracle import OracleConfig
  return OracleConfig(n_mel_channels=hp.n_mel_channels, n_flows=hp.n_flows, n_group=hp.n_group,
                      n_early_every=hp.n_early_every, n_early_size=hp.n_early_size,
                      n_layers=hp.n_layers, n_channels=hp.n_channels, kernel_size=hp.kernel_size)


def rms(x):
  return float(torch.as_tensor(x).double().pow(2).mean().sqrt())


GRAD_TOL = 5e-3     # measured worst case 1.1e-3


def _check(grads, ref, what):
  worst = []
  for name, g_ref in ref.items():
    g = grads[name]
    assert g.shape == g_ref.shape, name
    assert torch.isfinite(g).all(), name
    err = float((g - g_ref).norm())
    den = float(g_ref.norm())
    worst.append((err / max(den, 1e-12), name, err, den))
  worst.sort(reverse=True)
  for rel, name, err, den in worst[:8]:
    print(f"{what}: {name}: rel {rel:.3e} (err {err:.3e}, ref norm {den:.3e})")
  for rel, name, err, den in worst:
    assert err <= GRAD_TOL * den + 1e-7, f"{name}: gradient error {err:.3e} vs norm {den:.3e}"


# ---------------------------------------------------------------- K-step trajectories (golden/make_golden_trajectory.py)
def trajectory_batches(B, T, crop):
  """The two alternating batches of a trajectory case: step k trains on batch k % 2."""
  out = []
  for k in (0, 1):
    mel = synthetic.make_mel(B, T, seed=1234 + B + T + k)
    g = torch.Generator().manual_seed(99 + T + k)
    out.append((mel, torch.rand(B, 256 * T - crop, generator=g) * 0.6 - 0.3))
  return out


def sub_count(numel, full, nmin):
  """How many values of an update the fixture keeps: all of a tensor of at most ``full`` elements, otherwise one per
  2048 elements, at least ``nmin`` and at most 4096."""
  return numel if numel <= full else min(numel, max(nmin, min(4096, numel // 2048)))


def sub_index(numel, n):
  """Evenly strided positions of the kept values in the flattened tensor."""
  return (torch.arange(n, dtype=torch.int64) * numel) // n


def sub_take(t, full, nmin):
  t = t.detach().flatten()
  n = sub_count(t.numel(), full, nmin)
  return t if n == t.numel() else t[sub_index(t.numel(), n)]


def sub_errors(delta, ref_sub, full, nmin):
  """Update errors as far as the kept values can see them.  delta: {name: theta_K - theta_0} (whole tensors),
  ref_sub: {name: kept values of the reference update}.  Returns ({name: (||d - d_ref||, ||d_ref||) over the kept
  values}, global): the global figure is ||D - D_ref|| / ||D_ref|| over ALL parameters, each tensor's kept values
  standing for numel / kept elements (exact where a tensor is kept whole)."""
  per, num, den = {}, 0.0, 0.0
  for name, r in ref_sub.items():
    d = sub_take(delta[name], full, nmin).double()
    r = r.double()
    assert d.shape == r.shape, name
    e2, r2 = float((d - r).pow(2).sum()), float(r.pow(2).sum())
    w = delta[name].numel() / r.numel()
    num += w * e2
    den += w * r2
    per[name] = (e2 ** 0.5, r2 ** 0.5)
  return per, (num / den) ** 0.5


class Trajectory:
  """One leg of tests/golden/NAME_trajectory.npz, its per-parameter records unpacked by name, and the bounds the GPU
  tests hold the HIP path to -- all from the fixture, i.e. from the reference alone."""

  def __init__(self, name, leg):
    z = np.load(os.path.join(GOLDEN, f"{name}_trajectory.npz"), allow_pickle=False)
    self.name, self.leg = name, leg
    over = dict(ast.literal_eval(str(z["hp_json"])))
    self.hp = HParams(**over)
    self.K, self.lr = int(z["K"]), float(z[f"{leg}/lr"])
    self.B, self.T, self.crop = int(z["B"]), int(z["T"]), int(z["crop"])
    self.full, self.nmin = int(z["sub_full"]), int(z["sub_min"])
    self.weight_seed = int(z["weight_seed"])
    g = lambda key: z[f"{leg}/{key}"]     # noqa: E731
    self.loss = g("loss").astype(np.float64)
    self.names = [str(n) for n in g("names")]
    self.numel = dict(zip(self.names, (int(v) for v in g("numel"))))
    self.dglobal = float(g("dglobal"))
    self.dnorm = dict(zip(self.names, (float(v) for v in g("dnorm"))))
    self.dsum = dict(zip(self.names, (float(v) for v in g("dsum"))))
    self.dhead = {n: torch.from_numpy(h[:min(8, self.numel[n])].copy()) for n, h in zip(self.names, g("dhead"))}
    flat, self.dsub, o = torch.from_numpy(g("dsub")), {}, 0
    for n in self.names:
      c = sub_count(self.numel[n], self.full, self.nmin)
      self.dsub[n] = flat[o:o + c]
      o += c
    assert o == flat.numel()
    self.yard = dict(zip(self.names, (float(v) for v in g("yard"))))
    self.yard_loss = g("yard_loss").astype(np.float64)
    self.yard_global_random, self.yard_global_fixed = float(g("yard_global_random")), float(g("yard_global_fixed"))
    self.faults = {f: (float(g(f"fault_{f}_loss")), float(g(f"fault_{f}_global")))
                   for f in ("skip", "stale") if f"{leg}/fault_{f}_loss" in z.files}

  def dfull(self, name):
    """The whole reference update of a tensor the fixture keeps whole, else None."""
    return self.dsub[name] if self.dsub[name].numel() == self.numel[name] else None

  def state_dict(self):
    return synthetic.to_weightnorm_form(synthetic.make_state_dict(self.hp, seed=self.weight_seed))

  def batches(self):
    return trajectory_batches(self.B, self.T, self.crop)

  # the bounds: the project's one-forward loss bound + the yardstick; the larger global yardstick itself (it already
  # assumes 5e-3 per gradient where the path measures 1.1e-3; a factor of 1.5 on top would let the Adam bound, 5.5e-2, pass
  # more than half of the stale-step fault, 7.8e-2: test_trajectory_cpu.py); 2 x the per-tensor yardstick (spread over
  # seeds about 25 %)
  def loss_bound(self, k):
    return 2e-3 * max(1.0, abs(self.loss[k])) + self.yard_loss[k]

  def global_bound(self):
    return max(self.yard_global_random, self.yard_global_fixed)

  def tensor_bound(self, name):
    return 2.0 * self.yard[name] * self.dnorm[name] + 1e-7

  def check(self, losses, delta, what, steps=None):
    """losses[k] for the steps in ``steps`` (default: all K + 1), delta {name: theta_K - theta_0} on the CPU."""
    steps = range(self.K + 1) if steps is None else steps
    lerr = [abs(float(losses[k]) - self.loss[k]) for k in steps]
    print(f"{what}: loss error per step", " ".join(f"{e:.2e}" for e in lerr),
          f"(worst {max(lerr):.2e}, bounds {self.loss_bound(steps[0]):.2e} .. {self.loss_bound(steps[-1]):.2e})")
    per, glob = sub_errors(delta, self.dsub, self.full, self.nmin)
    print(f"{what}: global update error {glob:.4e} (bound {self.global_bound():.4e})")
    worst = sorted(((e / max(r, 1e-30), n, e, r) for n, (e, r) in per.items()), reverse=True)
    for rel, n, e, r in worst[:8]:
      print(f"{what}: {n}: update rel {rel:.3e} (yardstick {self.yard[n]:.3e})")
    for k, e in zip(steps, lerr):
      assert e <= self.loss_bound(k), f"step {k}: loss off by {e:.3e}, bound {self.loss_bound(k):.3e}"
    assert glob <= self.global_bound(), f"global update error {glob:.4e}, bound {self.global_bound():.4e}"
    for rel, n, e, r in worst:
      d = delta[n].double()
      assert torch.isfinite(d).all(), n
      bound = self.tensor_bound(n)
      kept = 2.0 * self.yard[n] * r + 1e-7         # r: the reference update's norm over the kept values (= dnorm if whole)
      assert e <= kept, f"{n}: update error {e:.3e} over the kept values, bound {kept:.3e}"
      assert abs(float(d.norm()) - self.dnorm[n]) <= bound, f"{n}: update norm {float(d.norm()):.4e} vs {self.dnorm[n]:.4e}"
      h = self.dhead[n].double()
      assert float((d.flatten()[:h.numel()] - h).norm()) <= bound, f"{n}: first values of the update"
    return max(lerr), glob, worst[0]
