"""Weight-normed checkpoints away from g = ||v||, without moving any dense weight.

``synthetic.to_weightnorm_form`` sets g = ||v|| row by row, so the row scale s = g / ||v|| that the training plumbing
computes (csrc/train_prep.hip: rownorm_kernel) and applies (pack_kernel, wes_fold_kernel, end_grad_kernel,
small_prep_kernel, wn_grad_kernel) is 1 everywhere: a wrong index into the scale arrays, an ``s`` left out of d v, or g and
||v|| exchanged change nothing.  ``reparametrise`` draws one u per output row of every weight-normed module and sets

    v_off = v / u        g_off = sign(u) g

The dense weight g v / ||v|| is the same up to fp32 rounding, so the forward, the loss and the gradient of everything that is
not a (g, v) pair are unchanged and keep their references and bounds; the scale is now s = u, and

    d g_off = sign(u) d g_on        d v_off = u d v_on      (row by row)

``to_on_metric`` undoes the two factors: a gradient in that form is weighted exactly like the on-manifold one, so the
bound of tests/_cases.py (GRAD_TOL) applies to it as it stands.  One exception: a row of length 1 (``start`` of a flow with
h_k = 1) has d v = 0 in exact arithmetic -- both sides are rounding noise, compared with the absolute floor only.
"""
import zlib

import torch

from _cases import GRAD_TOL

V0 = "parametrizations.weight.original0"
V1 = "parametrizations.weight.original1"
FLOOR = 1e-7          # the absolute floor of _cases._check


def _draw(n, key, seed, span, neg_share):
  g = torch.Generator().manual_seed((zlib.crc32(key.encode()) ^ (seed * 0x9E3779B1)) & 0x7FFFFFFF)
  mag = torch.exp((torch.rand(n, generator=g, dtype=torch.float64) * 2 - 1) * torch.log(torch.tensor(span, dtype=torch.float64)))
  neg = torch.rand(n, generator=g, dtype=torch.float64) < neg_share
  return torch.where(neg, -mag, mag).float()


def _covers(u):
  return bool((u < 0).any()) and bool((u.abs() < 0.5).any()) and bool((u.abs() > 2.0).any())


def reparametrise(sd_normed, seed, span=4.0, neg_share=0.125):
  """(state dict with v / u and sign(u) g, {module prefix: u [rows]}).  |u| is log-uniform in [1 / span, span], a share
  ``neg_share`` of the rows negative.  Every module must hold a negative row, a row with |u| < 1/2 and one with |u| > 2: a
  draw that misses one of them for any module is thrown away and the next seed taken."""
  prefixes = [k[:-len(V1)] for k in sd_normed if k.endswith(V1)]
  assert prefixes, "no weight-normed module in this state dict"
  for s in range(seed, seed + 64):
    U = {p: _draw(sd_normed[p + V1].shape[0], p, s, span, neg_share) for p in prefixes}
    if all(_covers(u) for u in U.values()):
      break
  for p, u in U.items():
    assert _covers(u), f"{p}: the draw misses a negative, a small or a large row scale"
    assert float(u.abs().min()) >= 1.0 / span * (1 - 1e-6) and float(u.abs().max()) <= span * (1 + 1e-6), p
  out = {}
  for k, t in sd_normed.items():
    if k.endswith(V1):
      out[k] = t / U[k[:-len(V1)]].view(-1, 1, 1)
    elif k.endswith(V0):
      out[k] = t * torch.sign(U[k[:-len(V0)]]).view(-1, 1, 1)
    else:
      out[k] = t.clone()
  return out, U


def to_on_metric(grads, U):
  """Gradients of a reparametrised model in the weighting of the on-manifold one: d v / u and sign(u) d g per row."""
  out = dict(grads)
  for p, u in U.items():
    u = u.to(grads[p + V1].device)
    out[p + V1] = grads[p + V1] / u.view(-1, 1, 1)
    out[p + V0] = grads[p + V0] * torch.sign(u).view(-1, 1, 1)
  return out


def floor_only_names(sd_normed):
  """The v tensors whose rows have length 1 (d v = 0 exactly)."""
  return tuple(k for k, t in sd_normed.items() if k.endswith(V1) and t[0].numel() == 1)


def dense_of(sd_normed):
  """The 470-key dense form, composed as the parametrization composes it (torch._weight_norm)."""
  dense = {}
  for k, t in sd_normed.items():
    if k.endswith(V1):
      dense[k[:-len(V1)] + "weight"] = torch._weight_norm(t, sd_normed[k[:-len(V1)] + V0], 0)
    elif not k.endswith(V0):
      dense[k] = t
  return dense


def check(grads, ref, what, floor_only=(), tol=GRAD_TOL):
  """_cases._check with the names in ``floor_only`` held to the absolute floor alone.  Prints the worst tensors and returns
  the worst relative error among the others."""
  worst = []
  for name, g_ref in ref.items():
    g = grads[name].cpu()
    assert g.shape == g_ref.shape, name
    assert torch.isfinite(g).all(), name
    err = float((g - g_ref).norm())
    if name in floor_only:
      print(f"{what}: {name}: floor only: err {err:.3e} (ref norm {float(g_ref.norm()):.3e})")
      assert err <= FLOOR, f"{name}: {err:.3e} where the gradient is zero"
      continue
    den = float(g_ref.norm())
    worst.append((err / max(den, 1e-12), name, err, den))
  worst.sort(reverse=True)
  for rel, name, err, den in worst[:6]:
    print(f"{what}: {name}: rel {rel:.3e} (err {err:.3e}, ref norm {den:.3e})")
  for rel, name, err, den in worst:
    assert err <= tol * den + FLOOR, f"{what}: {name}: gradient error {err:.3e} vs norm {den:.3e}"
  return worst[0][0]


def raw_worst(grads, ref, skip=()):
  """Worst per-tensor relative L2 of the untransformed gradients (printed beside the on-manifold metric)."""
  return max((float((grads[n].cpu() - r).norm()) / max(float(r.norm()), 1e-12), n) for n, r in ref.items() if n not in skip)


def oracle_infer_grads(sd_normed, c, r):
  """CPU fp32 autograd through oracle.infer_ref on torch._weight_norm leaves (the construction of
  tests/test_gpu_infer_weight_grads.py: _oracle_grads) for ANY weight-normed state dict: (audio, {parameter name: grad},
  d mel, d z_init, [d z_early, descending k])."""
  from oracle import torch_oracle as O
  leaves = {k: v.clone().requires_grad_(True) for k, v in sd_normed.items()}
  dense = dense_of(leaves)
  mel = c.mel.clone().requires_grad_(True)
  zi = c.z_init.clone().requires_grad_(True)
  ze = {k: v.clone().requires_grad_(True) for k, v in c.z_early.items()}
  x = O.infer_ref(dense, mel, zi, ze, c.sigma, c.oracle_cfg())
  keys = sorted(ze, reverse=True)
  names = list(leaves)
  gs = torch.autograd.grad((x * r).sum(), [leaves[n] for n in names] + [mel, zi] + [ze[k] for k in keys])
  n = len(names)
  return x.detach(), dict(zip(names, gs[:n])), gs[n], gs[n + 1], list(gs[n + 2:])
