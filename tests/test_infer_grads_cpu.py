"""CPU: the yardstick of the full-size inverse identity in tests/test_gpu_infer_grads.py, pinned in fp64 with the oracle.

``x = g(z, mel)`` is synthesis (oracle.torch_oracle.infer_ref), ``f`` the training forward (forward_ref).  Then
``f(g(z, mel), mel) = sigma P z``, where P puts z_init / z_early onto the channels of forward's z (model.py:201-203, :220),
and for any u, with ``a = J_fx^T u`` and ``m = J_fmel^T u``:  ``J_gz^T a = sigma P^T u``  and  ``J_gmel^T a = -m``.
Also: infer_differentiable refuses CPU tensors."""
import pytest
import torch

from _cases import Case, oracle_cfg_from_hp
from waveglow_amd._lib import WgError
from waveglow_amd.model import WaveGlow


class _F64(torch.Tensor):
  """infer_ref inverts W through ``W.float()`` (model.py:54); this tensor type keeps fp64 there."""

  def float(self, *args, **kwargs):
    return self.double()


def early_channel_map(cfg):
  """{flow k: channel offset of its early output in forward's z}; the remaining channels (z_init) come last."""
  out, off = {}, 0
  for k in cfg.early_flows():
    out[k] = off
    off += cfg.n_early_size
  return out, off


def _fp64_case():
  c = Case("c64")
  w = {k: v.double() for k, v in c.sd.items()}
  for k in range(c.hp.n_flows):
    key = f"convinv.{k}.conv.weight"
    w[key] = w[key].as_subclass(_F64)
  return c, w


def _plain(t):
  return t.as_subclass(torch.Tensor) if isinstance(t, _F64) else t


def test_channel_map_and_inverse_identity_fp64():
  from oracle import torch_oracle as O
  c, w = _fp64_case()
  cfg = c.oracle_cfg()
  early, n_e = early_channel_map(cfg)
  assert n_e + c.z_init.shape[1] == c.hp.n_group
  mel, zi = c.mel.double(), c.z_init.double()
  ze = {k: v.double() for k, v in c.z_early.items()}
  x = _plain(O.infer_ref(w, mel, zi, ze, c.sigma, cfg))
  z, _, _ = O.forward_ref(w, mel, x, cfg)
  z = _plain(z)
  want = torch.zeros_like(z)
  for k, off in early.items():
    want[:, off:off + cfg.n_early_size] = c.sigma * ze[k]
  want[:, n_e:] = c.sigma * zi
  err = float((z - want).norm() / want.norm())
  assert err <= 1e-12, err


def test_inverse_identity_jacobians_fp64():
  from oracle import torch_oracle as O
  c, w = _fp64_case()
  cfg = c.oracle_cfg()
  early, n_e = early_channel_map(cfg)
  mel = c.mel.double().requires_grad_(True)
  zi = c.z_init.double().requires_grad_(True)
  ze = {k: v.double().requires_grad_(True) for k, v in c.z_early.items()}
  x = _plain(O.infer_ref(w, mel, zi, ze, c.sigma, cfg))
  u = torch.randn(x.shape[0], cfg.n_group, x.shape[1] // cfg.n_group, generator=torch.Generator().manual_seed(3),
                  dtype=torch.float64)
  # a = J_fx^T u, m = J_fmel^T u at x = g(z, mel)
  x0 = x.detach().requires_grad_(True)
  mel0 = mel.detach().requires_grad_(True)
  z, _, _ = O.forward_ref(w, mel0, x0, cfg)
  a, m = torch.autograd.grad((_plain(z) * u).sum(), [x0, mel0])
  # backpropagating a through x
  gs = torch.autograd.grad(x, [mel, zi] + [ze[k] for k in sorted(ze)], grad_outputs=a)
  g_mel, g_zi, g_ze = gs[0], gs[1], dict(zip(sorted(ze), gs[2:]))
  rel = lambda g, r: float((_plain(g) - r).norm() / r.norm())
  assert rel(g_zi, c.sigma * u[:, n_e:]) <= 1e-10
  for k, off in early.items():
    assert rel(g_ze[k], c.sigma * u[:, off:off + cfg.n_early_size]) <= 1e-10, k
  assert rel(g_mel, -_plain(m)) <= 1e-10


def test_cpu_inputs_raise():
  c = Case("c64")
  model = WaveGlow.remove_weightnorm(WaveGlow(c.hp))
  model.load_state_dict(c.sd)
  model.requires_grad_(False)
  mel = c.mel.clone().requires_grad_(True)
  with pytest.raises(WgError):
    model.infer_differentiable(mel, c.sigma)
  ze = [c.z_early[k] for k in sorted(c.z_early, reverse=True)]
  with pytest.raises(WgError):
    model.infer_differentiable(mel, c.sigma, z_init=c.z_init, z_early=ze)
