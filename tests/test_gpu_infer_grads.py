"""GPU: ``WaveGlow.infer_differentiable`` -- synthesis whose output carries a graph back to mel and to the noise.

Yardsticks: the reference's own ``audio`` of the golden cases (values, RMS <= 1e-3 as test_gpu_parity.py), CPU fp32
autograd through oracle.torch_oracle.infer_ref (gradients, ``||g - g_ref|| <= 5e-3 ||g_ref||`` as the other input
gradients), and at full size the inverse identity ``f(g(z, mel), mel) = sigma P z`` against the training direction's own
input gradients (pinned in fp64 by tests/test_infer_grads_cpu.py).
"""
import pytest
import torch

from _cases import Case, oracle_cfg_from_hp, rms
from test_infer_grads_cpu import early_channel_map
from waveglow_amd import synthetic
from waveglow_amd._lib import WgError
from waveglow_amd.hparams import HParams
from waveglow_amd.model import WaveGlow

pytestmark = pytest.mark.gpu

RMS_TOL = 1e-3
GRAD_TOL = 5e-3
IDENTITY_TOL = 3e-3      # measured 4.1e-4 .. 8.9e-4 (d mel the largest)


@pytest.fixture(autouse=True)
def _poisoned_gradient_buffers(monkeypatch):
  """Gradient outputs start from NaN: an entry the library never writes makes grad_finite false."""
  monkeypatch.setenv("WG_TRAIN_POISON_GRADS", "1")


def _frozen(hp, sd, normed=False):
  m = WaveGlow(hp)
  if normed:
    m.load_state_dict(synthetic.to_weightnorm_form(sd))
  else:
    m = WaveGlow.remove_weightnorm(m)
    m.load_state_dict(sd)
  return m.to("cuda:0").eval().requires_grad_(False)


def _inputs(c, rg=(True, True, True)):
  mel = c.mel.cuda().requires_grad_(rg[0])
  zi = c.z_init.cuda().requires_grad_(rg[1])
  ze = [c.z_early[k].cuda().requires_grad_(rg[2]) for k in sorted(c.z_early, reverse=True)]
  return mel, zi, ze


def _rel(g, ref):
  return float((g.double() - ref.double()).norm() / ref.double().norm())


@pytest.mark.parametrize("name,normed", [("c64", False), ("c64", True), ("c256", False)])
def test_values_match_reference_audio(name, normed):
  c = Case(name)
  model = _frozen(c.hp, c.sd, normed)
  mel, zi, ze = _inputs(c)
  audio = model.infer_differentiable(mel, c.sigma, z_init=zi, z_early=ze)
  assert audio.requires_grad and audio.grad_fn is not None
  torch.cuda.synchronize()
  ref = torch.from_numpy(c.npz["audio_from_weightnorm_ckpt"]) if normed else c.audio
  err = rms(audio.detach().cpu() - ref)
  print(f"{name} normed={normed}: rms err {err:.3e}")
  assert audio.shape == ref.shape and err <= RMS_TOL


def _oracle_grads(c, r):
  from oracle import torch_oracle as O
  mel = c.mel.clone().requires_grad_(True)
  zi = c.z_init.clone().requires_grad_(True)
  ze = {k: v.clone().requires_grad_(True) for k, v in c.z_early.items()}
  x = O.infer_ref(c.sd, mel, zi, ze, c.sigma, c.oracle_cfg())
  keys = sorted(ze, reverse=True)
  gs = torch.autograd.grad((x * r).sum(), [mel, zi] + [ze[k] for k in keys])
  return gs[0], gs[1], list(gs[2:])


@pytest.mark.parametrize("name,normed", [("c64", False), ("c64", True), ("c256", False)])
def test_gradients_match_oracle(name, normed):
  c = Case(name)
  model = _frozen(c.hp, c.sd, normed)
  r = torch.randn(c.audio.shape, generator=torch.Generator().manual_seed(11)) / c.audio.numel()
  o_mel, o_zi, o_ze = _oracle_grads(c, r)
  mel, zi, ze = _inputs(c)
  (model.infer_differentiable(mel, c.sigma, z_init=zi, z_early=ze) * r.cuda()).sum().backward()
  torch.cuda.synchronize()
  assert bool(model.grad_finite)
  for what, g, ref in [("d mel", mel.grad, o_mel), ("d z_init", zi.grad, o_zi)] + \
                      [(f"d z_early[{i}]", z.grad, o) for i, (z, o) in enumerate(zip(ze, o_ze))]:
    assert g is not None and g.shape == ref.shape, what
    e = _rel(g.cpu(), ref)
    print(f"{name} normed={normed} {what}: rel {e:.3e}")
    assert e <= GRAD_TOL, what
  assert all(p.grad is None for p in model.parameters())
  # only what is asked for: mel alone, then the first early noise alone -- the same values
  mel2, zi2, ze2 = _inputs(c, (True, False, False))
  (model.infer_differentiable(mel2, c.sigma, z_init=zi2, z_early=ze2) * r.cuda()).sum().backward()
  assert zi2.grad is None and all(z.grad is None for z in ze2)
  assert torch.equal(mel2.grad, mel.grad)
  mel3, zi3, ze3 = _inputs(c, (False, False, False))
  ze3[0].requires_grad_(True)
  (model.infer_differentiable(mel3, c.sigma, z_init=zi3, z_early=ze3) * r.cuda()).sum().backward()
  assert mel3.grad is None and zi3.grad is None and all(z.grad is None for z in ze3[1:])
  assert torch.equal(ze3[0].grad, ze[0].grad)
  assert all(p.grad is None for p in model.parameters())


def test_full_size_inverse_identity():
  """configs[3] shapes (batch 32 x 63 frames, 256 channels): backpropagating a = J_fx^T u through x = g(z, mel) gives
  d z = sigma P^T u and d mel = -J_fmel^T u (see tests/test_infer_grads_cpu.py)."""
  hp = HParams()
  B, T, sigma = 32, 63, 0.6
  model = _frozen(hp, synthetic.make_state_dict(hp, seed=0))
  cfg = oracle_cfg_from_hp(hp)
  early, n_e = early_channel_map(cfg)
  L = 32 * T
  gen = torch.Generator(device="cuda:0").manual_seed(5)
  mel = synthetic.make_mel(B, T, seed=7).cuda().requires_grad_(True)
  zi = torch.randn(B, model.n_remaining_channels, L, device="cuda:0", generator=gen).requires_grad_(True)
  ks = [k for k in reversed(range(hp.n_flows)) if k % hp.n_early_every == 0 and k > 0]
  ze = [torch.randn(B, hp.n_early_size, L, device="cuda:0", generator=gen).requires_grad_(True) for _ in ks]
  x = model.infer_differentiable(mel, sigma, z_init=zi, z_early=ze)
  u = torch.randn(B, hp.n_group, L, device="cuda:0", generator=gen) / (B * hp.n_group * L)
  x0 = x.detach().requires_grad_(True)
  mel0 = mel.detach().requires_grad_(True)
  z, _, _ = model((mel0, x0))
  (z * u).sum().backward()
  assert bool(model.grad_finite)
  a, m = x0.grad, mel0.grad
  x.backward(a)
  torch.cuda.synchronize()
  assert bool(model.grad_finite)
  errs = {"d z_init": _rel(zi.grad, sigma * u[:, n_e:]), "d mel": _rel(mel.grad, -m)}
  for k, z in zip(ks, ze):
    errs[f"d z_early (flow {k})"] = _rel(z.grad, sigma * u[:, early[k]:early[k] + hp.n_early_size])
  print("full-size inverse identity, relative L2:", {k: f"{v:.3e}" for k, v in errs.items()})
  for k, v in errs.items():
    assert v <= IDENTITY_TOL, (k, v)


def test_bookkeeping():
  c = Case("c256")
  model = _frozen(c.hp, c.sd)
  r = (torch.randn(c.audio.shape, generator=torch.Generator().manual_seed(2)) / c.audio.numel()).cuda()
  mel, zi, ze = _inputs(c)
  # grad mode off: infer_with_noise bit for bit, and so is a call whose inputs need no gradient
  with torch.no_grad():
    ref = model.infer_with_noise(mel, zi, ze, c.sigma)
    out = model.infer_differentiable(mel, c.sigma, z_init=zi, z_early=ze)
  assert torch.equal(out, ref) and out.grad_fn is None
  m0, z0, e0 = _inputs(c, (False, False, False))
  out = model.infer_differentiable(m0, c.sigma, z_init=z0, z_early=e0)
  assert torch.equal(out, ref) and out.grad_fn is None
  # default noise: drawn as infer draws it
  torch.manual_seed(9)
  ref_inf = model.infer(mel.detach(), c.sigma)
  torch.manual_seed(9)
  out_d = model.infer_differentiable(mel, c.sigma)
  assert rms((out_d.detach() - ref_inf).cpu()) <= RMS_TOL
  # two outstanding graphs backpropagated together = the two separate runs
  mel_b = (mel.detach() * 0.9).requires_grad_(True)
  sep = []
  for m in (mel, mel_b):
    mm = m.detach().requires_grad_(True)
    (model.infer_differentiable(mm, c.sigma, z_init=zi.detach(), z_early=[z.detach() for z in ze]) * r).sum().backward()
    sep.append(mm.grad)
  m1, m2 = mel.detach().requires_grad_(True), mel_b.detach().requires_grad_(True)
  y1 = model.infer_differentiable(m1, c.sigma, z_init=zi.detach(), z_early=[z.detach() for z in ze])
  y2 = model.infer_differentiable(m2, c.sigma, z_init=zi.detach(), z_early=[z.detach() for z in ze])
  ((y1 * r).sum() + (y2 * r).sum()).backward()
  assert torch.equal(m1.grad, sep[0]) and torch.equal(m2.grad, sep[1])
  # a loss scale far too large overflows the fp16 planes: reported, not hidden
  model.grad_scale = 1e30
  m3 = mel.detach().requires_grad_(True)
  (model.infer_differentiable(m3, c.sigma, z_init=zi.detach(), z_early=[z.detach() for z in ze]) * r).sum().backward()
  assert not bool(model.grad_finite)
  del model.grad_scale
  (model.infer_differentiable(m3, c.sigma, z_init=zi.detach(), z_early=[z.detach() for z in ze]) * r).sum().backward()
  assert bool(model.grad_finite)


def test_refusals():
  tiny = Case("tiny")
  model = _frozen(tiny.hp, tiny.sd)
  with pytest.raises(WgError):
    model.infer_differentiable(tiny.mel.cuda().requires_grad_(True), tiny.sigma)
  c = Case("c64")
  model = _frozen(c.hp, c.sd)
  with pytest.raises(WgError):
    model.infer_differentiable(c.mel.cuda().half().requires_grad_(True), c.sigma)
  mel, zi, ze = _inputs(c)
  y = model.infer_differentiable(mel, c.sigma, z_init=zi, z_early=ze)
  y.sum().backward(retain_graph=True)
  with pytest.raises(WgError):
    y.sum().backward()
  model.WN[0].start.bias.requires_grad_(True)
  with pytest.raises(WgError):
    model.infer_differentiable(c.mel.cuda().requires_grad_(True), c.sigma)
