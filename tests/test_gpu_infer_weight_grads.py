"""GPU: ``WaveGlow.infer_differentiable(..., weight_grads=True)`` -- synthesis whose output carries a graph to the
vocoder's own parameters (and to mel / the noise as before).

Yardsticks: the reference's golden ``audio`` (values, RMS <= 1e-3), CPU fp32 autograd through
oracle.torch_oracle.infer_ref for every parameter gradient (``||g - g_ref|| <= 5e-3 ||g_ref|| + 1e-7``, the bound and floor
tests/test_gpu_train.py applies to the same tensors), and at full size the identity ``J_g,theta^T a = - J_f,theta^T u``
against the training direction's own weight gradients (pinned in fp64 by tests/test_infer_weight_grads_cpu.py).
"""
import pytest
import torch

from _cases import Case, rms
from waveglow_amd import synthetic
from waveglow_amd._lib import WgError
from waveglow_amd.hparams import HParams
from waveglow_amd.model import WaveGlow

pytestmark = pytest.mark.gpu

RMS_TOL = 1e-3           # tests/test_gpu_infer_grads.py: the project's parity bar
GRAD_TOL = 5e-3          # tests/test_gpu_train.py / test_gpu_infer_grads.py
DSPECT_TOL = 1e-4        # tests/test_gpu_recompute.py: gradients behind d spect, recompute vs full save
UPSAMPLE = ("upsample.weight", "upsample.bias")
# Full-size identity, relative L2 per parameter tensor.  Worst measured per group (MI355X): in_layers 1.76e-3, res_skip
# 2.15e-3, cond 1.54e-3, start 1.83e-3, end 2.07e-3, convinv 8.6e-4, upsample 1.19e-3.  3 x 2.15e-3 = 6.4e-3 is above the
# parity bar of the same tensors, so the bar is the bound.
IDENTITY_TOL = min(3 * 2.15e-3, GRAD_TOL)
GROUPS = ("in_layers", "res_skip_layers", "cond_layer", "start", "end", "convinv", "upsample")


@pytest.fixture(autouse=True)
def _poisoned_gradient_buffers(monkeypatch):
  """Gradient buffers start from NaN: a packed-gradient or output entry the library never writes makes grad_finite false."""
  monkeypatch.setenv("WG_TRAIN_POISON_GRADS", "1")


def _model(hp, sd, normed, trainable=True):
  m = WaveGlow(hp)
  if normed:
    m.load_state_dict(synthetic.to_weightnorm_form(sd))
  else:
    m = WaveGlow.remove_weightnorm(m)
    m.load_state_dict(sd)
  return m.to("cuda:0").train().requires_grad_(trainable)


def _inputs(c, rg=(True, True, True)):
  mel = c.mel.cuda().requires_grad_(rg[0])
  zi = c.z_init.cuda().requires_grad_(rg[1])
  ze = [c.z_early[k].cuda().requires_grad_(rg[2]) for k in sorted(c.z_early, reverse=True)]
  return mel, zi, ze


def _rel(g, ref):
  return float((g.double() - ref.double()).norm() / max(float(ref.double().norm()), 1e-30))


def _group(name):
  for g in GROUPS:
    if g in name:
      return g
  raise AssertionError(name)


def _golden(c, normed):
  return torch.from_numpy(c.npz["audio_from_weightnorm_ckpt"]) if normed else c.audio


def _r(c):
  return torch.randn(c.audio.shape, generator=torch.Generator().manual_seed(11)) / c.audio.numel()


def _run(c, normed, r, recompute=False, rg=(True, True, True), only=None):
  """One weight_grads=True call and its backward: (audio, {name: grad}, mel.grad, z_init.grad, [z_early grads], model)."""
  model = _model(c.hp, c.sd, normed)
  model.recompute_activations = recompute
  if only is not None:
    model.requires_grad_(False)
    for p in only(model).parameters():
      p.requires_grad_(True)
  mel, zi, ze = _inputs(c, rg)
  audio = model.infer_differentiable(mel, c.sigma, z_init=zi, z_early=ze, weight_grads=True)
  assert audio.requires_grad and audio.grad_fn is not None
  (audio * r.cuda()).sum().backward()
  torch.cuda.synchronize()
  assert bool(model.grad_finite), "an entry of a (NaN-poisoned) gradient buffer was left unwritten"
  grads = {n: (p.grad.detach().clone() if p.grad is not None else None) for n, p in model.named_parameters()}
  return audio.detach(), grads, mel.grad, zi.grad, [z.grad for z in ze], model


@pytest.mark.parametrize("name,normed", [("c64", False), ("c64", True), ("c256", False)])
def test_values_match_reference_audio(name, normed):
  c = Case(name)
  model = _model(c.hp, c.sd, normed)
  mel, zi, ze = _inputs(c, (False, False, False))
  audio = model.infer_differentiable(mel, c.sigma, z_init=zi, z_early=ze, weight_grads=True)
  assert audio.requires_grad and audio.grad_fn is not None
  torch.cuda.synchronize()
  ref = _golden(c, normed)
  err = rms(audio.detach().cpu() - ref)
  # the frozen path takes W^-1 from the finalised engine (host fp64), this one inverts on the device (fp64 Gauss-Jordan)
  frozen = _model(c.hp, c.sd, normed, trainable=False)
  m2, z2, e2 = _inputs(c)
  a_frozen = frozen.infer_differentiable(m2, c.sigma, z_init=z2, z_early=e2)
  d = float((audio.detach() - a_frozen.detach()).abs().max())
  print(f"{name} normed={normed}: rms err {err:.3e}; max abs difference to the frozen path's audio {d:.3e}")
  assert audio.shape == ref.shape and err <= RMS_TOL
  # measured 0 on all three cases: the device inverse runs the handle's algorithm (fp64 Gauss-Jordan, partial pivoting)
  # and rounds to the same fp32 matrices
  assert torch.equal(audio.detach(), a_frozen.detach())


def _oracle_grads(c, normed, r):
  """CPU fp32 autograd through infer_ref: ({parameter name: grad}, d mel, d z_init, [d z_early descending])."""
  from oracle import torch_oracle as O
  sd = synthetic.to_weightnorm_form(c.sd) if normed else c.sd
  leaves = {k: v.clone().requires_grad_(True) for k, v in sd.items()}
  v1, v0 = "parametrizations.weight.original1", "parametrizations.weight.original0"
  dense = {}
  for k, v in leaves.items():
    if k.endswith(v1):
      dense[k[:-len(v1)] + "weight"] = torch._weight_norm(v, leaves[k[:-len(v1)] + v0], 0)      # g v / ||v||
    elif not k.endswith(v0):
      dense[k] = v
  mel = c.mel.clone().requires_grad_(True)
  zi = c.z_init.clone().requires_grad_(True)
  ze = {k: v.clone().requires_grad_(True) for k, v in c.z_early.items()}
  x = O.infer_ref(dense, mel, zi, ze, c.sigma, c.oracle_cfg())
  keys = sorted(ze, reverse=True)
  names = list(leaves)
  gs = torch.autograd.grad((x * r).sum(), [leaves[n] for n in names] + [mel, zi] + [ze[k] for k in keys])
  n = len(names)
  return dict(zip(names, gs[:n])), gs[n], gs[n + 1], list(gs[n + 2:])


@pytest.mark.parametrize("name,normed", [("c64", False), ("c64", True), ("c256", False)])
def test_gradients_match_oracle(name, normed):
  c = Case(name)
  r = _r(c)
  o_par, o_mel, o_zi, o_ze = _oracle_grads(c, normed, r)
  audio, grads, g_mel, g_zi, g_ze, model = _run(c, normed, r)
  assert set(grads) == set(o_par) and len(grads) == len(list(model.parameters()))
  worst = []
  for pname, ref in o_par.items():
    g = grads[pname]
    assert g is not None and g.shape == ref.shape, pname
    assert torch.isfinite(g).all(), pname
    err, den = float((g.cpu() - ref).norm()), float(ref.norm())
    worst.append((err / max(den, 1e-12), pname, err, den))
  worst.sort(reverse=True)
  for rel, pname, err, den in worst[:8]:
    print(f"{name} normed={normed}: {pname}: rel {rel:.3e} (err {err:.3e}, ref norm {den:.3e})")
  for rel, pname, err, den in worst:
    assert err <= GRAD_TOL * den + 1e-7, f"{pname}: gradient error {err:.3e} vs norm {den:.3e}"
  for what, g, ref in [("d mel", g_mel, o_mel), ("d z_init", g_zi, o_zi)] + \
                      [(f"d z_early[{i}]", z, o) for i, (z, o) in enumerate(zip(g_ze, o_ze))]:
    assert g is not None and g.shape == ref.shape, what
    e = _rel(g.cpu(), ref)
    print(f"{name} normed={normed} {what}: rel {e:.3e}")
    assert e <= GRAD_TOL, what
  # the device W^-1 is bit-equal to the handle's on these cases (test_values_match_reference_audio): the data-gradient
  # chain is the frozen call's, launch by launch, so the input gradients are the frozen call's bit for bit
  frozen = _model(c.hp, c.sd, normed, trainable=False)
  mel, zi, ze = _inputs(c)
  (frozen.infer_differentiable(mel, c.sigma, z_init=zi, z_early=ze) * r.cuda()).sum().backward()
  assert torch.equal(mel.grad, g_mel) and torch.equal(zi.grad, g_zi)
  assert all(torch.equal(z.grad, g) for z, g in zip(ze, g_ze))


def test_full_size_weight_identity():
  """configs[3] shapes (batch 32 x 63 frames, 256 channels), synthetic weight-normed model: backpropagating
  a = J_fx^T u through x = g(z, mel; theta) gives, for every parameter, minus the training direction's gradient of
  (z * u).sum() (tests/test_infer_weight_grads_cpu.py).  Both sides are gradients through fp16 planes."""
  hp = HParams()
  B, T, sigma = 32, 63, 0.6
  model = _model(hp, synthetic.make_state_dict(hp, seed=0), normed=True)
  L = 32 * T
  gen = torch.Generator(device="cuda:0").manual_seed(5)
  mel = synthetic.make_mel(B, T, seed=7).cuda()
  zi = torch.randn(B, model.n_remaining_channels, L, device="cuda:0", generator=gen)
  ks = [k for k in reversed(range(hp.n_flows)) if k % hp.n_early_every == 0 and k > 0]
  ze = [torch.randn(B, hp.n_early_size, L, device="cuda:0", generator=gen) for _ in ks]
  x = model.infer_differentiable(mel, sigma, z_init=zi, z_early=ze, weight_grads=True)
  u = torch.randn(B, hp.n_group, L, device="cuda:0", generator=gen) / (B * hp.n_group * L)
  x0 = x.detach().requires_grad_(True)
  z, _, _ = model((mel, x0))
  (z * u).sum().backward()
  assert bool(model.grad_finite)
  a = x0.grad
  rhs = {n: p.grad.detach().clone() for n, p in model.named_parameters()}
  model.zero_grad(set_to_none=True)
  x.backward(a)
  torch.cuda.synchronize()
  assert bool(model.grad_finite)
  lhs = {n: p.grad for n, p in model.named_parameters()}
  assert all(g is not None for g in lhs.values()) and len(lhs) == 686
  gmax = {g: 0.0 for g in GROUPS}
  for n, ref in rhs.items():
    gmax[_group(n)] = max(gmax[_group(n)], float(ref.norm()))
  worst = {g: (0.0, "") for g in GROUPS}
  fails = []
  for n, ref in rhs.items():
    grp = _group(n)
    err, den = float((lhs[n].double() + ref.double()).norm()), float(ref.norm())
    # a tensor far below its group's largest: the absolute floor of tests/test_gpu_train.py:379
    den_eff = max(den, 1e-3 * gmax[grp])
    rel = err / max(den_eff, 1e-30)
    if rel > worst[grp][0]:
      worst[grp] = (rel, n)
    if err > IDENTITY_TOL * den_eff + 1e-7:
      fails.append((n, err, den))
  print("full-size weight identity, worst relative L2 per group:",
        {g: f"{v:.3e} ({n})" for g, (v, n) in worst.items()})
  assert not fails, fails[:8]


def test_only_what_is_asked_for():
  c = Case("c64")
  r = _r(c)
  _, g_all, g_mel, _, _, _ = _run(c, True, r)
  _, g_one, mel_grad, zi_grad, ze_grad, model = _run(c, True, r, rg=(False, False, False), only=lambda m: m.WN[3])
  asked = {"WN.3." + n for n, _ in model.WN[3].named_parameters()}
  assert asked and asked <= set(g_one)
  for n, g in g_one.items():
    if n in asked:
      assert g is not None and torch.equal(g, g_all[n]), n
    else:
      assert g is None, n
  # parameters trainable, inputs not: no input gradient
  assert mel_grad is None and zi_grad is None and all(g is None for g in ze_grad)
  _, g_par, mel_grad, _, _, _ = _run(c, True, r, rg=(False, True, False))
  assert mel_grad is None
  for n in g_all:
    assert torch.equal(g_par[n], g_all[n]), n
  # nothing trainable, no input gradient: infer_with_noise
  frozen = _model(c.hp, c.sd, True, trainable=False)
  mel, zi, ze = _inputs(c, (False, False, False))
  out = frozen.infer_differentiable(mel, c.sigma, z_init=zi, z_early=ze, weight_grads=True)
  with torch.no_grad():
    ref = frozen.infer_with_noise(mel, zi, ze, c.sigma)
  assert out.grad_fn is None and torch.equal(out, ref)


@pytest.mark.parametrize("name,normed", [("c64", True), ("c256", False)])
def test_recompute_equals_full_save(name, normed):
  c = Case(name)
  r = _r(c)
  a_f, g_f, mel_f, zi_f, ze_f, _ = _run(c, normed, r, recompute=False)
  a_r, g_r, mel_r, zi_r, ze_r, _ = _run(c, normed, r, recompute=True)
  assert torch.equal(a_r, a_f)
  for n in g_f:
    if n in UPSAMPLE:
      rel = _rel(g_r[n], g_f[n])
      print(f"{name}: {n} rel {rel:.3e}")
      assert rel <= DSPECT_TOL, (n, rel)
    else:
      assert torch.equal(g_r[n], g_f[n]), n
  assert _rel(mel_r, mel_f) <= DSPECT_TOL
  assert torch.equal(zi_r, zi_f) and all(torch.equal(x, y) for x, y in zip(ze_r, ze_f))


@pytest.mark.parametrize("name,normed,recompute", [("c64", True, False), ("c256", False, False), ("c256", False, True)])
def test_single_stream_mode_is_bit_identical(name, normed, recompute, monkeypatch):
  """The weight-gradient launches run on a low-priority stream beside the data-gradient chain, their reductions on a third;
  WG_TRAIN_SERIAL=1 keeps everything on the caller's stream.  Same gradients bit for bit, twice in a row."""
  c = Case(name)
  r = _r(c)
  a_c, g_c, mel_c, zi_c, ze_c, _ = _run(c, normed, r, recompute=recompute)
  a_c2, g_c2, mel_c2, _, _, _ = _run(c, normed, r, recompute=recompute)
  monkeypatch.setenv("WG_TRAIN_SERIAL", "1")
  a_s, g_s, mel_s, zi_s, ze_s, _ = _run(c, normed, r, recompute=recompute)
  assert torch.equal(a_s, a_c) and torch.equal(a_c2, a_c)
  for n in g_s:
    assert torch.equal(g_s[n], g_c[n]), n
    assert torch.equal(g_c2[n], g_c[n]), n
  assert torch.equal(mel_s, mel_c) and torch.equal(mel_c2, mel_c) and torch.equal(zi_s, zi_c)
  assert all(torch.equal(x, y) for x, y in zip(ze_s, ze_c))


def test_optimiser_moves_the_loss():
  """Adam on the weight-normed c64 model, fixed mel and noise, target = 0.9 x the golden audio.  The weights change every
  step, so every forward must invert the CURRENT 1x1 matrices: its output is held to infer_with_noise of the same weights."""
  c = Case("c64")
  model = _model(c.hp, c.sd, True)
  opt = torch.optim.Adam(model.parameters(), lr=1e-4)
  mel, zi, ze = _inputs(c, (False, False, False))
  target = (0.9 * _golden(c, True)).cuda()
  losses, sigs = [], []
  for step in range(11):
    sigs.append(model._weights_signature())
    audio = model.infer_differentiable(mel, c.sigma, z_init=zi, z_early=ze, weight_grads=True)
    # the inference engine was not re-finalised for this call
    assert model._engine.signature != sigs[-1]
    loss = torch.nn.functional.mse_loss(audio, target)
    losses.append(float(loss.detach()))
    if step == 10:
      break
    opt.zero_grad()
    loss.backward()
    assert bool(model.grad_finite), step
    with torch.no_grad():
      ref = model.infer_with_noise(mel, zi, ze, c.sigma)
    e = rms((audio.detach() - ref).cpu())
    assert e <= RMS_TOL, (step, e)
    opt.step()
  assert len(set(sigs)) == len(sigs), "the weights' versions did not change every step"
  print("losses:", " ".join(f"{v:.6e}" for v in losses))
  assert losses[10] < losses[0]


def test_singular_matrix_gives_non_finite_output():
  c = Case("c64")
  model = _model(c.hp, c.sd, False)
  with torch.no_grad():
    model.convinv[1].conv.weight.zero_()
  mel, zi, ze = _inputs(c, (False, False, False))
  audio = model.infer_differentiable(mel, c.sigma, z_init=zi, z_early=ze, weight_grads=True)
  audio.sum().backward()
  torch.cuda.synchronize()
  assert not bool(torch.isfinite(audio).all())
  assert not bool(model.grad_finite)


def test_refusals():
  tiny = Case("tiny")
  model = _model(tiny.hp, tiny.sd, False)
  with pytest.raises(WgError):
    model.infer_differentiable(tiny.mel.cuda(), tiny.sigma, weight_grads=True)
  c = Case("c64")
  model = _model(c.hp, c.sd, False)
  with pytest.raises(WgError):
    model.infer_differentiable(c.mel.cuda().half(), c.sigma, weight_grads=True)
  mel, zi, ze = _inputs(c)
  model.ddp_group = object()
  with pytest.raises(WgError, match="process group"):
    model.infer_differentiable(mel, c.sigma, z_init=zi, z_early=ze, weight_grads=True)
  model.ddp_group = None
  # the weights moved between the call and its backward(): the saved state belongs to the old weights
  y = model.infer_differentiable(mel, c.sigma, z_init=zi, z_early=ze, weight_grads=True)
  with torch.no_grad():
    model.WN[0].start.bias.add_(1.0)
  with pytest.raises(WgError):
    y.sum().backward()
  # retain_graph stays unsupported
  y = model.infer_differentiable(mel, c.sigma, z_init=zi, z_early=ze, weight_grads=True)
  y.sum().backward(retain_graph=True)
  with pytest.raises(WgError):
    y.sum().backward()
