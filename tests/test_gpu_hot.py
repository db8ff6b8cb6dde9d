"""GPU: every direction of the library at the dynamic range of a TRAINED checkpoint (tests/_hot.py).

Every other GPU test draws its weights from ``synthetic.make_state_dict``: gate pre-activations below about 6, ``log_s``
below 0.7, every 1x1 matrix exactly orthogonal.  There ``W^-1 = W^T``, ``logdet W = 0`` and ``e^{+-s}`` is within 1.5x of 1,
and the clamps of the gate (kernels.hip: gate_act / gate_act3) never act.  The hot cases have saturated gates (max |a| 31 ...
98, sigmoid arguments down to -105), ``log_s`` up to 8.7 and 1x1 matrices of condition 5 ... 53 with a non-zero logdet
(tests/test_hot_cpu.py asserts all of that on the oracle).

Yardstick: the fp64 oracle evaluated on the inputs the kernel really receives.  Bound, per compared quantity: 3 x the error
of the fp16-operand emulation of the documented design against the same oracle, read from the case's fixture
(tests/golden/hot_*.npz, make_golden_hot.py; DESIGN.md section 4 has the reasoning and the measured ratios), plus the
absolute floor of ``_cases._check``.  Every test prints error, yardstick and ratio per quantity.
"""
import functools

import pytest
import torch

import _hot as H
import test_gpu_infer_grads as IG
import test_gpu_infer_weight_grads as WGT
import test_gpu_recompute as RC
from test_gpu_input_grads import _model as _ig_model, _step as _ig_step
from test_gpu_parity import build_model, gpu_infer
from test_gpu_train import _gpu_step
from waveglow_amd.model import WaveGlowLoss

pytestmark = pytest.mark.gpu

EVEN_BATCH = [n for n in H.IDS if H.CASES[n][1] % 2 == 0]       # the half-batch chains need two utterances


@pytest.fixture(autouse=True)
def _poisoned_gradient_buffers(monkeypatch):
  """Gradient buffers start from NaN: an entry the library never writes makes grad_finite false."""
  monkeypatch.setenv("WG_TRAIN_POISON_GRADS", "1")


@functools.lru_cache(maxsize=None)
def _case(name, direction):
  return H.Hot(name, direction)


@functools.lru_cache(maxsize=None)
def _oracle(name, direction, normed, grads=True, io16=False):
  """The fp64 oracle of a case: one training step ("fwd") or synthesis with the backward of sum(audio r) ("inv"), on the
  dense or the weight-norm form, optionally on fp16-rounded inputs.  Computed once, shared, never modified."""
  c = _case(name, direction)
  sd = c.sdn if normed else c.sd
  inputs = c.inputs
  if io16:
    rnd = lambda t: t.half().float()     # noqa: E731
    inputs = (rnd(inputs[0]), rnd(inputs[1]), {k: rnd(v) for k, v in inputs[2].items()})
  r = H.cotangent(name) if direction == "inv" and grads else None
  return H.exact(direction, sd, inputs, c.cfg, r=r)


def _pick(ref, keys):
  return {q: t for q, t in ref.items() if keys(q)}


# (case, quantity) of the training step that the fp16 design itself does not hold to 3 x yardstick: an honest precision
# limit, not a kernel fault.  Each is checked on its own by test_known_precision_limits under xfail(strict=True) -- the bound
# stays 3 x, and the day the quantity meets it the mark fails the suite -- and left out of the other checks of that step.
# hot_f6, WN.3.in_layers.1 v (the direction of a weight-normed conv of flow 3): measured 5.285e-2 relative on the MI355X,
# yardstick 8.867e-3 (6.5e-3, 4.8e-3, 8.9e-3 on the three draws), ratio 5.96; grad_finite true; the next quantities are at
# 2.63 and 2.51.  Why it is a limit: the yardstick is one realisation (round to nearest) of the fp16 roundings; with every
# rounded value moved by up to half an ulp first, the EMULATION itself puts 31 ... 37 of hot_f6's 210 quantities beyond
# 3 x, this tensor at 7.35 x, and none of hot_f1's (test_hot_cpu.py::test_rounding_realisations_spread_with_depth).
KNOWN_LIMITS = {
  ("hot_f6", "p/WN.3.in_layers.1.parametrizations.weight.original1"):
    "fp16-design precision limit at 6 hot flows: measured ratio 5.96 to the yardstick (bound 3); other realisations of the "
    "emulation's own roundings reach 7.35 on this tensor",
}


def _without_known_limits(name, ref):
  return {q: t for q, t in ref.items() if (name, q) not in KNOWN_LIMITS}


def _hold(got, ref, yard, what):
  miss = H.check(got, ref, yard, what)
  assert not miss, f"{what}: beyond 3 x yardstick (ratio to the yardstick, quantity): {miss[:8]}"


def _forward_quantities(y, loss):
  z, log_s, log_det = y
  out = {"z": z, "loss": loss.detach().reshape(1), "log_det": torch.stack([x.detach().reshape(()) for x in log_det])}
  out.update({f"log_s.{k}": t for k, t in enumerate(log_s)})
  return out


# ------------------------------------------------------------------ inference
@pytest.mark.parametrize("name,normed", [(n, False) for n in H.IDS] + [("hot_f1", True)])
def test_infer_fp32(name, normed):
  c = _case(name, "inv")
  out = gpu_infer(build_model(c.hp, c.sd, normed=normed), c.mel, c.z_init, c.z_early, c.sigma)
  ref = _oracle(name, "inv", normed, grads=False)
  _hold({"audio": out}, ref, c.yard("infer"), f"{name} infer fp32 normed={normed}")


@pytest.mark.parametrize("name", ["hot_f1", "hot_c256"])
def test_infer_fp16_io(name):
  """fp16 I/O: the oracle runs on the fp16-rounded mel and noise, as test_gpu_parity.test_infer_golden_case_fp16_io; the
  fp16 rounding of the output itself (2^-11 relative) is far inside the yardstick (5.9e-3 and more)."""
  c = _case(name, "inv")
  out = gpu_infer(build_model(c.hp, c.sd), c.mel, c.z_init, c.z_early, c.sigma, torch.float16)
  _hold({"audio": out}, _oracle(name, "inv", False, grads=False, io16=True), c.yard("infer"), f"{name} infer fp16 io")


# ------------------------------------------------------------------ forward, training step, input gradients
@pytest.mark.parametrize("name", H.IDS)
def test_forward_no_grad(name):
  """The no-grad forward (dense weights): z, every log_s, every log_det_W (non-zero here) and the loss."""
  c = _case(name, "fwd")
  model = build_model(c.hp, c.sd)
  with torch.no_grad():
    y = model((c.mel.cuda(), c.wav.cuda()))
    loss = WaveGlowLoss(1.0)(y, None)
  torch.cuda.synchronize()
  ref = _pick(_oracle(name, "fwd", False), lambda q: not q.startswith(("p/", "d ")))
  assert len(ref) == 3 + c.hp.n_flows
  _hold(_forward_quantities(y, loss), ref, c.yard("train"), f"{name} forward")


@pytest.mark.parametrize("name", H.IDS)
def test_train_step(name):
  """One training step on the weight-normed model: the forward outputs with saved activations, the loss, and every
  parameter gradient, from a NaN-poisoned gradient buffer, with grad_finite at the automatic loss scale.

  Measured on the MI355X: every ratio to the yardstick at most 1.01 on hot_f1, hot_f2e and hot_c256 and at most 2.63 on
  hot_f6, whose one quantity beyond 3 x is checked by test_known_precision_limits (KNOWN_LIMITS above)."""
  c = _case(name, "fwd")
  loss, y, grads = _gpu_step(c.hp, c.sdn, c.mel, c.wav)
  got = _forward_quantities([y[0].detach(), [t.detach() for t in y[1]], y[2]], torch.tensor(loss, dtype=torch.float64))
  got.update({f"p/{n}": g for n, g in grads.items()})
  ref = _pick(_oracle(name, "fwd", True), lambda q: not q.startswith("d "))
  assert {q for q in ref if q.startswith("p/")} == {f"p/{n}" for n in grads}
  assert all(torch.isfinite(g).all() for g in grads.values())          # the quantities of KNOWN_LIMITS included
  _hold(got, _without_known_limits(name, ref), c.yard("train"), f"{name} train step")


@pytest.mark.parametrize("name,quantity", [pytest.param(n, q, marks=pytest.mark.xfail(strict=True, reason=why))
                                           for (n, q), why in KNOWN_LIMITS.items()])
def test_known_precision_limits(name, quantity):
  """The quantities of KNOWN_LIMITS, each alone against the same 3 x yardstick (test_train_step asserts they are finite)."""
  c = _case(name, "fwd")
  _, _, grads = _gpu_step(c.hp, c.sdn, c.mel, c.wav)
  _hold({quantity: grads[quantity[2:]]}, {quantity: _oracle(name, "fwd", True)[quantity]}, c.yard("train"),
        f"{name} known limit")


@pytest.mark.parametrize("name", H.IDS)
def test_input_grads(name):
  """mel.grad and audio.grad, trainable and frozen (bit-identical, as at cold weights)."""
  c = _case(name, "fwd")
  _, g_mel, g_audio, pg = _ig_step(_ig_model(c.hp, c.sdn), c.mel, c.wav)
  ref = _pick(_oracle(name, "fwd", True), lambda q: q.startswith("d "))
  _hold({"d mel": g_mel, "d audio": g_audio}, ref, c.yard("train"), f"{name} input gradients")
  _, f_mel, f_audio, fpg = _ig_step(_ig_model(c.hp, c.sdn, frozen=True), c.mel, c.wav)
  assert torch.equal(f_mel, g_mel) and torch.equal(f_audio, g_audio)
  assert all(g is None for g in fpg.values()) and all(g is not None for g in pg.values())


# ------------------------------------------------------------------ gradients through synthesis
def _synth_got(audio, g_mel, g_zi, g_ze):
  got = {"audio": audio, "d mel": g_mel, "d z_init": g_zi}
  got.update({f"d z_early.{i}": g for i, g in enumerate(g_ze)})
  return got


@pytest.mark.parametrize("name", H.IDS)
def test_infer_differentiable_frozen(name):
  c = _case(name, "inv")
  model = IG._frozen(c.hp, c.sd)
  mel, zi, ze = IG._inputs(c)
  audio = model.infer_differentiable(mel, c.sigma, z_init=zi, z_early=ze)
  (audio * H.cotangent(name).cuda()).sum().backward()
  torch.cuda.synchronize()
  assert bool(model.grad_finite), "a gradient plane overflowed at the automatic loss scale"
  ref = _pick(_oracle(name, "inv", False), lambda q: not q.startswith("p/"))
  assert len(ref) == 3 + len(ze)
  _hold(_synth_got(audio.detach(), mel.grad, zi.grad, [z.grad for z in ze]), ref, c.yard("synth"),
        f"{name} infer_differentiable frozen")
  assert all(p.grad is None for p in model.parameters())


@pytest.mark.parametrize("name", H.IDS)
def test_infer_differentiable_weight_grads(name):
  """weight_grads=True on the weight-normed model: the audio, every parameter gradient and the input gradients."""
  c = _case(name, "inv")
  audio, grads, g_mel, g_zi, g_ze, model = WGT._run(c, True, H.cotangent(name))
  got = _synth_got(audio, g_mel, g_zi, g_ze)
  got.update({f"p/{n}": g for n, g in grads.items()})
  ref = _oracle(name, "inv", True)
  assert {q for q in ref if q.startswith("p/")} == {f"p/{n}" for n in grads}
  _hold(got, ref, c.yard("synth"), f"{name} infer_differentiable weight_grads")


# ------------------------------------------------------------------ equalities that need no tolerance
@pytest.mark.parametrize("name", H.IDS)
def test_recompute_equals_full_save(name):
  """By the rules of test_gpu_recompute.py: everything bit for bit, the gradients behind d spect within its 1e-4."""
  c = _case(name, "fwd")
  out_f, g_f = RC._train_step(c.hp, c.sdn, c.mel, c.wav, False)
  out_r, g_r = RC._train_step(c.hp, c.sdn, c.mel, c.wav, True)
  RC._check_modes(out_r, g_r, out_f, g_f, name)
  ci = _case(name, "inv")
  res = {rc: RC._synthesis(ci.hp, ci.sdn, ci.mel, rc) for rc in (False, True)}
  assert all(torch.isfinite(t).all() for t in res[False][:3])
  RC._check_synthesis(res[True], res[False], name)


@pytest.mark.parametrize("name", EVEN_BATCH)
def test_streams_only_reorder(name, monkeypatch):
  """Two half-batch chains and the weight-gradient stream against everything on one stream, bit for bit, as
  test_gpu_train.test_train_step_half_batch_chains asserts at cold weights."""
  c = _case(name, "fwd")
  monkeypatch.setenv("WG_TRAIN_HALVES", "2")
  monkeypatch.setenv("WG_TRAIN_BWD_HALVES", "2")
  monkeypatch.setenv("WG_TRAIN_SERIAL", "1")
  loss_s, y_s, g_s = _gpu_step(c.hp, c.sdn, c.mel, c.wav)
  monkeypatch.setenv("WG_TRAIN_SERIAL", "0")
  for halves in ("2", "1"):
    monkeypatch.setenv("WG_TRAIN_BWD_HALVES", halves)
    loss_c, y_c, g_c = _gpu_step(c.hp, c.sdn, c.mel, c.wav)
    assert loss_c == loss_s
    assert torch.equal(y_c[0].detach().cpu(), y_s[0].detach().cpu())
    for pname in g_s:
      assert torch.equal(g_c[pname], g_s[pname]), f"{pname}: chains differ from the serial run (bwd halves {halves})"
  assert all(torch.isfinite(g).all() for g in g_c.values())


@pytest.mark.parametrize("bn", ["128", "64"])
def test_c256_both_tile_widths(bn, monkeypatch):
  """hot_c256 (8 waves, the pipelined epilogue) under WG_FORCE_BN = 128 and 64: inference and the training step, both
  against the oracle."""
  monkeypatch.setenv("WG_FORCE_BN", bn)
  c = _case("hot_c256", "inv")
  out = gpu_infer(build_model(c.hp, c.sd), c.mel, c.z_init, c.z_early, c.sigma)
  _hold({"audio": out}, _oracle("hot_c256", "inv", False, grads=False), c.yard("infer"), f"hot_c256 bn{bn} infer")
  c = _case("hot_c256", "fwd")
  loss, y, grads = _gpu_step(c.hp, c.sdn, c.mel, c.wav)
  got = _forward_quantities([y[0].detach(), [t.detach() for t in y[1]], y[2]], torch.tensor(loss, dtype=torch.float64))
  got.update({f"p/{n}": g for n, g in grads.items()})
  _hold(got, _pick(_oracle("hot_c256", "fwd", True), lambda q: not q.startswith("d ")), c.yard("train"),
        f"hot_c256 bn{bn} train step")
