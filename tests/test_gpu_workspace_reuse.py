"""GPU: the ``fresh = 0`` contract of the training pool (``_Engine.train_workspace``).

``forward`` under autograd and ``infer_differentiable`` both take their saved-state workspace from one pool, keyed by
(B, n_frames, audio_len) and the wg_train flags.  With ``audio_len == 256 * n_frames`` the keys of the two directions
coincide: a model that alternates them on one batch shape (a cycle-consistency step) hands the slot of one direction to the
other with ``fresh = 0``, so the library clears nothing -- unless the call is ragged -- and every region a kernel reads must
have been written by the call itself, or hold the zeros (guard rows, rows behind an utterance) that both directions leave.

The truth of every step is the same step on a new model and engine (a new slot, ``fresh = 1``): its "alone" bytes, values
and every gradient.  One model then runs the steps in sequence and every step must give its alone bytes.
"""
import gc

import pytest
import torch

import _batch_independence as BI
import _dirty as D
import _hot as H
from test_gpu_dirty_workspace import TRAIN, _env, inputs, synth_step, train_step
from waveglow_amd import synthetic

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
RECOMPUTE = {"full-save": (False, False), "recompute": (True, True), "alternating": (False, True)}


@pytest.fixture(autouse=True)
def _poisoned_gradient_buffers(monkeypatch):
  monkeypatch.setenv("WG_TRAIN_POISON_GRADS", "1")


class Full:
  """A case of tests/_batch_independence.py with the training direction at ``audio_len = 256 T``: the geometry, and so the
  pool key, of ``infer_differentiable``.  Has what ``train_step``, ``synth_step`` and ``BI.train_loss`` read of a case."""

  def __init__(self, name):
    c = BI.case(name)
    B, T = c.B, c.T
    g = torch.Generator().manual_seed(9100 + 10 * B + T)
    amp = torch.full((B,), 1.0 / BI.LOUD)
    amp[BI.LOUD_ROW] = 1.0
    self.name, self.hp, self.B, self.T, self.mel = name, c.hp, B, T, c.mel
    self.S, self.L = 256 * T, 32 * T
    self.wav = (torch.rand(B, self.S, generator=g) * 1.2 - 0.6) * amp[:, None]
    n = B * self.S
    cot = amp * BI.LOUD / n
    self.r_z = torch.randn(B, c.hp.n_group, self.L, generator=g) * cot[:, None, None]
    self.r_ls = [torch.randn(B, ck // 2, self.L, generator=g) * cot[:, None, None] for ck in synthetic.flow_channels(c.hp)]
    self.c_ld = [(0.5 + 0.25 * k) * (-1.0) ** k / n for k in range(c.hp.n_flows)]
    self.scale_fwd = self.scale_inv = H.grad_scale(n)
    assert self.scale_inv == c.scale_inv
    self.z_init, self.z_early_list, self.r_audio = c.z_init, c.z_early_list, c.r_audio


_full = {}


def full(name):
  if name not in _full:
    _full[name] = Full(name)
  return _full[name]


def run(model, c, x, kind, recompute):
  """One step of ``kind`` on ``model``: A (training step), LOUD (A with inputs and cotangents times ``BI.LOUD``), D (dense
  ``infer_differentiable`` with weight gradients), R (the same on the ragged batch)."""
  model.recompute_activations = recompute
  if kind == "A":
    out = train_step(model, c, 1.0, kind)
  elif kind == "LOUD":
    out = train_step(model, c, BI.LOUD, kind)
  elif kind == "D":
    out = synth_step(model, c, True, None, 1.0, kind)
  else:
    out = synth_step(model, c, True, x.frames, 1.0, kind)
  torch.cuda.synchronize()
  return D.snapshot(out)


_alone = {}


def alone(mode, kind, recompute):
  """The step on a new model and engine, computed once per (mode, step, save mode) inside the mode's environment."""
  key = (mode, kind, recompute)
  if key not in _alone:
    x = inputs(TRAIN[mode][0])
    _alone[key] = run(x.model(train=True), full(TRAIN[mode][0]), x, kind, recompute)
    for q, t in _alone[key].items():
      assert bool(torch.isfinite(t).all()), (key, q)
  return _alone[key]


SEQUENCE = ("A", "D", "A", "R", "A", "D", "LOUD", "A")


@pytest.mark.parametrize("save", list(RECOMPUTE))
@pytest.mark.parametrize("mode", list(TRAIN))
def test_alternating_directions_on_one_slot(mode, save, monkeypatch):
  name, env = TRAIN[mode]
  _env(monkeypatch, env)
  x, c = inputs(name), full(name)
  model = x.model(train=True)
  flags = RECOMPUTE[save]
  for i, kind in enumerate(SEQUENCE):
    rc = flags[i % 2]
    got = run(model, c, x, kind, rc)
    D.same_outputs(got, alone(mode, kind, rc), f"{mode} {save}: step {i} ({kind}, recompute {rc}) against the step alone")
    pool = model._engine._train_pool
    assert len(pool) == len(set(flags)) if i else len(pool) == 1, (i, len(pool))        # one slot per save mode, no more
    assert not any(e["busy"] for e in pool), i
  assert all(e["key"] == (c.B, c.T, c.S) for e in model._engine._train_pool)


@pytest.mark.parametrize("save", ["full-save", "recompute"])
@pytest.mark.parametrize("mode", list(TRAIN))
def test_two_pending_forwards_and_a_dropped_graph(mode, save, monkeypatch):
  """One forward of each direction pending at once -- the second gets a slot of its own -- with the backwards in reverse
  order; then a forward whose graph is dropped without a backward; a training step behind each."""
  name, env = TRAIN[mode]
  _env(monkeypatch, env)
  x, c = inputs(name), full(name)
  rc = RECOMPUTE[save][0]
  model = x.model(train=True)
  D.same_outputs(run(model, c, x, "A", rc), alone(mode, "A", rc), f"{mode}: first step")
  model.zero_grad(set_to_none=True)
  model.grad_scale = c.scale_fwd
  # the training direction first ...
  m1, a1 = c.mel.to(DEV).requires_grad_(True), c.wav.to(DEV).requires_grad_(True)
  z, log_s, log_det = model((m1, a1))
  from waveglow_amd.model import WaveGlowLoss
  nll = WaveGlowLoss(BI.SIGMA)((z, log_s, log_det))
  loss = BI.train_loss(c, slice(None), z, log_s, log_det) + nll
  # ... synthesis while it is pending, and its backward first
  m2, zi = c.mel.to(DEV).requires_grad_(True), c.z_init.to(DEV).requires_grad_(True)
  ze = [t.to(DEV).requires_grad_(True) for t in c.z_early_list(slice(None))]
  audio = model.infer_differentiable(m2, BI.SIGMA, z_init=zi, z_early=ze, weight_grads=True)
  assert len(model._engine._train_pool) == 2 and all(e["busy"] for e in model._engine._train_pool)
  audio.backward(c.r_audio.to(DEV))
  assert bool(model.grad_finite)
  synth = {"audio": audio.detach(), "d mel": m2.grad, "d z_init": zi.grad}
  synth.update({f"d z_early.{i}": t.grad for i, t in enumerate(ze)})
  synth.update({"p/" + n: p.grad.detach().clone() for n, p in model.named_parameters()})
  D.same_outputs(synth, alone(mode, "D", rc), f"{mode}: synthesis beside a pending training forward")
  model.zero_grad(set_to_none=True)
  loss.backward()
  assert bool(model.grad_finite)
  train = {"z": z.detach(), "WaveGlowLoss": nll.detach(), "d mel": m1.grad, "d audio": a1.grad}
  train.update({f"log_s.{k}": t.detach() for k, t in enumerate(log_s)})
  train.update({"p/" + n: p.grad.detach().clone() for n, p in model.named_parameters()})
  D.same_outputs(train, alone(mode, "A", rc), f"{mode}: the pending training step, its backward last")
  del z, log_s, log_det, nll, loss, audio
  assert not any(e["busy"] for e in model._engine._train_pool)
  D.same_outputs(run(model, c, x, "A", rc), alone(mode, "A", rc), f"{mode}: step behind the two pending forwards")
  D.same_outputs(run(model, c, x, "R", rc), alone(mode, "R", rc), f"{mode}: ragged synthesis behind them")
  # a forward whose graph is dropped without a backward (a loss that is only logged), with LOUD inputs
  dropped = model((c.mel.to(DEV).requires_grad_(True), (BI.LOUD * c.wav).to(DEV)))
  assert any(e["busy"] for e in model._engine._train_pool)
  del dropped
  gc.collect()
  assert not any(e["busy"] for e in model._engine._train_pool)
  D.same_outputs(run(model, c, x, "A", rc), alone(mode, "A", rc), f"{mode}: step behind a dropped forward")
  D.same_outputs(run(model, c, x, "D", rc), alone(mode, "D", rc), f"{mode}: synthesis behind it")
