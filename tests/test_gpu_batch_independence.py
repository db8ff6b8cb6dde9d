"""GPU: the gradient paths do not depend on the batch an utterance is in (tests/_batch_independence.py).

The training forward (MODE 1 with saved planes), the dgrad launches (MODE 2 / 3 / 4), ``wgrad_kernel`` and its slabs, the
``d spect`` GEMM, the upsample backward, the two half-batch chains, the recompute slots and the shared backward chain of
``infer_differentiable`` are otherwise compared with the oracle at ``GRAD_TOL`` or with another configuration of the SAME
batch: a leak between neighbouring utterances below 5e-3 of a tensor's norm is identical in both legs of those.  Here one
model runs the batch and then every utterance alone, with the same explicit power-of-two loss scale, and

* row b of z, every log_s_k and the audio, and of mel.grad, audio.grad, z_init.grad and every z_early[i].grad, must be the
  single call's bit for bit (compared on the device);
* every parameter gradient must be the fp64 sum of the single calls' within ``FACTOR`` x the float32 oracle's own reorder
  ratio (``F32_RATIO``) plus the suite's floor; log_det_W_k to 2^-22 relative.
"""
import pytest
import torch

import _batch_independence as BI
from waveglow_amd.model import WaveGlow

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
HALVES = {"WG_TRAIN_HALVES": "2", "WG_TRAIN_BWD_HALVES": "2"}      # test_gpu_train.py: test_train_step_half_batch_chains
SLABS = {"WG_TRAIN_SLABS": "3,5"}                                  # ... test_train_step_every_slab_shape
# id: (case, environment, recompute_activations)
MODES = {
  "c64_l8": ("c64_l8", {}, False),
  "c64_l10": ("c64_l10", {}, False),
  "c256_l8-bn128": ("c256_l8", {"WG_FORCE_BN": "128"}, False),
  "c256_l8-bn64": ("c256_l8", {"WG_FORCE_BN": "64"}, False),
  "c64_l8-recompute": ("c64_l8", {}, True),
  "c64_l8-halves": ("c64_l8", HALVES, False),
  "c64_l8-slabs": ("c64_l8", SLABS, False),
  "c2": ("c2", {}, False),
}
# the slab count only reaches the weight-gradient launches: no frozen leg
TRAIN = [(m, False) for m in MODES] + [(m, True) for m in MODES if m != "c64_l8-slabs"]
SYNTH = [(m, wg) for m in ("c64_l8", "c64_l10", "c256_l8-bn128", "c256_l8-bn64") for wg in (False, True)] + \
        [("c64_l8-recompute", True), ("c64_l8-halves", True)]


@pytest.fixture(autouse=True)
def _poisoned_gradient_buffers(monkeypatch):
  """Gradient buffers start from NaN: an entry the library never writes makes grad_finite false."""
  monkeypatch.setenv("WG_TRAIN_POISON_GRADS", "1")


def _model(mode, frozen, monkeypatch):
  """A fresh model inside the mode's environment (the tile width is read when the engine is created)."""
  name, env, recompute = MODES[mode]
  for k, v in env.items():
    monkeypatch.setenv(k, v)
  c = BI.case(name)
  model = WaveGlow(c.hp)
  model.load_state_dict(c.sd)
  model = model.to(DEV).train()
  model.recompute_activations = recompute
  if frozen:
    model.requires_grad_(False)
  return c, model


def _finish(model, out, what):
  torch.cuda.synchronize()
  assert bool(model.grad_finite), f"{what}: non-finite gradients, or an entry of a (NaN-poisoned) gradient buffer left unwritten"
  for n, p in model.named_parameters():
    if p.requires_grad:
      assert p.grad is not None, (what, n)
      out["p/" + n] = p.grad.detach().clone()
  return out


def _train_call(model, c, b):
  rows = c.rows(b)
  model.zero_grad(set_to_none=True)
  model.grad_scale = c.scale_fwd
  m, a = c.mel[rows].to(DEV).requires_grad_(True), c.wav[rows].to(DEV).requires_grad_(True)
  z, log_s, log_det = model((m, a))
  BI.train_loss(c, rows, z, log_s, log_det).backward()
  out = {"z": z.detach(), "log_det": torch.stack([x.detach().reshape(()) for x in log_det]), "d mel": m.grad, "d audio": a.grad}
  out.update({f"log_s.{k}": t.detach() for k, t in enumerate(log_s)})
  return _finish(model, out, f"{c.name} b={b}")


def _synth_call(model, c, b, weight_grads):
  rows = c.rows(b)
  model.zero_grad(set_to_none=True)
  model.grad_scale = c.scale_inv
  m, zi = c.mel[rows].to(DEV).requires_grad_(True), c.z_init[rows].to(DEV).requires_grad_(True)
  ze = [z.to(DEV).requires_grad_(True) for z in c.z_early_list(rows)]
  audio = model.infer_differentiable(m, BI.SIGMA, z_init=zi, z_early=ze, weight_grads=weight_grads)
  assert audio.grad_fn is not None
  (audio * c.r_audio[rows].to(DEV)).sum().backward()
  out = {"audio": audio.detach(), "d mel": m.grad, "d z_init": zi.grad}
  out.update({f"d z_early.{i}": z.grad for i, z in enumerate(ze)})
  return _finish(model, out, f"{c.name} b={b}")


@pytest.mark.parametrize("mode,frozen", TRAIN, ids=[f"{m}-{'frozen' if f else 'trainable'}" for m, f in TRAIN])
def test_training_direction(mode, frozen, monkeypatch):
  """``model((mel, audio))`` under autograd with the linear loss of ``train_loss``: trainable weight-normed parameters
  (mel and audio want their gradients too), and the frozen model as a likelihood loss."""
  c, model = _model(mode, frozen, monkeypatch)
  batch = _train_call(model, c, None)
  assert batch["z"].shape == (c.B, c.hp.n_group, c.L) and batch["d audio"].shape == (c.B, c.S)
  singles = [_train_call(model, c, b) for b in range(c.B)]
  BI.compare(batch, singles, c, "fwd", f"{mode} training {'frozen' if frozen else 'trainable'}")


@pytest.mark.parametrize("mode,weight_grads", SYNTH, ids=[f"{m}-{'weight_grads' if w else 'frozen'}" for m, w in SYNTH])
def test_synthesis_direction(mode, weight_grads, monkeypatch):
  """``infer_differentiable`` with the loss (audio r).sum(): the frozen vocoder, and ``weight_grads=True``."""
  c, model = _model(mode, not weight_grads, monkeypatch)
  batch = _synth_call(model, c, None, weight_grads)
  assert batch["audio"].shape == (c.B, 256 * c.T)
  singles = [_synth_call(model, c, b, weight_grads) for b in range(c.B)]
  BI.compare(batch, singles, c, "inv", f"{mode} synthesis {'weight_grads' if weight_grads else 'frozen'}")
