"""GPU: ``WaveGlow.infer_differentiable(..., frames=)`` -- synthesis under autograd on a padded batch of utterances of
different lengths (tests/_ragged_infer_grads.py).

Every utterance must get what a batch-of-one call on its crop gets: audio and input gradients bit for bit in front of its
count and exact zeros behind it, parameter gradients that are the sum of the single calls'.  Everything behind a count is
NaN in the mel, the noise and the incoming audio gradient of every ragged call here, and the gradient buffers start from
NaN (``WG_TRAIN_POISON_GRADS``): one padding value that is read, or one entry that is not written, shows.
"""
import pytest
import torch

import _batch_independence as BI
import _ragged_infer_grads as R
from _cases import GRAD_TOL
from waveglow_amd._lib import WgError
from waveglow_amd.model import WaveGlow
from waveglow_amd.stft_loss import MultiResolutionSTFTLoss
from waveglow_amd.taco_stft import TacotronSTFT, TSTFTHParams

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
DSPECT_TOL = 3e-5        # gradients behind d spect, recompute against full save (fp32 partial sums)
UPSAMPLE = ("upsample.weight", "upsample.bias")
# id: (case, environment).  c256_l8 under both forward tile widths, the narrow one with the half-batch chains and pinned
# slab counts of tests/test_gpu_batch_independence.py on top
MODES = {
  "c64_l8": ("c64_l8", {}),
  "c64_l10": ("c64_l10", {}),
  "c256_l8-bn128": ("c256_l8", {"WG_FORCE_BN": "128"}),
  "c256_l8-bn64": ("c256_l8", {"WG_FORCE_BN": "64", "WG_TRAIN_HALVES": "2", "WG_TRAIN_SLABS": "3,5"}),
}


@pytest.fixture(autouse=True)
def _poisoned_gradient_buffers(monkeypatch):
  """Gradient buffers start from NaN: an entry the library never writes makes grad_finite false."""
  monkeypatch.setenv("WG_TRAIN_POISON_GRADS", "1")


def _model(mode, monkeypatch, weight_grads, dense=False, recompute=False):
  """A fresh model (and engine, and workspaces) inside the mode's environment."""
  name, env = MODES[mode]
  for k, v in env.items():
    monkeypatch.setenv(k, v)
  rc = R.case(name)
  model = WaveGlow(rc.hp)
  if dense:
    model = WaveGlow.remove_weightnorm(model)
    model.load_state_dict(rc.dense_sd())
  else:
    model.load_state_dict(rc.sd)
  model = model.to(DEV).train().requires_grad_(bool(weight_grads))
  model.recompute_activations = recompute
  return rc, model


def _call(model, rc, tensors, weight_grads, frames=None, what=""):
  """One call and its backward with the cotangent ``tensors[3]``: audio, d mel, d z_init, d z_early.i, p/<parameter>."""
  mel, zi, ze, r = tensors
  model.zero_grad(set_to_none=True)
  model.grad_scale = rc.scale
  m, zi = mel.to(DEV).requires_grad_(True), zi.to(DEV).requires_grad_(True)
  ze = [z.to(DEV).requires_grad_(True) for z in ze]
  kw = {} if frames is None else {"frames": frames}
  audio = model.infer_differentiable(m, R.SIGMA, z_init=zi, z_early=ze, weight_grads=weight_grads, **kw)
  assert audio.grad_fn is not None and audio.shape == (mel.shape[0], 256 * mel.shape[2])
  audio.backward(r.to(DEV))
  torch.cuda.synchronize()
  assert bool(model.grad_finite), f"{what}: non-finite gradients, or an entry of a (NaN-poisoned) gradient buffer left unwritten"
  out = {"audio": audio.detach(), "d mel": m.grad, "d z_init": zi.grad}
  out.update({f"d z_early.{i}": z.grad for i, z in enumerate(ze)})
  for n, p in model.named_parameters():
    if p.requires_grad:
      assert p.grad is not None, (what, n)
      out["p/" + n] = p.grad.detach().clone()
    else:
      assert p.grad is None, (what, n)
  return out


def _ragged(model, rc, weight_grads, frames=None, what=""):
  frames = rc.frames if frames is None else frames
  return _call(model, rc, rc.padded(R.NAN, frames), weight_grads, list(frames), what)


def _single(model, rc, b, weight_grads, what=""):
  mel, zi, ze, r = rc.crop(b)
  return _call(model, rc, (mel, zi, [ze[k] for k in rc.keys], r), weight_grads, None, f"{what} b={b}")


def _same_bits(x, y, what):
  assert set(x) == set(y), what
  for q in x:
    assert torch.equal(x[q], y[q]), f"{what}: {q} differs: {int((x[q] != y[q]).sum())} of {x[q].numel()} entries"


def _additive(rc, batch, singles, what):
  rel = R.bound(rc.name)
  assert 0.0 < rel <= R.BOUND_LIMIT
  misses, worst = BI.check_additive(batch, singles, rel, what, rc.hp)
  print(f"{what}: worst additive ratio {worst:.3e}, bound {rel:.3e} (+ {R.FLOOR:g})")
  assert not misses, f"{what}: parameter gradients of the ragged call are not the sum of the single calls': {misses[:8]}"


SYNTH = [(m, wg) for m in MODES for wg in (False, True)]


@pytest.mark.parametrize("mode,weight_grads", SYNTH, ids=[f"{m}-{'weight_grads' if w else 'frozen'}" for m, w in SYNTH])
def test_every_utterance_gets_its_batch_of_one_call(mode, weight_grads, monkeypatch):
  """Rows bit for bit and zeros behind the counts; with ``weight_grads`` the parameter gradients (weight-norm form) against
  the fp64 host sum of the GPU single calls (additivity) and against the fp64 oracle's sum over the crops (``GRAD_TOL``)."""
  rc, model = _model(mode, monkeypatch, weight_grads)
  what = f"{mode} {'weight_grads' if weight_grads else 'frozen'}"
  batch = _ragged(model, rc, weight_grads, what=what)
  singles = [_single(model, rc, b, weight_grads, what) for b in range(rc.B)]
  R.rows_bit_for_bit(rc, batch, singles, what)
  for b, f in enumerate(rc.frames):
    assert float(batch["d mel"][b, :, :f].abs().max()) > 0.0 and float(batch["audio"][b, :256 * f].abs().max()) > 0.0
  if weight_grads:
    _additive(rc, batch, singles, what)
    grads = {q: g for q, g in batch.items() if q.startswith("p/")}
    misses = R.check_parity(grads, rc.name, False, GRAD_TOL, what)
    assert not misses, f"{what}: parameter gradients against the fp64 oracle's sum over the crops: {misses[:8]}"


@pytest.mark.parametrize("mode", ["c64_l8", "c64_l10", "c256_l8-bn128"])
def test_parameter_gradients_after_remove_weightnorm(mode, monkeypatch):
  rc, model = _model(mode, monkeypatch, True, dense=True)
  batch = _ragged(model, rc, True, what=mode)
  grads = {q: g for q, g in batch.items() if q.startswith("p/")}
  misses = R.check_parity(grads, rc.name, True, GRAD_TOL, f"{mode} dense weights")
  assert not misses, f"{mode}: parameter gradients against the fp64 oracle's sum over the crops: {misses[:8]}"
  # the values and the input gradients do not know the form of the weights' parametrisation beyond fp32 rounding of g v / ||v||
  assert bool(torch.isfinite(batch["audio"]).all())
  for b, f in enumerate(rc.frames):
    assert not batch["audio"][b, 256 * f:].any() and not batch["d mel"][b, :, f:].any()


def test_frozen_parameters_get_no_gradient(monkeypatch):
  rc, model = _model("c64_l8", monkeypatch, True)
  every = _ragged(model, rc, True)
  frozen = [n for n, _ in model.named_parameters() if n.startswith("WN.0.") or n.startswith("upsample.")]
  assert frozen
  for n, p in model.named_parameters():
    p.requires_grad_(n not in frozen)
  some = _ragged(model, rc, True)          # _call asserts: no .grad where requires_grad is False
  assert not any("p/" + n in some for n in frozen)
  _same_bits(some, {q: t for q, t in every.items() if q[2:] not in frozen}, "a subset of trainable parameters")


@pytest.mark.parametrize("mode,weight_grads", [("c64_l8", True), ("c64_l10", False), ("c256_l8-bn128", True)])
def test_full_counts_are_the_dense_call(mode, weight_grads, monkeypatch):
  """``frames=[T] * B`` (list, CPU tensor, device tensor) and the call without ``frames``: the same bits, values and
  gradients."""
  rc, model = _model(mode, monkeypatch, weight_grads)
  c = rc.c
  tensors = (c.mel, c.z_init, [c.z_early[k] for k in rc.keys], c.r_audio)
  dense = _call(model, rc, tensors, weight_grads, None, mode)
  full = [rc.T] * rc.B
  for frames in (full, torch.tensor(full), torch.tensor(full, dtype=torch.int32, device=DEV)):
    _same_bits(_call(model, rc, tensors, weight_grads, frames, mode), dense, f"{mode} frames=[T]*B as {type(frames).__name__}")


def test_device_counts_are_trusted(monkeypatch):
  """An int32 device tensor is never read on the host.  Counts outside [1, T] -- 0 and 99 -- make their utterances all
  padding: zero audio, zero input gradients, nothing added to the parameter gradients; the other rows keep their bits."""
  rc, model = _model("c64_l8", monkeypatch, True)
  given, eff = [13, 0, 99, 9], [13, 0, 0, 9]
  assert [rc.frames[0], rc.frames[3]] == [13, 9]
  frames = torch.tensor(given, dtype=torch.int32, device=DEV)
  batch = _call(model, rc, rc.padded(R.NAN, eff), True, frames, "device counts")
  assert torch.equal(frames.cpu(), torch.tensor(given, dtype=torch.int32))          # the caller's tensor is left alone
  singles = [_single(model, rc, 0, True), None, None, _single(model, rc, 3, True)]
  R.rows_bit_for_bit(rc, batch, singles, "device counts", eff)
  for q in BI.row_quantities(batch):
    assert not batch[q][1:3].any(), q
  _additive(rc, batch, [singles[0], singles[3]], "device counts")
  for bad in (torch.tensor(given, device=DEV), torch.tensor(given[:3], dtype=torch.int32, device=DEV),
              torch.tensor(given, dtype=torch.float32, device=DEV)):
    with pytest.raises(WgError, match="int32"):
      model.infer_differentiable(rc.c.mel.to(DEV), R.SIGMA, frames=bad)


@pytest.mark.parametrize("mode", ["c64_l8", "c256_l8-bn128"])
def test_stale_workspace(mode, monkeypatch):
  """The workspace of a (B, T) is handed back with whatever the last call left in it.  A dense call with LOUD inputs, and a
  ragged call with other counts, in between: the ragged call gives the bits of its first run, parameter gradients too."""
  rc, model = _model(mode, monkeypatch, True)
  first = _ragged(model, rc, True, what="first run")
  c = rc.c
  loud = (c.mel, BI.LOUD * c.z_init, [BI.LOUD * c.z_early[k] for k in rc.keys], BI.LOUD * c.r_audio)
  _call(model, rc, loud, True, None, "dense LOUD call")
  _same_bits(_ragged(model, rc, True, what="after a dense call"), first, f"{mode}: after a dense call on the same workspace")
  other = _ragged(model, rc, True, R.FRAMES_2[rc.name], "other counts")
  for b, f in enumerate(R.FRAMES_2[rc.name]):
    assert not other["audio"][b, 256 * f:].any() and not other["d mel"][b, :, f:].any()
  _same_bits(_ragged(model, rc, True, what="after other counts"), first, f"{mode}: after a ragged call with other counts")


@pytest.mark.parametrize("mode,weight_grads", [("c64_l8", True), ("c256_l8-bn128", True), ("c64_l10", False)])
def test_recompute_equals_full_save(mode, weight_grads, monkeypatch):
  rc, model = _model(mode, monkeypatch, weight_grads)
  full = _ragged(model, rc, weight_grads, what="full save")
  _, model_r = _model(mode, monkeypatch, weight_grads, recompute=True)
  rec = _ragged(model_r, rc, weight_grads, what="recompute")
  assert set(rec) == set(full)
  for q in full:
    if q == "d mel" or q[2:] in UPSAMPLE:      # the documented exception: d spect is summed flow by flow in fp32
      rel = float((rec[q].double() - full[q].double()).norm() / full[q].double().norm())
      print(f"{mode}: {q}: recompute against full save, rel {rel:.3e}")
      assert rel <= DSPECT_TOL, (q, rel)
    else:
      assert torch.equal(rec[q], full[q]), q
  for b, f in enumerate(rc.frames):
    assert not rec["d mel"][b, :, f:].any()


def test_no_grad_route_is_infer_with_noise(monkeypatch):
  rc, model = _model("c64_l8", monkeypatch, False)
  mel, zi, ze, _ = (t.to(DEV) if torch.is_tensor(t) else [z.to(DEV) for z in t] for t in rc.padded())
  ref = model.infer_with_noise(mel, zi, ze, R.SIGMA, frames=torch.tensor(rc.frames, dtype=torch.int32))
  with torch.no_grad():
    out = model.infer_differentiable(mel.clone().requires_grad_(True), R.SIGMA, z_init=zi, z_early=ze, frames=rc.frames)
  assert out.grad_fn is None and torch.equal(out, ref)
  # grad mode on, nothing requires grad: the same route
  out = model.infer_differentiable(mel, R.SIGMA, z_init=zi, z_early=ze, frames=tuple(rc.frames))
  assert out.grad_fn is None and torch.equal(out, ref)
  assert bool(torch.isfinite(ref).all())
  for b, f in enumerate(rc.frames):
    assert not ref[b, 256 * f:].any() and ref[b, :256 * f].any()


def test_end_to_end_with_the_ragged_losses(monkeypatch):
  """An acoustic model's step on a ragged batch: infer_differentiable(frames=) -> MultiResolutionSTFTLoss(lengths=) plus a
  mel-cycle term through mel_spectrogram_differentiable(lengths=) -> backward().  NaN behind every count, everywhere."""
  rc, model = _model("c64_l8", monkeypatch, False)
  F = [13, 5, 7, 9]                         # the STFT loss reflect-pads by 1024: at least 5 frames per utterance
  lengths = [256 * f for f in F]
  mel, zi, ze, target = rc.padded(R.NAN, F)
  target = (0.1 * rc.scale * target).to(DEV)          # a waveform-sized target, NaN behind the lengths
  m = mel.to(DEV).requires_grad_(True)
  model.grad_scale = 0.0                    # the automatic loss scale: both losses are means
  audio = model.infer_differentiable(m, R.SIGMA, z_init=zi.to(DEV), z_early=[z.to(DEV) for z in ze], frames=F)
  for b, f in enumerate(F):
    assert not audio[b, 256 * f:].any()
  crit = MultiResolutionSTFTLoss(device=DEV)
  taco = TacotronSTFT(TSTFTHParams(), DEV)
  mel_hat = taco.mel_spectrogram_differentiable(audio, lengths)
  cycle = sum(torch.nn.functional.l1_loss(mel_hat[b, :, :f], m.detach()[b, :, :f]) for b, f in enumerate(F)) / len(F)
  loss = crit(audio, target, lengths) + cycle
  assert bool(torch.isfinite(loss))
  loss.backward()
  torch.cuda.synchronize()
  assert bool(model.grad_finite) and bool(torch.isfinite(m.grad).all())
  for b, f in enumerate(F):
    assert not m.grad[b, :, f:].any(), b
    assert bool((m.grad[b, :, :f].abs().amax(0) > 0).all()), b
