"""STOI / ESTOI with a gradient on the device (``wg_stoi_forward``, ``wg_stoi_backward``, ``metrics.stoi_differentiable``,
``waveglow_amd.STOILoss``) against CPU autograd through the torch restatement tests/_stoi_loss_oracle.py, computed once per
case and shared (tests/_stoi_loss_cases.py).

Values: bit for bit the rows of ``stoi_enqueue`` / ``intelligibility_metrics_enqueue``, and within the project's 1e-10 of the
oracle.  Gradient at 10 kHz (fp64): ``|g - g_oracle| <= 100 Y max|g_oracle|`` with Y the distance of the oracle's own two DFT
forms (tests/_stoi_loss_cases.py).  End to end (fp32 ``audio.grad``): one fp32 rounding on top, ``2^-24 |g_oracle|``, with
the fp64 term carried through the transposed filter by its largest row sum.  Measured on MI355X: see the comment on Y."""
import numpy as np
import pytest
import torch

import _stoi_loss_cases as cases
import _stoi_loss_oracle as lo
from _cases import Case
from waveglow_amd import STOILoss, _lib, metrics, resample, synthetic
from waveglow_amd.model import WaveGlow

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
VALUE_BAR = 1e-10                                # tests/test_gpu_stoi.py: the project's bar of the two values
G = cases.WEIGHTS


def _batch(signals, fill=np.nan, pitch=None):
  """fp32 [B, pitch] on the device, row b holding signals[b] and `fill` behind it."""
  out = np.full((len(signals), pitch or max(len(s) for s in signals)), fill, np.float32)
  for b, s in enumerate(signals):
    out[b, :len(s)] = s
  return torch.from_numpy(out).to(DEV)


def _g_rows(B):
  return torch.tensor([G] * B, dtype=torch.float64, device=DEV)


def _device_gradient(xs, ys, pitch=None):
  """(rows [B, 8], d_y fp64 [B, pitch]) of wg_stoi_forward + wg_stoi_backward with the upstream gradients G."""
  lens = [len(x) for x in xs]
  rows, state = metrics.stoi_forward_saved(_batch(xs, pitch=pitch), lens, _batch(ys, pitch=pitch), lens)
  d_y = metrics.stoi_backward_enqueue(state, _g_rows(len(xs)))
  again = metrics.stoi_backward_enqueue(state, _g_rows(len(xs)))
  assert torch.equal(d_y, again), "a second backward on the same saved state must give the same bits"
  return rows.cpu().numpy(), d_y.cpu().numpy()


@pytest.mark.parametrize("name", cases.NAMES)
def test_values_and_gradient_at_10k_equal_the_oracle(name):
  x, y = cases.pair(name)
  g_ref, d_ref, e_ref, info = cases.reference(name)
  assert info["margin"] >= cases.MIN_MARGIN
  rows, d_y = _device_gradient([x], [y])
  plain = metrics.stoi_enqueue(_batch([x]), [len(x)], _batch([y]), [len(y)]).cpu().numpy()
  assert rows.tobytes() == plain.tobytes(), "wg_stoi_forward must give the bits of wg_stoi"
  assert (rows[0, 2], rows[0, 3], rows[0, 4]) == (info["frames"], info["frames_kept"], info["segments"])
  print(f"{name}: device {rows[0, :2].tolist()} oracle {(d_ref, e_ref)}")
  assert abs(rows[0, 0] - d_ref) <= VALUE_BAR and abs(rows[0, 1] - e_ref) <= VALUE_BAR
  assert d_y.dtype == np.float64 and d_y.shape == (1, len(y)) and not np.isnan(d_y).any()
  top = float(np.max(np.abs(g_ref)))
  dist = float(np.max(np.abs(d_y[0] - g_ref)))
  print(f"{name}: max |g| {top:.3e}, max |g_device - g_oracle| {dist:.3e} = {dist / top if top else 0.0:.3e} max |g|, "
        f"bar {cases.bar(g_ref):.3e}")
  assert dist <= cases.bar(g_ref)
  if name == "silent":
    assert rows[0, 0] == 0.0 and rows[0, 1] == 0.0 and not d_y.any()
  else:
    assert top > 0 and d_y.any()
  if name == "gated":                            # gated frames hold no gradient: frame 0's first hop, the silent stretch
    assert not d_y[0, :128].any() and not d_y[0, 21 * 128:24 * 128 + 128].any() and not d_y[0, 50 * 128:].any()
  # the autograd wrapper: the same values with a graph, the gradient rounded to fp32 once
  yt = _batch([y]).requires_grad_(True)
  s = metrics.stoi_differentiable(_batch([x]), None, yt, None)
  assert s.dtype == torch.float64 and tuple(s.shape) == (1, 2) and s.grad_fn is not None
  assert s.detach().cpu().numpy().tobytes() == rows[:, :2].tobytes()
  (G[0] * s[0, 0] + G[1] * s[0, 1]).backward()
  assert yt.grad.cpu().numpy().tobytes() == d_y.astype(np.float32).tobytes()


def test_ragged_batch_rows_are_their_own_calls():
  """B = 3, different lengths, one utterance without a segment, NaN behind the lengths in both tensors."""
  names = ("j5", "short", "gated")
  xs, ys = [cases.pair(n)[0] for n in names], [cases.pair(n)[1] for n in names]
  rows, d_y = _device_gradient(xs, ys, pitch=7000)
  assert not np.isnan(d_y).any()
  assert np.isnan(rows[1, 0]) and np.isnan(rows[1, 1]) and rows[1, 4] == 0 and not d_y[1].any()
  for b, n in enumerate(names):
    own_rows, own = _device_gradient([xs[b]], [ys[b]])
    assert own_rows.tobytes() == rows[b:b + 1].tobytes(), n
    assert own.tobytes() == d_y[b, :len(xs[b])].tobytes(), f"{n}: a row of the batch is not its own call's bits"
    assert not d_y[b, len(xs[b]):].any(), n
    assert float(np.max(np.abs(d_y[b, :len(xs[b])] - cases.reference(n)[0]))) <= cases.bar(cases.reference(n)[0])
  # lengths of the two sides differ: the common length rules, nothing behind it gets a gradient
  lx, ly = [len(x) for x in xs], [len(xs[0]) - 300, len(xs[1]), len(xs[2])]
  r2, state = metrics.stoi_forward_saved(_batch(xs, pitch=7000), lx, _batch(ys, pitch=7000), ly)
  d2 = metrics.stoi_backward_enqueue(state, _g_rows(3)).cpu().numpy()
  assert r2.cpu().numpy()[0, 4] > 0 and not np.isnan(d2).any() and not d2[0, ly[0]:].any() and d2[0, :ly[0]].any()


@pytest.fixture(scope="module")
def through_the_resampler():
  """The 22 050 Hz batch: (audio leaf, target, lengths, crit, scores with a graph)."""
  x, y = (a.copy() for a in cases.pair_22k())
  lens = list(cases.LENGTHS_22K)
  for b, n in enumerate(lens):
    x[b, n:] = np.nan
    y[b, n:] = np.nan
  crit = STOILoss(sampling_rate=cases.SR, factor_stoi=G[0], factor_estoi=G[1], device=DEV)
  target = torch.from_numpy(x).to(DEV)
  audio = torch.from_numpy(y).to(DEV).requires_grad_(True)
  return audio, target, lens, crit, crit.scores(audio, target, lens)


def test_audio_grad_end_to_end_equals_the_oracle(through_the_resampler):
  audio, target, lens, crit, s = through_the_resampler
  assert s.dtype == torch.float64 and tuple(s.shape) == (3, 2) and s.grad_fn is not None
  ref_rows = metrics.intelligibility_metrics_enqueue(target, lens, audio.detach(), lens, cases.SR)
  assert s.detach().cpu().numpy().tobytes() == ref_rows[:, :2].cpu().numpy().tobytes()
  with torch.no_grad():
    quiet = crit.scores(audio, target, lens)
  assert quiet.grad_fn is None and not quiet.requires_grad
  assert quiet.cpu().numpy().tobytes() == s.detach().cpu().numpy().tobytes()
  assert crit.scores(audio.detach(), target, lens).grad_fn is None
  weights = torch.tensor(G, dtype=torch.float64, device=DEV)
  audio.grad = None
  (s[:2] * weights).sum().backward(retain_graph=True)          # row 2 has no segment: its scores are NaN
  first = audio.grad.clone()
  audio.grad = None
  (s[:2] * weights).sum().backward(retain_graph=True)
  assert torch.equal(first, audio.grad), "a second backward under retain_graph must give the same bits"
  g = first.cpu().numpy()
  assert g.dtype == np.float32 and not np.isnan(g).any() and not g[2].any()
  sv = s.detach().cpu().numpy()
  assert np.isnan(sv[2]).all() and not np.isnan(sv[:2]).any()
  # the oracle: the device's own 10 kHz signals (pinned by tests/test_gpu_resample.py), CPU autograd, the numpy transpose
  up, down, half, h = resample.resample_plan(cases.SR, metrics.STOI_RATE)
  gain = max(float(np.abs(h[r::down]).sum()) for r in range(down))              # largest row sum of the transposed table
  x10, n10 = resample.resample(target, lens, cases.SR, metrics.STOI_RATE)
  y10, _ = resample.resample(audio.detach(), lens, cases.SR, metrics.STOI_RATE)
  x10, y10 = x10.cpu().numpy(), y10.cpu().numpy()
  for b in (0, 1):
    g10, d_ref, e_ref, info = lo.gradient(x10[b, :n10[b]], y10[b, :n10[b]], G[0], G[1])
    assert info["margin"] >= cases.MIN_MARGIN and info["segments"] > 0
    assert abs(sv[b, 0] - d_ref) <= VALUE_BAR and abs(sv[b, 1] - e_ref) <= VALUE_BAR
    ref = lo.resample_backward(g10, lens[b], up, down)
    tol = 2.0 ** -24 * np.abs(ref) + gain * cases.bar(g10)
    dist = np.abs(g[b, :lens[b]].astype(np.float64) - ref)
    print(f"row {b}: max |g| {np.max(np.abs(ref)):.3e}, largest distance {np.max(dist):.3e}, "
          f"largest distance / bound {np.max(dist / tol):.3f}")
    assert (dist <= tol).all()
    assert not g[b, lens[b]:].any() and g[b, :lens[b]].any()


def test_loss_reduction(through_the_resampler):
  audio, target, lens, crit, _ = through_the_resampler
  audio.grad = None
  loss = crit(audio, target, lens)
  assert loss.dtype == torch.float32 and loss.dim() == 0 and loss.grad_fn is not None
  loss.backward()
  got = audio.grad.clone()
  audio.grad = None
  s = crit.scores(audio, target, lens)
  want = -(G[0] * s[:2, 0].mean() + G[1] * s[:2, 1].mean()).to(torch.float32)   # the two utterances that have a segment
  want.backward()
  assert torch.equal(loss.detach(), want.detach()) and torch.equal(got, audio.grad)
  assert -1.5 < float(loss.detach()) < 0 and not got[2].any()
  audio.grad = None
  # every utterance unscored: the value is 0 and the gradient zero
  short = [2000, 3000, 0]
  loss = crit(audio, target, short)
  loss.backward()
  assert float(loss.detach()) == 0.0 and not audio.grad.any() and not torch.isnan(audio.grad).any()
  audio.grad = None
  # at 10 kHz the resampler is skipped
  x, y = cases.pair("j5")
  crit10 = STOILoss(sampling_rate=10000, factor_stoi=1.0, factor_estoi=0.0, device=DEV)
  yt = _batch([y]).requires_grad_(True)
  loss = crit10(yt, _batch([x]))
  loss.backward()
  rows, state = metrics.stoi_forward_saved(_batch([x]), None, _batch([y]), None)
  d = metrics.stoi_backward_enqueue(state, torch.tensor([[-1.0, 0.0]], dtype=torch.float64, device=DEV))
  assert float(loss.detach()) == float((-rows[0, 0]).to(torch.float32)) and torch.equal(yt.grad, d.to(torch.float32))
  # refusals on the device
  with pytest.raises(_lib.WgError):
    crit(audio, target.clone().requires_grad_(True), lens)
  with pytest.raises(_lib.WgError):
    crit(audio, target[:, :-1], lens)
  with pytest.raises(_lib.WgError):
    crit(audio, target, [cases.N_22K + 1, 0, 0])
  with pytest.raises(_lib.WgError):
    metrics.stoi_differentiable(_batch([x]).requires_grad_(True), None, yt, None)


def test_one_step_through_the_vocoder():
  """``infer_differentiable(mel, 0.6, weight_grads=True)`` -> STOILoss -> ``backward()``: every parameter has a finite
  gradient and ``grad_finite`` holds.  The model is the 64-channel golden case: the weight-gradient path takes the
  training direction's widths only and refuses the 16-channel "tiny" model (tests/test_gpu_infer_weight_grads.py:
  test_refusals), so 64 channels is the smallest model this step can run on.  40 mel frames are 10 240 samples, 35 frames
  at 10 kHz: the loss has segments to score."""
  c = Case("c64")
  model = WaveGlow(c.hp)
  model.load_state_dict(synthetic.to_weightnorm_form(c.sd))
  model = model.to(DEV).train().requires_grad_(True)
  mel = synthetic.make_mel(1, 40, seed=5).to(DEV)
  audio = model.infer_differentiable(mel, 0.6, weight_grads=True)
  assert audio.requires_grad and audio.dim() == 2 and audio.shape[0] == 1 and audio.shape[1] >= 9400
  target = 0.1 * torch.randn(audio.shape, generator=torch.Generator().manual_seed(3)).to(DEV)
  crit = STOILoss(sampling_rate=22050, factor_stoi=1.0, factor_estoi=1.0, device=DEV)
  assert not bool(crit.scores(audio.detach(), target).isnan().any()), "the utterance must have a segment"
  loss = crit(audio, target)
  loss.backward()
  torch.cuda.synchronize()
  assert bool(torch.isfinite(loss)) and bool(model.grad_finite)
  some = 0
  for n, p in model.named_parameters():
    assert p.grad is not None and bool(torch.isfinite(p.grad).all()), n
    some += int(bool(p.grad.any()))
  assert some > 0, "the loss reached no parameter"
