"""GPU: the soft-DTW kernels (wg_softdtw_forward / wg_softdtw_backward) and the Python layer on them against the oracle of
tests/_softdtw_oracle.py, and the invariants of include/waveglow_amd.h: bit-reproducible, batch-independent, nothing read
behind a count, no output dependent on what its buffers held.

Accuracy bar of a case (tests/_softdtw_cases.py: bar): 100 max(Y, 2^-52 (Ta + Tb) max(1, max|R| / gamma)), Y the disagreement
of the two oracle formulations; relative to max(1, |value|) for the value, absolute for E, relative to max|g| for the
gradients, which add one fp32 rounding 2^-24 |g|.  The reference is formulation (b) in longdouble."""
import ctypes as C
import math

import numpy as np
import pytest
import torch

import _dirty as D
import _softdtw_cases as cases
import _softdtw_oracle as O

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
F32 = 2.0 ** -24


def _dev(x, grad=False):
  return torch.tensor(np.asarray(x)[None], dtype=torch.float32, device=DEV).requires_grad_(grad)


def run(a, b, gamma, cost):
  """One pair through the Python layer with B = 1 and tmax = its counts: value, E, g_a, g_b as numpy."""
  from waveglow_amd import softdtw
  ta, tb = _dev(a, True), _dev(b, True)
  v = softdtw.soft_dtw(ta, None, tb, None, gamma, cost)
  v.sum().backward()
  v2, e = softdtw.soft_dtw_alignment(ta, None, tb, None, gamma, cost)
  D.same_bytes(v.detach(), v2, "value of the alignment call")
  return dict(value=float(v.detach()[0]), E=e[0].cpu().numpy(), g_a=ta.grad[0].cpu().numpy(), g_b=tb.grad[0].cpu().numpy())


def check(got, want, bar, what):
  """``got`` (device; fp32 gradients) against ``want`` (longdouble oracle) within ``bar``; prints each figure first."""
  d = O.distance(got, want)
  g_ok = True
  worst32 = 0.0
  for q in ("g_a", "g_b"):
    ref = np.asarray(want[q], dtype=np.float64)
    err = np.abs(got[q].astype(np.float64) - ref)
    tol = bar * d["gmax"] + F32 * np.abs(ref)
    worst32 = max(worst32, float((err / np.maximum(tol, 1e-300)).max()))
    g_ok = g_ok and bool((err <= tol).all())
  print(f"{what}: value {d['value']:.2e} E {d['E']:.2e} grad/max|g| {d['grad']:.2e} (max|g| {d['gmax']:.3g}; error over its "
        f"tolerance {worst32:.2f}); bar {bar:.2e}")
  assert d["value"] <= bar, (what, d)
  assert d["E"] <= bar, (what, d)
  assert g_ok, (what, d, worst32)


@pytest.mark.parametrize("cost", cases.COSTS)
@pytest.mark.parametrize("index", range(len(cases.CASES)), ids=cases.IDS)
def test_matches_the_oracle(index, cost):
  ref = cases.reference(index, cost)
  got = run(ref["a"], ref["b"], ref["gamma"], cost)
  check(got, ref["ld"], cases.bar(ref), f"{cases.IDS[index]} {cost}")


# three utterances of different counts at a larger pitch (1100 rows: two rows per thread, where their own calls take one)
BATCH = ((16, 70, 45, 0.01), (16, 37, 41, 1.0), (16, 9, 1, 0.5))
PITCH_A, PITCH_B = 1100, 50


def _batch(gamma, counts_a=None, counts_b=None):
  """The padded batch with NaN behind every count, and the device counts."""
  K = BATCH[0][0]
  fa = torch.full((len(BATCH), K, PITCH_A), float("nan"), dtype=torch.float32)
  fb = torch.full((len(BATCH), K, PITCH_B), float("nan"), dtype=torch.float32)
  pairs = []
  for u, case in enumerate(BATCH):
    a, b = cases.inputs(case)
    fa[u, :, :case[1]], fb[u, :, :case[2]] = torch.tensor(a), torch.tensor(b)
    pairs.append((a, b))
  na = torch.tensor(counts_a or [c[1] for c in BATCH], dtype=torch.int32, device=DEV)
  nb = torch.tensor(counts_b or [c[2] for c in BATCH], dtype=torch.int32, device=DEV)
  return fa.to(DEV), na, fb.to(DEV), nb, pairs


def _all_outputs(fa, na, fb, nb, gamma, cost, g=None):
  from waveglow_amd import softdtw
  ta, tb = fa.clone().requires_grad_(True), fb.clone().requires_grad_(True)
  v = softdtw.soft_dtw(ta, na, tb, nb, gamma, cost)
  (v * (g if g is not None else torch.ones_like(v))).nan_to_num(0.0).sum().backward()
  _, e = softdtw.soft_dtw_alignment(fa, na, fb, nb, gamma, cost)
  return dict(value=v.detach(), E=e, g_a=ta.grad, g_b=tb.grad)


@pytest.mark.parametrize("cost", cases.COSTS)
def test_an_utterance_has_the_bits_of_its_own_call(cost):
  from waveglow_amd import softdtw
  gamma = 0.25
  fa, na, fb, nb, pairs = _batch(gamma)
  out = _all_outputs(fa, na, fb, nb, gamma, cost)
  for u, (case, (a, b)) in enumerate(zip(BATCH, pairs)):
    Ta, Tb = case[1], case[2]
    ta, tb = _dev(a, True), _dev(b, True)
    v = softdtw.soft_dtw(ta, [Ta], tb, [Tb], gamma, cost)
    v.sum().backward()
    _, e = softdtw.soft_dtw_alignment(ta, None, tb, None, gamma, cost)
    D.same_bytes(out["value"][u:u + 1], v.detach(), f"utterance {u}: value")
    D.same_bytes(out["E"][u, :Ta, :Tb], e[0], f"utterance {u}: E")
    D.same_bytes(out["g_a"][u, :, :Ta], ta.grad[0], f"utterance {u}: g_a")
    D.same_bytes(out["g_b"][u, :, :Tb], tb.grad[0], f"utterance {u}: g_b")
    # exact zeros (not -0.0, not NaN) behind the frames
    for q, t in (("E rows", out["E"][u, Ta:]), ("E columns", out["E"][u, :, Tb:]), ("g_a", out["g_a"][u, :, Ta:]),
                 ("g_b", out["g_b"][u, :, Tb:])):
      assert not D.raw(t).any(), f"utterance {u}: {q} behind the frames"
    assert bool(torch.isfinite(out["value"][u])) and bool(torch.isfinite(out["E"][u]).all())


def test_two_calls_and_two_backwards_give_the_same_bytes():
  from waveglow_amd import softdtw
  fa, na, fb, nb, _ = _batch(0.25)
  first, second = _all_outputs(fa, na, fb, nb, 0.25, "l2"), _all_outputs(fa, na, fb, nb, 0.25, "l2")
  D.same_outputs(first, second, "two calls")
  ta, tb = fa.clone().requires_grad_(True), fb.clone().requires_grad_(True)
  v = softdtw.soft_dtw(ta, na, tb, nb, 0.25, "l2").sum()
  g1 = torch.autograd.grad(v, (ta, tb), retain_graph=True)
  g2 = torch.autograd.grad(v, (ta, tb))
  D.same_bytes(g1[0], g2[0], "g_a of the second backward")
  D.same_bytes(g1[1], g2[1], "g_b of the second backward")
  D.same_bytes(g1[0], first["g_a"], "g_a against the first call")


def test_without_a_graph_only_the_values_are_computed():
  from waveglow_amd import softdtw
  fa, na, fb, nb, _ = _batch(0.25)
  with_graph = softdtw.soft_dtw(fa.clone().requires_grad_(True), na, fb, nb, 0.25)
  assert with_graph.grad_fn is not None and with_graph.dtype == torch.float64
  plain = softdtw.soft_dtw(fa, na, fb, nb, 0.25)
  with torch.no_grad():
    quiet = softdtw.soft_dtw(fa.clone().requires_grad_(True), na, fb, nb, 0.25)
  assert plain.grad_fn is None and quiet.grad_fn is None and not quiet.requires_grad
  D.same_bytes(plain, with_graph.detach(), "values without a graph")
  D.same_bytes(quiet, with_graph.detach(), "values without grad mode")
  with pytest.raises(RuntimeError):                      # no double backward
    x = fa.clone().requires_grad_(True)
    g, = torch.autograd.grad(softdtw.soft_dtw(x, na, fb, nb, 0.25).sum(), x, create_graph=True)
    g.nan_to_num(0.0).sum().backward()


@pytest.mark.parametrize("cost", cases.COSTS)
def test_a_refused_count_harms_no_other_utterance(cost):
  fa, na, fb, nb, _ = _batch(0.25)
  good = _all_outputs(fa, na, fb, nb, 0.25, cost)
  g = torch.tensor([float("nan"), 1.0, float("inf")], dtype=torch.float64, device=DEV)     # not read for a refused row
  for counts_a, counts_b in (([0, 37, PITCH_A + 1], None), (None, [PITCH_B + 1, 41, 0]), ([-5, 37, 9], [45, 41, 4097])):
    fa2, na2, fb2, nb2, _ = _batch(0.25, counts_a, counts_b)
    out = _all_outputs(fa2, na2, fb2, nb2, 0.25, cost, g)
    for u in (0, 2):
      assert bool(torch.isnan(out["value"][u])), (counts_a, counts_b, u)
      for q in ("E", "g_a", "g_b"):
        assert not D.raw(out[q][u]).any(), (counts_a, counts_b, u, q)
    for q in good:
      D.same_bytes(out[q][1], good[q][1], f"the valid utterance beside refused ones: {q}")


def test_no_output_depends_on_what_its_buffers_held(monkeypatch):
  """Values, E and both gradients through the Python layer, whose R, E and output buffers come from torch.empty."""
  fa, na, fb, nb, _ = _batch(0.25)
  for cost in cases.COSTS:
    out = D.four_runs(monkeypatch, lambda: _all_outputs(fa, na, fb, nb, 0.25, cost), f"soft_dtw {cost}")
    assert bool(torch.isfinite(out["value"]).all())


def test_a_null_alignment_buffer_gives_the_same_gradients():
  """wg_softdtw_backward with e_out null takes its own temporary: the gradients have the bits of the call that keeps E."""
  from waveglow_amd import _lib, softdtw
  lib = _lib.load()
  fa, na, fb, nb, _ = _batch(0.25)
  B, K, Ta = fa.shape
  Tb = fb.shape[2]
  value = torch.empty(B, dtype=torch.float64, device=DEV)
  r = torch.empty(softdtw.r_bytes(B, Ta, Tb) // 8, dtype=torch.float64, device=DEV)
  s = C.c_void_p(torch.cuda.current_stream().cuda_stream)
  _lib.check(lib.wg_softdtw_forward(fa.data_ptr(), na.data_ptr(), fb.data_ptr(), nb.data_ptr(), 0.25, 0, value.data_ptr(),
                                    r.data_ptr(), B, K, Ta, Tb, s))
  g = torch.ones(B, dtype=torch.float64, device=DEV)
  outs = []
  for keep in (True, False):
    e = torch.empty((B, Ta, Tb), dtype=torch.float64, device=DEV)
    g_a = torch.full((B, K, Ta), float("nan"), dtype=torch.float32, device=DEV)
    g_b = torch.full((B, K, Tb), float("nan"), dtype=torch.float32, device=DEV)
    _lib.check(lib.wg_softdtw_backward(fa.data_ptr(), na.data_ptr(), fb.data_ptr(), nb.data_ptr(), 0.25, 0, r.data_ptr(),
                                       g.data_ptr(), e.data_ptr() if keep else None, g_a.data_ptr(), g_b.data_ptr(), B, K,
                                       Ta, Tb, s))
    torch.cuda.synchronize()
    outs.append((g_a, g_b))
  D.same_bytes(outs[0][0], outs[1][0], "g_a without e_out")
  D.same_bytes(outs[0][1], outs[1][1], "g_b without e_out")
  ref = _all_outputs(fa, na, fb, nb, 0.25, "l2")
  D.same_bytes(outs[0][0], ref["g_a"], "g_a through the C entry point")


@pytest.mark.parametrize("index", (4, 5, 6), ids=cases.IDS[4:7])
def test_the_value_tends_to_the_exact_dtw_cost_on_the_device(index):
  """cost - value in [-tol, gamma (Ta + Tb) ln 3 + tol] at gamma = 1e-3: at most 3^(Ta + Tb) paths; tol = 1e-9 max(1, cost)
  covers rounding."""
  from waveglow_amd import metrics, softdtw
  K, Ta, Tb, _ = cases.CASES[index]
  a, b = cases.inputs(cases.CASES[index])
  ta, tb = _dev(a), _dev(b)
  cost, _ = metrics.dtw_distance(ta, None, tb, None)
  v = softdtw.soft_dtw(ta, None, tb, None, 1e-3, "l2")
  cost, v = float(cost[0]), float(v.detach()[0])
  tol = 1e-9 * max(1.0, cost)
  print(f"{cases.IDS[index]}: dtw {cost!r} soft {v!r} difference {cost - v:.3e}")
  assert -tol <= cost - v <= 1e-3 * (Ta + Tb) * math.log(3.0) + tol


def test_the_same_tensor_on_both_sides():
  """Autograd sums the two gradients; d(i, i) = 0 takes the root's zero gradient.  Three fp32 roundings: both outputs and
  their sum."""
  from waveglow_amd import softdtw
  a, _ = cases.inputs(cases.CASES[4])
  want = O.explicit(a, a, 1.0, "l2", np.longdouble)
  y = O.distance(O.autograd(a, a, 1.0, "l2"), O.explicit(a, a, 1.0, "l2"))["worst"]
  bar = 100.0 * max(y, 2.0 ** -52 * 2 * a.shape[1] * max(1.0, float(np.abs(want["R"]).max())))
  x = _dev(a, True)
  v = softdtw.soft_dtw(x, None, x, None, 1.0, "l2")
  v.sum().backward()
  ref = np.asarray(want["g_a"] + want["g_b"], dtype=np.float64)
  gmax = max(float(np.abs(want["g_a"]).max()), float(np.abs(want["g_b"]).max()))
  err = np.abs(x.grad[0].cpu().numpy().astype(np.float64) - ref)
  tol = 2 * bar * gmax + 3 * F32 * (np.abs(np.asarray(want["g_a"], dtype=np.float64)) + np.abs(np.asarray(want["g_b"], dtype=np.float64)))
  print(f"same tensor: value error {abs(float(v.detach()[0]) - float(want['value'])):.2e}, worst gradient error {err.max():.2e}, bar {bar:.2e}")
  assert abs(float(v.detach()[0]) - float(want["value"])) <= bar * max(1.0, abs(float(want["value"])))
  assert (err <= tol).all()


# --------------------------------------------------------------------------------------------------------- SoftDTWLoss
def test_mfcc_features_are_one_rounding_of_the_fp64_product():
  import _metrics_oracle as MO
  from waveglow_amd import softdtw
  rng = np.random.default_rng(5)
  mel = (rng.standard_normal((2, 80, 23)) * 2 - 5).astype(np.float32)
  crit = softdtw.SoftDTWLoss(device=DEV)
  got = crit.feats(torch.tensor(mel, device=DEV)).cpu().numpy()
  assert got.dtype == np.float32 and got.shape == (2, 16, 23)
  want = np.einsum("kn,bnt->bkt", MO.dct_basis(80, 16), mel.astype(np.float64))
  # the fp64 product itself carries 80 roundings of 2^-53 of its terms
  slack = 80 * 2.0 ** -53 * np.einsum("kn,bnt->bkt", np.abs(MO.dct_basis(80, 16)), np.abs(mel.astype(np.float64)))
  assert (np.abs(got.astype(np.float64) - want) <= F32 * np.abs(want) + slack).all()


def _loss_oracle(feats_a, frames_a, feats_b, frames_b, gamma, cost):
  """mean_b value_b / ((Ta_b + Tb_b) / 2) in torch fp64 (formulation (a)); feats_* are fp64 tensors [B, K, T] with a graph."""
  total = 0.0
  for u, (Ta, Tb) in enumerate(zip(frames_a, frames_b)):
    Dm = O.distances_torch(feats_a[u][:, :Ta], feats_b[u][:, :Tb], cost)
    total = total + O.value_torch(Dm, gamma) / ((Ta + Tb) / 2.0)
  return total / len(frames_a)


def _pair_bar(fa, na, fb, nb, gamma, cost):
  """The accuracy bar over the utterances of a batch of fp64 numpy features."""
  bar = 0.0
  for u, (Ta, Tb) in enumerate(zip(na, nb)):
    a, b = fa[u][:, :Ta], fb[u][:, :Tb]
    ex = O.explicit(a, b, gamma, cost)
    y = O.distance(O.autograd(a, b, gamma, cost), ex)["worst"]
    bar = max(bar, 100.0 * max(y, 2.0 ** -52 * (Ta + Tb) * max(1.0, float(np.abs(ex["R"]).max()) / gamma)))
  return bar


def _end_to_end(features):
  from waveglow_amd import softdtw
  from waveglow_amd.taco_stft import TacotronSTFT, TSTFTHParams
  taco = TacotronSTFT(TSTFTHParams(), DEV)
  gen = torch.Generator().manual_seed(11)
  audio = (torch.rand((2, 4096), generator=gen) * 0.6 - 0.3).to(DEV).requires_grad_(True)
  lengths, frames_hat, frames_ref = [4096, 3000], [17, 12], [23, 15]
  mel_ref = (torch.randn((2, 80, 23), generator=gen) * 1.5 - 6.0).to(DEV)
  crit = softdtw.SoftDTWLoss(gamma=1.0, features=features, device=DEV)
  mel_hat = taco.mel_spectrogram_differentiable(audio, lengths=lengths)
  assert tuple(mel_hat.shape) == (2, 80, 17)
  mel_hat.retain_grad()
  loss = crit(mel_hat, frames_hat, mel_ref, frames_ref)
  assert loss.dim() == 0 and loss.dtype == torch.float32
  loss.backward()
  assert bool(torch.isfinite(audio.grad).all()) and float(audio.grad.abs().max()) > 0.0
  assert not bool(audio.grad[1, 3000:].any())
  return crit, mel_hat, mel_ref, frames_hat, frames_ref, loss


def test_one_training_step_through_the_mel_front_end():
  """audio -> mel_spectrogram_differentiable -> SoftDTWLoss(features="mel") against a target of another length: the mel's
  gradient is the kernel's g_a, so it equals the oracle within the bar plus its one fp32 rounding."""
  crit, mel_hat, mel_ref, na, nb, loss = _end_to_end("mel")
  ha, hb = mel_hat.detach().cpu().double(), mel_ref.cpu().double()
  ta = ha.clone().requires_grad_(True)
  want = _loss_oracle(ta, na, hb, nb, 1.0, "l2")
  want.backward()
  bar = _pair_bar(ha.numpy(), na, hb.numpy(), nb, 1.0, "l2")
  ref = ta.grad.numpy()
  err = np.abs(mel_hat.grad.cpu().numpy().astype(np.float64) - ref)
  print(f"end to end (mel): loss {float(loss.detach())!r} oracle {float(want.detach())!r}; worst gradient error {err.max():.2e} of max|g| "
        f"{np.abs(ref).max():.3g}; bar {bar:.2e}")
  assert abs(float(loss.detach()) - float(want.detach())) <= (bar + F32) * max(1.0, abs(float(want.detach())))
  assert (err <= bar * np.abs(ref).max() + F32 * np.abs(ref)).all()
  assert not np.abs(mel_hat.grad[1, :, 12:].cpu().numpy()).any()


def test_one_training_step_with_mfcc_features():
  """The same step with the DCT in front.  The feature gradient is rounded to fp32 by the kernel and then goes through the
  transposed fp64 matmul, whose result is rounded to the mel's fp32: the first rounding reaches the mel gradient as at most
  2^-24 |basis|^T |g_feat|, the second is 2^-24 |g_mel|."""
  import _metrics_oracle as MO
  crit, mel_hat, mel_ref, na, nb, loss = _end_to_end("mfcc")
  basis = torch.tensor(MO.dct_basis(80, 16))
  ha, hb = mel_hat.detach().cpu().double(), mel_ref.cpu().double()
  ta = ha.clone().requires_grad_(True)

  def feats(m):                                      # the fp32 rounding passes the gradient through unchanged
    f = torch.matmul(basis, m)
    return f + (f.detach().float().double() - f.detach())

  fa, fb = feats(ta), feats(hb)
  fa.retain_grad()
  want = _loss_oracle(fa, na, fb, nb, 1.0, "l2")
  want.backward()
  bar = _pair_bar(fa.detach().numpy(), na, fb.numpy(), nb, 1.0, "l2")
  ref, gf = ta.grad.numpy(), fa.grad.numpy()
  err = np.abs(mel_hat.grad.cpu().numpy().astype(np.float64) - ref)
  spread = np.einsum("kn,bkt->bnt", np.abs(basis.numpy()), np.abs(gf))
  tol = bar * np.abs(gf).max() * np.abs(basis.numpy()).sum(axis=0).max() + F32 * (spread + np.abs(ref))
  print(f"end to end (mfcc): loss {float(loss.detach())!r} oracle {float(want.detach())!r}; worst gradient error {err.max():.2e} of max|g| "
        f"{np.abs(ref).max():.3g}; bar {bar:.2e}")
  assert abs(float(loss.detach()) - float(want.detach())) <= (bar + F32) * max(1.0, abs(float(want.detach())))
  assert (err <= tol).all()


def test_values_and_loss_agree_and_no_valid_utterance_gives_zero():
  from waveglow_amd import softdtw
  gen = torch.Generator().manual_seed(3)
  mel_a = (torch.randn((2, 80, 9), generator=gen) - 5.0).to(DEV).requires_grad_(True)
  mel_b = (torch.randn((2, 80, 12), generator=gen) - 5.0).to(DEV).requires_grad_(True)
  crit = softdtw.SoftDTWLoss(gamma=0.5, device=DEV)
  v = crit.values(mel_a, [9, 7], mel_b, [10, 12])
  assert v.dtype == torch.float64 and tuple(v.shape) == (2,) and v.grad_fn is not None
  loss = crit(mel_a, [9, 7], mel_b, [10, 12])
  want = ((v[0] / 9.5 + v[1] / 9.5) / 2.0).to(torch.float32)
  assert float(loss.detach()) == float(want.detach())
  # one valid utterance of two: the mean is over it alone
  na = torch.tensor([9, 0], dtype=torch.int32, device=DEV)
  nb = torch.tensor([10, 12], dtype=torch.int32, device=DEV)
  assert float(crit(mel_a, na, mel_b, nb).detach()) == float((v[0] / 9.5).to(torch.float32).detach())
  # none: 0 with zero gradients
  nb0 = torch.tensor([13, 12], dtype=torch.int32, device=DEV)
  zero = crit(mel_a, na, mel_b, nb0)
  zero.backward()
  assert float(zero.detach()) == 0.0 and zero.dtype == torch.float32
  assert not bool(mel_a.grad.any()) and not bool(mel_b.grad.any())
  assert bool(torch.isfinite(mel_a.grad).all()) and bool(torch.isfinite(mel_b.grad).all())
