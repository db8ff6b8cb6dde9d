"""GPU: the banded soft-DTW kernels (wg_softdtw_banded_forward / wg_softdtw_banded_backward), the ``band`` keyword of the
Python layer, ``soft_dtw_divergence`` and ``SoftDTWLoss(band=..., divergence=...)`` against the oracle of
tests/_softdtw_band_oracle.py, and the invariants of include/waveglow_amd.h on the banded path: a covering band gives the
dense call's bytes, E is exactly 0 outside the band, bit-reproducible, batch-independent, nothing read behind a count, no
output dependent on what its buffers held.

Accuracy bar of a case, as tests/_softdtw_cases.py: 100 max(Y, 2^-52 (Ta + Tb) max(1, max|R| / gamma)), Y the disagreement
of two oracle formulations ((a) against (b) in fp64; for the two large shapes, where cell-by-cell Python takes too long,
formulation (c) in fp64 against itself in longdouble, over value and E); relative to max(1, |value|) for the value, absolute
for E, relative to max|g| for the gradients, which add one fp32 rounding 2^-24 |g|.  The reference is formulation (b) in
longdouble, for the large shapes (c) in fp64."""
import ctypes as C
import functools
import math

import numpy as np
import pytest
import torch

import _dirty as D
import _softdtw_band_oracle as BO
import _softdtw_cases as cases
import _softdtw_oracle as O

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
F32 = 2.0 ** -24

# (K, Ta, Tb, w, gamma)
CASES = (
  (4, 1, 1, 1, 1.0),
  (4, 1, 9, 1, 1.0),
  (4, 9, 1, 2, 1.0),
  (16, 37, 41, 1, 1.0),
  (16, 40, 40, 3, 0.1),
  (8, 200, 7, 1, 0.5),
  (8, 7, 200, 1, 0.5),
  (16, 300, 290, 5, 1.0),      # rows wrap the 64-thread workgroup many times
  (16, 70, 45, 2, 0.01),
)
LARGE = (
  (2, 600, 580, 511, 1.0),     # the widest band (1024 threads), still partial
  (2, 4096, 4095, 2, 1.0),     # the int32 products at their largest
)
ids = lambda cs: [f"K{K}-{Ta}x{Tb}-w{w}-g{g:g}" for K, Ta, Tb, w, g in cs]


def _inputs(case):
  K, Ta, Tb, _, gamma = case
  return cases.inputs((K, Ta, Tb, gamma))


def _bar(y, Ta, Tb, gamma, rmax):
  return 100.0 * max(y, 2.0 ** -52 * (Ta + Tb) * max(1.0, rmax / gamma))


def _finite_max(R):
  R = np.asarray(R, dtype=np.float64)
  return float(np.abs(R[np.isfinite(R)]).max())


@functools.lru_cache(maxsize=None)
def reference(index, cost):
  """a, b, the longdouble result of formulation (b) and the bar of case ``index``.  Read-only."""
  case = CASES[index]
  _, Ta, Tb, w, gamma = case
  a, b = _inputs(case)
  f64, ld = BO.explicit(a, b, gamma, cost, w), BO.explicit(a, b, gamma, cost, w, np.longdouble)
  y = O.distance(BO.autograd(a, b, gamma, cost, w), f64)["worst"]
  return dict(a=a, b=b, ld=ld, bar=_bar(y, Ta, Tb, gamma, _finite_max(ld["R"])))


def _dev(x, grad=False):
  return torch.tensor(np.asarray(x)[None], dtype=torch.float32, device=DEV).requires_grad_(grad)


def run(a, b, gamma, cost, w):
  """One pair through the Python layer with B = 1 and tmax = its counts: value, E, g_a, g_b as numpy."""
  from waveglow_amd import softdtw
  ta, tb = _dev(a, True), _dev(b, True)
  v = softdtw.soft_dtw(ta, None, tb, None, gamma, cost, band=w)
  v.sum().backward()
  v2, e = softdtw.soft_dtw_alignment(ta, None, tb, None, gamma, cost, band=w)
  D.same_bytes(v.detach(), v2, "value of the alignment call")
  return dict(value=float(v.detach()[0]), E=e[0].cpu().numpy(), g_a=ta.grad[0].cpu().numpy(), g_b=tb.grad[0].cpu().numpy())


def check(got, want, bar, what):
  """``got`` (device; fp32 gradients) against ``want`` (longdouble oracle) within ``bar``; prints each figure first."""
  d = O.distance(got, want)
  g_ok, worst32 = True, 0.0
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


# ------------------------------------------------------------------------------------------------- against the oracle
@pytest.mark.parametrize("cost", BO.COSTS)
@pytest.mark.parametrize("index", range(len(CASES)), ids=ids(CASES))
def test_matches_the_oracle(index, cost):
  ref = reference(index, cost)
  _, Ta, Tb, w, gamma = CASES[index]
  got = run(ref["a"], ref["b"], gamma, cost, w)
  check(got, ref["ld"], ref["bar"], f"{ids(CASES)[index]} {cost}")
  M = BO.mask(Ta, Tb, w)
  assert not got["E"][~M].view(np.uint8).any(), "E outside the band is not exactly 0"
  assert got["E"][Ta - 1, Tb - 1] == 1.0


@pytest.mark.parametrize("case", LARGE, ids=ids(LARGE))
def test_value_and_alignment_at_the_limits(case):
  from waveglow_amd import softdtw
  K, Ta, Tb, w, gamma = case
  a, b = _inputs(case)
  f64 = BO.diagonal(a, b, gamma, "l2", w)
  ld = BO.diagonal(a, b, gamma, "l2", w, np.longdouble)
  y = max(abs(float(f64["value"] - ld["value"])) / max(1.0, abs(float(ld["value"]))), float(np.abs(f64["E"] - ld["E"]).max()))
  bar = _bar(y, Ta, Tb, gamma, ld["rmax"])
  del ld
  v, e = softdtw.soft_dtw_alignment(_dev(a), None, _dev(b), None, gamma, "l2", band=w)
  dv = abs(float(v[0]) - float(f64["value"])) / max(1.0, abs(float(f64["value"])))
  want = torch.tensor(f64["E"], device=DEV)
  de = float((e[0] - want).abs().max())
  print(f"{case}: value {dv:.2e} E {de:.2e}; Y {y:.2e} bar {bar:.2e}")
  assert dv <= bar and de <= bar
  i, j = torch.arange(Ta, device=DEV)[:, None], torch.arange(Tb, device=DEV)[None, :]
  outside = (i * (Tb - 1) - j * (Ta - 1)).abs() > w * max(Ta - 1, Tb - 1)
  assert bool(outside.any()) and not D.raw(e[0][outside]).any(), "E outside the band is not exactly 0"


# --------------------------------------------------------------------------------------------------------- exactness
BATCH = ((16, 70, 45, 0.01), (16, 37, 41, 1.0), (16, 9, 1, 0.5))
PITCH_A, PITCH_B = 1100, 50


def _batch(counts_a=None, counts_b=None, pitch_a=PITCH_A, pitch_b=PITCH_B):
  """The padded three-utterance batch of tests/test_gpu_softdtw.py with NaN behind every count, and the device counts."""
  K = BATCH[0][0]
  fa = torch.full((len(BATCH), K, pitch_a), float("nan"), dtype=torch.float32)
  fb = torch.full((len(BATCH), K, pitch_b), float("nan"), dtype=torch.float32)
  for u, case in enumerate(BATCH):
    a, b = cases.inputs(case)
    fa[u, :, :case[1]], fb[u, :, :case[2]] = torch.tensor(a), torch.tensor(b)
  na = torch.tensor(counts_a or [c[1] for c in BATCH], dtype=torch.int32, device=DEV)
  nb = torch.tensor(counts_b or [c[2] for c in BATCH], dtype=torch.int32, device=DEV)
  return fa.to(DEV), na, fb.to(DEV), nb


def _all_outputs(fa, na, fb, nb, gamma, cost, w, g=None):
  from waveglow_amd import softdtw
  ta, tb = fa.clone().requires_grad_(True), fb.clone().requires_grad_(True)
  v = softdtw.soft_dtw(ta, na, tb, nb, gamma, cost, band=w)
  (v * (g if g is not None else torch.ones_like(v))).nan_to_num(0.0).sum().backward()
  _, e = softdtw.soft_dtw_alignment(fa, na, fb, nb, gamma, cost, band=w)
  return dict(value=v.detach(), E=e, g_a=ta.grad, g_b=tb.grad)


@pytest.mark.parametrize("cost", BO.COSTS)
@pytest.mark.parametrize("shape", ((16, 70, 45, 44), (16, 9, 1, 1), (16, 300, 290, 289)), ids=lambda s: f"{s[1]}x{s[2]}-w{s[3]}")
def test_a_covering_band_gives_the_dense_bytes(shape, cost):
  K, Ta, Tb, w = shape
  a, b = cases.inputs((K, Ta, Tb, 0.25))
  fa, fb = _dev(a), _dev(b)
  dense, banded = _all_outputs(fa, None, fb, None, 0.25, cost, None), _all_outputs(fa, None, fb, None, 0.25, cost, w)
  D.same_outputs(banded, dense, f"band {w} covering {Ta} x {Tb}")


@pytest.mark.parametrize("cost", BO.COSTS)
def test_a_covering_band_gives_the_dense_bytes_on_the_ragged_batch(cost):
  fa, na, fb, nb = _batch()
  dense, banded = _all_outputs(fa, na, fb, nb, 0.25, cost, None), _all_outputs(fa, na, fb, nb, 0.25, cost, 69)
  D.same_outputs(banded, dense, "band 69 on the three-utterance batch")
  assert bool(torch.isfinite(banded["value"]).all())


def test_the_value_does_not_grow_with_the_band():
  from waveglow_amd import softdtw
  K, Ta, Tb, gamma = 16, 70, 45, 0.5
  a, b = cases.inputs((K, Ta, Tb, gamma))
  ta, tb = _dev(a), _dev(b)
  ex = O.explicit(a, b, gamma, "l2")
  bar = _bar(O.distance(O.autograd(a, b, gamma, "l2"), ex)["worst"], Ta, Tb, gamma, float(np.abs(ex["R"]).max()))
  v = [float(softdtw.soft_dtw(ta, None, tb, None, gamma, band=w)[0]) for w in (1, 2, 5, 20, None)]
  print(f"values at w = 1, 2, 5, 20, dense: {v}; bar {bar:.2e}")
  for x, y in zip(v, v[1:]):
    assert x >= y - bar * max(1.0, abs(y))


@pytest.mark.parametrize("shape", ((16, 37, 41, 1), (16, 70, 45, 2), (16, 40, 40, 3)), ids=lambda s: f"{s[1]}x{s[2]}-w{s[3]}")
def test_the_value_tends_to_the_banded_dtw_cost(shape):
  """cost - value in [-tol, gamma (Ta + Tb) ln 3 + tol] at gamma = 1e-3: at most 3^(Ta + Tb) paths; tol = 1e-9 max(1, cost)."""
  from waveglow_amd import softdtw
  K, Ta, Tb, w = shape
  a, b = cases.inputs((K, Ta, Tb, 1.0))
  cost = BO.dtw(a, b, "l2", w)
  v = float(softdtw.soft_dtw(_dev(a), None, _dev(b), None, 1e-3, "l2", band=w)[0])
  tol = 1e-9 * max(1.0, cost)
  print(f"{shape}: banded dtw {cost!r} soft {v!r} difference {cost - v:.3e}")
  assert -tol <= cost - v <= 1e-3 * (Ta + Tb) * math.log(3.0) + tol


# -------------------------------------------------------------------------------- the header's invariants, with a band
@pytest.mark.parametrize("cost", BO.COSTS)
def test_an_utterance_has_the_bits_of_its_own_call(cost):
  from waveglow_amd import softdtw
  gamma, w = 0.25, 2
  fa, na, fb, nb = _batch()
  out = _all_outputs(fa, na, fb, nb, gamma, cost, w)
  for u, case in enumerate(BATCH):
    Ta, Tb = case[1], case[2]
    a, b = cases.inputs(case)
    ta, tb = _dev(a, True), _dev(b, True)
    v = softdtw.soft_dtw(ta, [Ta], tb, [Tb], gamma, cost, band=w)
    v.sum().backward()
    _, e = softdtw.soft_dtw_alignment(ta, None, tb, None, gamma, cost, band=w)
    D.same_bytes(out["value"][u:u + 1], v.detach(), f"utterance {u}: value")
    D.same_bytes(out["E"][u, :Ta, :Tb], e[0], f"utterance {u}: E")
    D.same_bytes(out["g_a"][u, :, :Ta], ta.grad[0], f"utterance {u}: g_a")
    D.same_bytes(out["g_b"][u, :, :Tb], tb.grad[0], f"utterance {u}: g_b")
    for q, t in (("E rows", out["E"][u, Ta:]), ("E columns", out["E"][u, :, Tb:]), ("g_a", out["g_a"][u, :, Ta:]),
                 ("g_b", out["g_b"][u, :, Tb:])):
      assert not D.raw(t).any(), f"utterance {u}: {q} behind the frames"
    outside = torch.tensor(~BO.mask(Ta, Tb, w), device=DEV)
    assert not D.raw(out["E"][u, :Ta, :Tb][outside]).any(), f"utterance {u}: E outside the band"
    assert bool(torch.isfinite(out["value"][u])) and bool(torch.isfinite(out["E"][u]).all())


def test_two_calls_and_two_backwards_give_the_same_bytes():
  from waveglow_amd import softdtw
  fa, na, fb, nb = _batch()
  first, second = _all_outputs(fa, na, fb, nb, 0.25, "l2", 2), _all_outputs(fa, na, fb, nb, 0.25, "l2", 2)
  D.same_outputs(first, second, "two calls")
  ta, tb = fa.clone().requires_grad_(True), fb.clone().requires_grad_(True)
  v = softdtw.soft_dtw(ta, na, tb, nb, 0.25, "l2", band=2).sum()
  g1 = torch.autograd.grad(v, (ta, tb), retain_graph=True)
  g2 = torch.autograd.grad(v, (ta, tb))
  D.same_bytes(g1[0], g2[0], "g_a of the second backward")
  D.same_bytes(g1[1], g2[1], "g_b of the second backward")
  D.same_bytes(g1[0], first["g_a"], "g_a against the first call")


def _c_calls(fill, keep_e=True):
  """Forward and backward through the C entry points with every buffer filled with ``fill`` before."""
  from waveglow_amd import _lib, softdtw
  lib = _lib.load()
  fa, na, fb, nb = _batch()
  B, K, Ta = fa.shape
  Tb, w = fb.shape[2], 2
  s = C.c_void_p(torch.cuda.current_stream().cuda_stream)
  value = torch.full((B,), fill, dtype=torch.float64, device=DEV)
  r = torch.full((softdtw.r_bytes(B, Ta, Tb, w) // 8,), fill, dtype=torch.float64, device=DEV)
  _lib.check(lib.wg_softdtw_banded_forward(fa.data_ptr(), na.data_ptr(), fb.data_ptr(), nb.data_ptr(), 0.25, 0,
                                           value.data_ptr(), r.data_ptr(), B, K, Ta, Tb, w, s))
  g = torch.ones(B, dtype=torch.float64, device=DEV)
  e = torch.full((B, Ta, Tb), fill, dtype=torch.float64, device=DEV)
  g_a = torch.full((B, K, Ta), fill, dtype=torch.float32, device=DEV)
  g_b = torch.full((B, K, Tb), fill, dtype=torch.float32, device=DEV)
  _lib.check(lib.wg_softdtw_banded_backward(fa.data_ptr(), na.data_ptr(), fb.data_ptr(), nb.data_ptr(), 0.25, 0, r.data_ptr(),
                                            g.data_ptr(), e.data_ptr() if keep_e else None, g_a.data_ptr(), g_b.data_ptr(),
                                            B, K, Ta, Tb, w, s))
  torch.cuda.synchronize()
  out = dict(value=value, g_a=g_a, g_b=g_b)
  if keep_e:
    out["E"] = e
  return out


def test_no_output_depends_on_what_its_buffers_held(monkeypatch):
  """Through the C entry points from NaN-filled and from 2.4e35-filled buffers, and through the Python layer, whose R and
  output buffers come from torch.empty."""
  zero, nan, big = _c_calls(0.0), _c_calls(float("nan")), _c_calls(2.4e35)
  D.same_outputs(nan, zero, "NaN-filled buffers")
  D.same_outputs(big, zero, "buffers filled with a large finite value")
  fa, na, fb, nb = _batch()
  ref = _all_outputs(fa, na, fb, nb, 0.25, "l2", 2)
  D.same_outputs({q: zero[q] for q in ref}, ref, "the C entry points against the Python layer")
  out = D.four_runs(monkeypatch, lambda: _all_outputs(fa, na, fb, nb, 0.25, "sq", 2), "soft_dtw sq band 2")
  assert bool(torch.isfinite(out["value"]).all())


def test_a_null_alignment_buffer_gives_the_same_gradients():
  kept, null = _c_calls(float("nan")), _c_calls(float("nan"), keep_e=False)
  D.same_outputs(null, {q: kept[q] for q in null}, "e_out null")


@pytest.mark.parametrize("cost", BO.COSTS)
def test_a_refused_count_harms_no_other_utterance(cost):
  fa, na, fb, nb = _batch()
  good = _all_outputs(fa, na, fb, nb, 0.25, cost, 2)
  g = torch.tensor([float("nan"), 1.0, float("inf")], dtype=torch.float64, device=DEV)     # not read for a refused row
  for counts_a, counts_b in (([0, 37, PITCH_A + 1], None), (None, [PITCH_B + 1, 41, 0]), ([-5, 37, 9], [45, 41, 4097])):
    fa2, na2, fb2, nb2 = _batch(counts_a, counts_b)
    out = _all_outputs(fa2, na2, fb2, nb2, 0.25, cost, 2, g)
    for u in (0, 2):
      assert bool(torch.isnan(out["value"][u])), (counts_a, counts_b, u)
      for q in ("E", "g_a", "g_b"):
        assert not D.raw(out[q][u]).any(), (counts_a, counts_b, u, q)
    for q in good:
      D.same_bytes(out[q][1], good[q][1], f"the valid utterance beside refused ones: {q}")


def test_without_a_graph_only_the_values_are_computed(monkeypatch):
  from waveglow_amd import softdtw
  fa, na, fb, nb = _batch()
  kept = []
  forward = softdtw._forward
  monkeypatch.setattr(softdtw, "_forward", lambda *args: kept.append(args[6]) or forward(*args))
  with_graph = softdtw.soft_dtw(fa.clone().requires_grad_(True), na, fb, nb, 0.25, band=2)
  assert with_graph.grad_fn is not None and with_graph.dtype == torch.float64
  plain = softdtw.soft_dtw(fa, na, fb, nb, 0.25, band=2)
  with torch.no_grad():
    quiet = softdtw.soft_dtw(fa.clone().requires_grad_(True), na, fb, nb, 0.25, band=2)
    dq = softdtw.soft_dtw_divergence(fa.clone().requires_grad_(True), na, fb, nb, 0.25, band=2)
  assert kept == [True, False, False, False]               # whether R is kept
  assert plain.grad_fn is None and quiet.grad_fn is None and not quiet.requires_grad and dq.grad_fn is None
  D.same_bytes(plain, with_graph.detach(), "values without a graph")
  D.same_bytes(quiet, with_graph.detach(), "values without grad mode")


# -------------------------------------------------------------------------------------------------------- divergence
@pytest.mark.parametrize("w", (None, 2), ids=("dense", "band2"))
@pytest.mark.parametrize("cost", BO.COSTS)
def test_the_divergence_of_a_sequence_with_itself_is_zero(cost, w):
  """D(x, x) = v - (v + v) / 2 is an exact 0.  Its gradient with respect to the left side is G_a - (G_a + G_b') / 2, G the
  gradient of the plain value there: three fp32 roundings and one fp32 sum, at most 4 * 2^-24 max|G|."""
  from waveglow_amd import softdtw
  a, _ = cases.inputs((16, 37, 41, 1.0))
  x, y = _dev(a, True), _dev(a)
  d = softdtw.soft_dtw_divergence(x, None, y, None, 1.0, cost, band=w)
  assert not D.raw(d).any(), float(d.detach()[0])
  d.sum().backward()
  p, q = _dev(a, True), _dev(a, True)
  softdtw.soft_dtw(p, None, q, None, 1.0, cost, band=w).sum().backward()
  gmax = max(float(p.grad.abs().max()), float(q.grad.abs().max()))
  print(f"D(x, x) {cost} band {w}: max|grad| {float(x.grad.abs().max()):.3e}, max|G| {gmax:.3e}")
  assert float(x.grad.abs().max()) <= 4 * F32 * gmax
  both = _dev(a, True)                                       # the same tensor on both sides
  d2 = softdtw.soft_dtw_divergence(both, None, both, None, 1.0, cost, band=w)
  d2.sum().backward()
  assert float(d2.detach()[0]) == 0.0 and float(both.grad.abs().max()) <= 8 * F32 * gmax


@pytest.mark.parametrize("w", (None, 2), ids=("dense", "band2"))
@pytest.mark.parametrize("cost", BO.COSTS)
def test_the_divergence_is_the_combination_of_three_calls(cost, w):
  """On the ragged batch with NaN behind the counts: D has the bits of v_ab - 0.5 (v_aa + v_bb) from three ``soft_dtw`` calls
  at other pitches; its gradients are the fp32 sums of three fp32 terms, within 2^-24 (|g1| + |g2| + |g3|) of their exact
  combination."""
  from waveglow_amd import softdtw
  gamma = 0.25
  fa, na, fb, nb = _batch(pitch_a=80, pitch_b=50)
  ta, tb = fa.clone().requires_grad_(True), fb.clone().requires_grad_(True)
  d = softdtw.soft_dtw_divergence(ta, na, tb, nb, gamma, cost, band=w)
  d.sum().backward()
  leaves = [t.clone().requires_grad_(True) for t in (fa, fb, fa, fa, fb, fb)]
  a1, b1, a2, a3, b2, b3 = leaves
  v_ab = softdtw.soft_dtw(a1, na, b1, nb, gamma, cost, band=w)
  v_aa = softdtw.soft_dtw(a2, na, a3, na, gamma, cost, band=w)
  v_bb = softdtw.soft_dtw(b2, nb, b3, nb, gamma, cost, band=w)
  D.same_bytes(d.detach(), (v_ab - 0.5 * (v_aa + v_bb)).detach(), "D against three calls")
  assert bool(torch.isfinite(d).all())
  (v_ab.sum() + v_aa.sum() + v_bb.sum()).backward()
  for name, got, (g1, g2, g3), n in (("g_a", ta.grad, (a1.grad, a2.grad, a3.grad), na), ("g_b", tb.grad, (b1.grad, b2.grad, b3.grad), nb)):
    g1, g2, g3 = g1.double(), -0.5 * g2.double(), -0.5 * g3.double()
    err, tol = (got.double() - (g1 + g2 + g3)).abs(), F32 * (g1.abs() + g2.abs() + g3.abs())
    print(f"{name} {cost} band {w}: worst error over its tolerance {float((err / tol.clamp(min=1e-300)).max()):.2f}")
    assert bool((err <= tol).all()), name
    for u in range(len(BATCH)):
      assert not D.raw(got[u, :, int(n[u]):]).any(), f"{name} behind the frames of utterance {u}"


def test_a_refused_count_refuses_all_three_pairs_of_the_divergence():
  from waveglow_amd import softdtw
  outs = []
  for counts_a, counts_b in ((None, None), ([0, 37, 9], [45, 41, 51])):
    fa, na, fb, nb = _batch(counts_a, counts_b, pitch_a=80, pitch_b=50)
    ta, tb = fa.clone().requires_grad_(True), fb.clone().requires_grad_(True)
    d = softdtw.soft_dtw_divergence(ta, na, tb, nb, 0.25, band=2)
    d.nan_to_num(0.0).sum().backward()
    outs.append(dict(value=d.detach(), g_a=ta.grad, g_b=tb.grad))
  good, out = outs
  for u in (0, 2):
    assert bool(torch.isnan(out["value"][u]))
    assert not D.raw(out["g_a"][u]).any() and not D.raw(out["g_b"][u]).any()
  for q in good:
    D.same_bytes(out[q][1], good[q][1], f"the valid utterance beside refused ones: {q}")


DIV = ((16, 37, 41, None, 1.0), (16, 37, 41, 2, 1.0), (8, 20, 33, None, 0.1), (16, 70, 45, 3, 0.5))


@functools.lru_cache(maxsize=None)
def div_reference(index, cost):
  K, Ta, Tb, w, gamma = DIV[index]
  a, b = cases.inputs((K, Ta, Tb, gamma))
  ld = BO.divergence(a, b, gamma, cost, w, np.longdouble)
  f64 = BO.divergence(a, b, gamma, cost, w)
  au = BO.divergence(a, b, gamma, cost, w, fn=lambda x, y: BO.autograd(x, y, gamma, cost, w))
  bar = 0.0
  for (x, y), p, (ta_, tb_) in zip(zip(au["parts"], f64["parts"]), ld["parts"], ((Ta, Tb), (Ta, Ta), (Tb, Tb))):
    bar = max(bar, _bar(O.distance(x, y)["worst"], ta_, tb_, gamma, _finite_max(p["R"])))
  return dict(a=a, b=b, ld=ld, bar=bar)


@pytest.mark.parametrize("cost", BO.COSTS)
@pytest.mark.parametrize("index", range(len(DIV)), ids=[f"{c[1]}x{c[2]}-w{c[3]}" for c in DIV])
def test_the_divergence_matches_the_oracle(index, cost):
  """Each of the three values is within bar max(1, |v|) and each gradient term within bar max|g| of its pair plus its fp32
  rounding, so D is within bar (m_ab + (m_aa + m_bb) / 2), m = max(1, |v|), and a gradient within bar (G_ab + G_self) plus
  the three roundings and that of the fp32 sum, 4 * 2^-24 (|g1| + |g2| + |g3|).  For the squared cost without a band D >= 0
  is a theorem (Blondel, Mensch and Vert 2021); the oracle's own D is checked for it first."""
  from waveglow_amd import softdtw
  K, Ta, Tb, w, gamma = DIV[index]
  ref = div_reference(index, cost)
  ld, bar = ref["ld"], ref["bar"]
  ta, tb = _dev(ref["a"], True), _dev(ref["b"], True)
  d = softdtw.soft_dtw_divergence(ta, None, tb, None, gamma, cost, band=w)
  d.sum().backward()
  m = [max(1.0, abs(float(ld[q]))) for q in ("v_ab", "v_aa", "v_bb")]
  dv = abs(float(d[0]) - float(ld["value"]))
  print(f"{DIV[index]} {cost}: D {float(d[0])!r} oracle {float(ld['value'])!r} error {dv:.2e}; bar {bar:.2e}")
  assert dv <= bar * (m[0] + 0.5 * (m[1] + m[2]))
  ab, aa, bb = ld["parts"]
  gmax = lambda p: max(float(np.abs(p["g_a"]).max()), float(np.abs(p["g_b"]).max()))
  for name, got, want, terms, self_ in (("g_a", ta.grad, ld["g_a"], (ab["g_a"], 0.5 * aa["g_a"], 0.5 * aa["g_b"]), aa),
                                        ("g_b", tb.grad, ld["g_b"], (ab["g_b"], 0.5 * bb["g_a"], 0.5 * bb["g_b"]), bb)):
    err = np.abs(got[0].cpu().numpy().astype(np.float64) - np.asarray(want, dtype=np.float64))
    tol = bar * (gmax(ab) + gmax(self_)) + 4 * F32 * np.asarray(sum(np.abs(t) for t in terms), dtype=np.float64)
    print(f"  {name}: worst error {err.max():.2e}, over its tolerance {float((err / tol).max()):.2f}")
    assert (err <= tol).all(), name
  if cost == "sq" and w is None:
    assert float(ld["value"]) >= 0.0
    assert float(d[0]) >= -bar * max(1.0, abs(float(ld["v_ab"])))


# --------------------------------------------------------------------------------------------------------- SoftDTWLoss
def test_one_optimiser_step_with_band_divergence_and_mfcc_features(monkeypatch):
  """mel -> DCT -> banded divergence -> loss -> SGD step.  The feature gradient is the fp32 sum of three fp32 kernel outputs
  and goes through the transposed fp64 matmul, whose result is rounded to the mel's fp32: tolerance in the form of
  tests/test_gpu_softdtw.py, bar max|g_feat| max_n sum_k |basis| + 2^-24 (|basis|^T (4 sum of the |terms|) + |g_mel|)."""
  import _metrics_oracle as MO
  from waveglow_amd import softdtw
  gen = torch.Generator().manual_seed(21)
  B, n_mel, Ta, Tb, w, gamma = 2, 80, 40, 37, 3, 1.0
  na, nb = [40, 33], [37, 30]
  walk = lambda T: (torch.cumsum(torch.randn((B, n_mel, T), generator=gen) * 0.3, dim=2) - 6.0)
  mel_hat = torch.nn.Parameter(walk(Ta).to(DEV))
  mel_ref = walk(Tb).to(DEV)
  crit = softdtw.SoftDTWLoss(gamma=gamma, features="mfcc", cost="sq", device=DEV, band=w, divergence=True)
  kept = []
  forward = softdtw._forward

  def spy(*args):                                     # what the one forward call keeps: R and the features it read
    out = forward(*args)
    kept.append((out[1], args[0], args[2]))
    return out

  monkeypatch.setattr(softdtw, "_forward", spy)
  opt = torch.optim.SGD([mel_hat], lr=0.1)
  before = mel_hat.detach().clone()
  loss = crit(mel_hat, na, mel_ref, nb)
  loss.backward()
  loss, (r, a3, b3) = loss.detach(), kept[0]
  assert len(kept) == 1
  assert tuple(a3.shape) == (3 * B, 16, Ta) and tuple(b3.shape) == (3 * B, 16, Ta)
  assert crit.workspace_bytes(B, Ta, Tb, n_mel) == 8 * r.numel() + 4 * (a3.numel() + b3.numel()) + 8 * B * n_mel * (Ta + Tb)
  assert loss.dim() == 0 and loss.dtype == torch.float32 and math.isfinite(float(loss)) and float(loss) >= 0.0
  grad = mel_hat.grad.detach().clone()
  opt.step()
  assert bool(torch.isfinite(mel_hat).all()) and not torch.equal(mel_hat.detach(), before)
  assert not bool(grad[1, :, 33:].any())

  basis = torch.tensor(MO.dct_basis(n_mel, 16))
  hm = before.cpu().double().requires_grad_(True)
  rm = mel_ref.cpu().double()

  def feats(mm):                                      # the fp32 rounding passes the gradient through unchanged
    f = torch.matmul(basis, mm)
    return f + (f.detach().float().double() - f.detach())

  fa, fb = feats(hm), feats(rm)
  terms, bar = [0.0, 0.0, 0.0], 0.0
  for u in range(B):
    x, y = fa[u][:, :na[u]], fb[u][:, :nb[u]]
    for t, (p, q, scale) in enumerate(((x, y, 1.0), (x, x, -0.5), (y, y, -0.5))):
      v = BO.value_torch(O.distances_torch(p, q, "sq"), gamma, BO.mask(p.shape[1], q.shape[1], w))
      terms[t] = terms[t] + scale * v / ((na[u] + nb[u]) / 2.0) / B
      pn, qn = p.detach().numpy(), q.detach().numpy()
      ex = BO.explicit(pn, qn, gamma, "sq", w)
      bar = max(bar, _bar(O.distance(BO.autograd(pn, qn, gamma, "sq", w), ex)["worst"], p.shape[1], q.shape[1], gamma,
                          _finite_max(ex["R"])))
  want = terms[0] + terms[1] + terms[2]
  terms_v = [float(t.detach()) for t in terms]
  gf = [torch.autograd.grad(t, fa, retain_graph=True)[0].numpy() for t in terms[:2]]
  ref, = torch.autograd.grad(want, hm)
  ref = ref.numpy()
  err = np.abs(grad.cpu().numpy().astype(np.float64) - ref)
  absb = np.abs(basis.numpy())
  spread = np.einsum("kn,bkt->bnt", absb, 4 * (np.abs(gf[0]) + np.abs(gf[1])))
  tol = bar * 2 * max(np.abs(g).max() for g in gf) * absb.sum(axis=0).max() + F32 * (spread + np.abs(ref))
  want = float(want.detach())
  print(f"end to end: loss {float(loss)!r} oracle {want!r}; worst gradient error {err.max():.2e} of max|g| "
        f"{np.abs(ref).max():.3g}, over its tolerance {float((err / tol).max()):.2f}; bar {bar:.2e}")
  assert abs(float(loss) - want) <= (3 * bar + F32) * max(1.0, abs(want), *(abs(t) for t in terms_v))
  assert (err <= tol).all()
