"""GPU: ``Denoiser.forward_differentiable`` -- the denoiser under autograd (wg_stft_denoise_forward_saved /
wg_stft_denoise_backward).

Values: bit for bit ``Denoiser.forward``.  Gradients: against the fp64 restatement of tests/_denoiser_grad_oracle.py in both
phase modes and, with the phase detached, against the gradients of the reference's own autograd
(tests/golden/denoiser_grads.npz), at GRAD_TOL of tests/test_gpu_mel_grads.py -- the bar of the same class of exact-fp32
MFMA GEMMs -- per utterance.  tests/test_denoiser_grad_cpu.py holds the restatement to the reference and to a central
difference, and asserts that no compared cell lies within 1e-4 of its clamp.  Measured on the MI355X: see each test.
"""
import ctypes as C

import numpy as np
import pytest
import torch

import _denoiser_grad_oracle as D
from test_gpu_mel_grads import GRAD_TOL
from test_gpu_parity import build_model
from waveglow_amd import Denoiser, _lib, synthetic
from waveglow_amd.hparams import HParams
from waveglow_amd.taco_stft import TSTFTHParams

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
NAN = float("nan")
HALF = dict(D.STRENGTHS)["shalf"]


class _Vocoder:
  """What ``Denoiser.__init__`` asks of a vocoder; the bias it yields is replaced by the cases' bias."""

  class _Up:
    weight = None

  def __init__(self):
    self.upsample = self._Up()
    self.upsample.weight = torch.zeros(1, device=DEV)

  @staticmethod
  def infer(mel, sigma):
    return torch.full((1, 256 * mel.shape[2]), 0.01, device=DEV)


@pytest.fixture(scope="module")
def den():
  d = Denoiser(_Vocoder(), TSTFTHParams(), "zeros", DEV)
  d.bias_spec.copy_(torch.from_numpy(D.make_bias()).to(DEV)[None, :, None])
  return d


@pytest.fixture(scope="module")
def refs():
  """fp64 reference gradients, each computed once: (case, strength, phase_grad) -> [B, N]."""
  cache = {}
  bias = D.make_bias()

  def get(case, s, phase_grad):
    key = (case, s, phase_grad)
    if key not in cache:
      x, r, lens = inputs(case)
      cache[key] = D.grad64(x, r, bias, s, phase_grad) if lens is None else D.grad64_ragged(x, r, lens, bias, s, phase_grad)
    return cache[key]
  return get


def inputs(case):
  """(x, r, lengths or None) of a case as fp32 CPU tensors."""
  if case == "ragged":
    x, lens = D.ragged_input(), list(D.RAGGED_LENS)
    r = D.make_weights(case, len(lens), D.RAGGED_PITCH)[1]
    return torch.from_numpy(x), torch.from_numpy(r), lens
  if case == "gap":
    return torch.from_numpy(D.gap_input()), torch.from_numpy(D.make_weights(case, D.DENSE_B, D.GAP_N)[1]), None
  N = int(case[1:])
  return torch.from_numpy(D.make_input(case, D.DENSE_B, N)[1]), torch.from_numpy(D.make_weights(case, D.DENSE_B, N)[1]), None


def run(den, x, r, s, lengths=None, phase_grad=True):
  """(out [B, N], d <r, out> / d x [B, N]) on the CPU."""
  xg = x.to(DEV).requires_grad_(True)
  out = den.forward_differentiable(xg, s, lengths=lengths, phase_grad=phase_grad)
  assert out.shape == (x.shape[0], 1, x.shape[1]) and out.grad_fn is not None
  out.backward(r.to(DEV)[:, None, :])
  torch.cuda.synchronize()
  return out.detach()[:, 0].cpu(), xg.grad.cpu()


def rel_rows(g, ref, lens=None):
  """Relative L2 distance per utterance."""
  g, ref = g.double(), ref.double()
  n = [g.shape[1]] * g.shape[0] if lens is None else lens
  return [float((g[b, :n[b]] - ref[b, :n[b]]).norm() / ref[b, :n[b]].norm()) for b in range(g.shape[0])]


DENSE = [f"N{N}" for N in D.DENSE_N]


@pytest.mark.parametrize("case", DENSE + ["gap", "ragged"])
def test_forward_bits(den, case):
  """forward_differentiable is torch.equal to forward, with and without a graph, at every strength."""
  x, _, lens = inputs(case)
  xd = x.to(DEV)
  for _, s in D.STRENGTHS:
    want = den(xd, s) if lens is None else den(xd, s, lengths=lens)
    xg = xd.clone().requires_grad_(True)
    with_graph = den.forward_differentiable(xg, s, lengths=lens)
    assert with_graph.grad_fn is not None and with_graph.shape == want.shape == (x.shape[0], 1, x.shape[1])
    assert torch.equal(with_graph.detach(), want)
    plain = den.forward_differentiable(xd, s, lengths=lens)
    with torch.no_grad():
      no_grad = den.forward_differentiable(xg, s, lengths=lens)
    assert plain.grad_fn is None and no_grad.grad_fn is None
    assert torch.equal(plain, want) and torch.equal(no_grad, want)
    if lens is not None:
      ld = torch.tensor(lens, dtype=torch.int32).to(DEV)
      assert torch.equal(den.forward_differentiable(xg, s, lengths=ld).detach(), want)
      assert torch.equal(den.forward_differentiable(xd, s, lengths=ld), want)


@pytest.mark.parametrize("phase_grad", (True, False))
@pytest.mark.parametrize("case", DENSE + ["gap", "ragged"])
def test_gradient_matches_oracle(den, refs, case, phase_grad):
  """Both phase modes against the fp64 restatement, per utterance, at s = 0 and at the strength that clamps half the cells.
  Measured on the MI355X: rel L2 7.0e-7 ... 1.0e-6 with the phase gradient, 7.0e-7 ... 2.2e-6 without (the worst at
  N = 1024, s = 0)."""
  x, r, lens = inputs(case)
  for s in (0.0, HALF):
    _, g = run(den, x, r, s, lens, phase_grad)
    ref = refs(case, s, phase_grad)
    assert g.shape == ref.shape and torch.isfinite(g).all()
    errs = rel_rows(g, ref, lens)
    print(f"{case} s={s} phase_grad={phase_grad}: rel L2 per utterance {['%.2e' % e for e in errs]}")
    assert max(errs) <= GRAD_TOL


@pytest.mark.parametrize("N", D.DENSE_N)
def test_gradient_matches_reference_autograd(den, N):
  """phase_grad=False against what the reference's own STFT and Denoiser give under autograd (fp32, CPU).
  Measured on the MI355X: rel L2 6.8e-7 ... 1.2e-6 (the fp64 restatement is 4.4e-7 ... 1.9e-6 from the same fixture)."""
  fx = D.fixture()
  x, r = torch.from_numpy(fx.audio(f"N{N}/x_q")), torch.from_numpy(fx.audio(f"N{N}/r_q"))
  assert np.array_equal(fx.bias(), den.bias_spec.reshape(-1).cpu().numpy())
  for sname, s in D.STRENGTHS:
    ref, is_zero = fx.grad(N, sname)
    _, g = run(den, x, r, s, None, False)
    if is_zero:
      assert s == 1e4 and not g.any()
      continue
    errs = rel_rows(g, torch.from_numpy(ref))
    print(f"N={N} {sname}: rel L2 vs the reference's gradient per utterance {['%.2e' % e for e in errs]}")
    assert max(errs) <= GRAD_TOL


@pytest.mark.parametrize("phase_grad", (True, False))
def test_exact_zeros(den, phase_grad):
  """Every cell clamps at s = 1e4: the gradient is exactly 0.  Silent frames (mag == 0) give 0, never NaN: a cotangent
  that is non-zero only where the silent frames alone reach gives an all-zero gradient."""
  for case in DENSE + ["ragged"]:
    x, r, lens = inputs(case)
    out, g = run(den, x, r, 1e4, lens, phase_grad)
    assert not out.any() and not g.any(), case
  x, r, _ = inputs("gap")
  lo, hi = D.GAP_ONLY_SILENT
  for s in (0.0, HALF, -0.5):
    _, g = run(den, x, r, s, None, phase_grad)
    assert torch.isfinite(g).all() and g.any()
    masked = torch.zeros_like(r)
    masked[:, lo:hi] = r[:, lo:hi]
    _, g0 = run(den, x, masked, s, None, phase_grad)
    assert masked.any() and not g0.any(), f"s={s}: silent frames contribute {float(g0.abs().max()):.3e}"


@pytest.mark.parametrize("phase_grad", (True, False))
def test_ragged_rows_have_their_dense_bits(den, phase_grad):
  """Row b of a ragged batch has the bits of the B = 1 dense call on its crop and exact zeros behind its length, with NaN
  planted behind every length in the audio and in the incoming gradient."""
  x, r, lens = inputs("ragged")
  xn, rn = x.clone(), r.clone()
  for b, n in enumerate(lens):
    xn[b, n:], rn[b, n:] = NAN, NAN
  out, g = run(den, xn, rn, HALF, lens, phase_grad)
  assert torch.isfinite(out).all() and torch.isfinite(g).all()
  for b, n in enumerate(lens):
    o1, g1 = run(den, x[b:b + 1, :n].contiguous(), r[b:b + 1, :n].contiguous(), HALF, None, phase_grad)
    assert torch.equal(out[b, :n], o1[0]) and torch.equal(g[b, :n], g1[0]), f"row {b} differs from its dense call"
    assert g1.any() and not out[b, n:].any() and not g[b, n:].any(), f"row {b}: not zero behind its length"
  # CPU tensor and tuple lengths give the same bits
  _, g_t = run(den, xn, rn, HALF, torch.tensor(lens, dtype=torch.int64), phase_grad)
  _, g_u = run(den, xn, rn, HALF, tuple(lens), phase_grad)
  assert torch.equal(g_t, g) and torch.equal(g_u, g)


def test_full_lengths_give_the_dense_bits(den):
  x, r, _ = inputs("N8448")
  out, g = run(den, x, r, HALF)
  out_l, g_l = run(den, x, r, HALF, [x.shape[1]] * x.shape[0])
  assert torch.equal(out, out_l) and torch.equal(g, g_l)


def test_device_lengths_outside_the_limits_zero_their_row(den):
  """An int32 device tensor is trusted: a count outside the limits (not a multiple of 256, below 1024, above the pitch)
  zeroes that row's output and gradient and leaves the other rows' bits alone."""
  x, r, lens = inputs("ragged")
  _, g_ok = run(den, x, r, HALF, lens)
  out_ok = den(x.to(DEV), HALF, lengths=lens)[:, 0].cpu()
  for bad in (1000, 768, D.RAGGED_PITCH + 256, 0, -256):
    ld = torch.tensor([lens[0], bad, lens[2]], dtype=torch.int32).to(DEV)
    out, g = run(den, x, r, HALF, ld)
    assert not out[1].any() and not g[1].any(), bad
    for b in (0, 2):
      assert torch.equal(out[b], out_ok[b]) and torch.equal(g[b], g_ok[b]), (bad, b)


def _abi(den, x, r, lens, fill_before, refill_scratch):
  """forward_saved + backward through the C ABI with a caller-owned workspace.  ``fill_before``: byte the workspace holds
  before forward_saved.  ``refill_scratch``: overwrite everything but the saved state with 0xFF between the two calls."""
  lib, h = den.lib, den._h
  B, N = x.shape
  nbytes = lib.wg_stft_denoise_grad_workspace_bytes(h, B, N)
  assert nbytes > 0 and nbytes == den.grad_workspace_bytes(B, N)
  saved = (nbytes - B * 1024 * 4) // 2                      # waveglow_amd.h: the saved state is the workspace's tail
  ws = torch.full((nbytes,), fill_before, dtype=torch.uint8, device=DEV)
  xd, rd = x.to(DEV), r.to(DEV)
  bias = den.bias_spec.reshape(-1).contiguous()
  ld = torch.tensor(lens, dtype=torch.int32).to(DEV) if lens is not None else None
  lp = ld.data_ptr() if ld is not None else None
  out = torch.full_like(xd, NAN)
  g = torch.full_like(xd, NAN)
  _lib.check(lib.wg_stft_denoise_forward_saved(h, xd.data_ptr(), lp, bias.data_ptr(), HALF, out.data_ptr(), B, N,
                                               ws.data_ptr(), nbytes, None))
  if refill_scratch:
    ws[:nbytes - saved] = 0xFF
  _lib.check(lib.wg_stft_denoise_backward(h, rd.data_ptr(), lp, bias.data_ptr(), HALF, 1, g.data_ptr(), B, N,
                                          ws.data_ptr(), nbytes, None))
  torch.cuda.synchronize()
  return out.cpu(), g.cpu()


@pytest.mark.parametrize("case", ["N8448", "ragged"])
def test_workspace_contents_do_not_matter(den, case):
  """A workspace full of NaN bit patterns before forward_saved, and NaN in all of it but the saved state before the
  backward, change no bit."""
  x, r, lens = inputs(case)
  out0, g0 = _abi(den, x, r, lens, 0, False)
  out_m, g_m = run(den, x, r, HALF, lens)
  assert torch.equal(out0, out_m) and torch.equal(g0, g_m)       # the module is this pair of calls
  out1, g1 = _abi(den, x, r, lens, 0xFF, False)
  out2, g2 = _abi(den, x, r, lens, 0xFF, True)
  assert torch.isfinite(g0).all() and g0.any()
  assert torch.equal(out1, out0) and torch.equal(g1, g0)
  assert torch.equal(out2, out0) and torch.equal(g2, g0)


def test_backward_twice_and_two_calls_give_the_same_bits(den):
  x, r, lens = inputs("ragged")
  xg = x.to(DEV).requires_grad_(True)
  out = den.forward_differentiable(xg, HALF, lengths=lens)
  cot = r.to(DEV)[:, None, :]
  out.backward(cot, retain_graph=True)
  first = xg.grad.clone()
  xg.grad = None
  out.backward(cot)
  torch.cuda.synchronize()
  assert first.any() and torch.equal(xg.grad, first)
  _, again = run(den, x, r, HALF, lens)
  assert torch.equal(again, first.cpu())


def test_bias_is_a_constant_of_the_graph(den):
  """The graph keeps the bias its forward ran with: changing bias_spec in place before the backward changes no bit."""
  x, r, _ = inputs("N1024")
  _, want = run(den, x, r, HALF)
  xg = x.to(DEV).requires_grad_(True)
  out = den.forward_differentiable(xg, HALF)
  keep = den.bias_spec.clone()
  try:
    den.bias_spec.mul_(3.0)
    out.backward(r.to(DEV)[:, None, :])
    torch.cuda.synchronize()
  finally:
    den.bias_spec.copy_(keep)
  assert torch.equal(xg.grad.cpu(), want)


def test_refusals(den):
  x = torch.zeros(2, 2048, device=DEV, requires_grad=True)
  with pytest.raises(_lib.WgError):
    den.forward_differentiable(torch.zeros(2, 2048, requires_grad=True), 0.1)             # a CPU tensor
  with pytest.raises(_lib.WgError):
    den.forward_differentiable(torch.zeros(2, 2048, device=DEV, dtype=torch.float16), 0.1)
  with pytest.raises(_lib.WgError):
    den.forward_differentiable(torch.zeros(2, 1, 2048, device=DEV), 0.1)                  # rank
  for n in (1280 - 1, 768):
    with pytest.raises(_lib.WgError):
      den.forward_differentiable(torch.zeros(2, n, device=DEV, requires_grad=True), 0.1)
    with pytest.raises(_lib.WgError):
      den.forward_differentiable(torch.zeros(2, n, device=DEV), 0.1)
  for bad in ([1024, 1100], [1024, 768], [1024, 2304], [1024], [1024, 1024, 1024], [1024, 1024.0], "ab",
              torch.tensor([1024.0, 1024.0]), torch.tensor([1024, 1024], dtype=torch.int64).to(DEV)):
    with pytest.raises(_lib.WgError):
      den.forward_differentiable(x, 0.1, lengths=bad)
  for s in (float("nan"), float("inf")):
    with pytest.raises(_lib.WgError):
      den.forward_differentiable(x, s)
  assert den.grad_workspace_bytes(2, 1279) == 0 and den.grad_workspace_bytes(2, 768) == 0
  assert den.grad_workspace_bytes(2, 2048) > 0


@pytest.fixture(scope="module")
def c64():
  hp = HParams(n_channels=64, n_layers=4, n_flows=6, n_early_every=2)
  return hp, build_model(hp, synthetic.make_state_dict(hp, seed=5)).requires_grad_(False)


def test_refresh_bias_follows_the_weights(c64):
  _, model = c64
  den = Denoiser(model, TSTFTHParams(), "zeros", DEV)
  stale = den.bias_spec.clone()
  w = dict(model.named_parameters())["WN.0.end.weight"]
  keep = w.detach().clone()
  try:
    with torch.no_grad():
      w[0, 0, 0] += 0.5
    fresh = Denoiser(model, TSTFTHParams(), "zeros", DEV).bias_spec
    assert torch.equal(den.bias_spec, stale) and not torch.equal(stale, fresh)       # before: the stale one
    ptr = den.bias_spec.data_ptr()
    got = den.refresh_bias(model)
    assert got is den.bias_spec and den.bias_spec.data_ptr() == ptr                  # in place
    assert torch.equal(den.bias_spec, fresh)
  finally:
    with torch.no_grad():
      w.copy_(keep)
  assert torch.equal(den.refresh_bias(model, "zeros"), stale)


def test_end_to_end_mel_gradient_through_the_denoiser(c64):
  """infer_differentiable(frames=) -> forward_differentiable(lengths=) -> a loss: mel.grad is finite, non-zero in front of
  every frame count and exactly 0 behind it."""
  hp, model = c64
  den = Denoiser(model, TSTFTHParams(), "zeros", DEV)
  T = [5, 9, 4]
  mel = synthetic.make_mel(len(T), max(T), seed=7).to(DEV).requires_grad_(True)
  audio = model.infer_differentiable(mel, sigma=0.6, frames=T)
  out = den.forward_differentiable(audio, 0.1, lengths=[256 * t for t in T])[:, 0]
  assert out.shape == (len(T), 256 * max(T))
  out.square().mean().backward()
  torch.cuda.synchronize()
  g = mel.grad
  assert g is not None and torch.isfinite(g).all()
  for b, t in enumerate(T):
    assert g[b, :, :t].any() and not g[b, :, t:].any(), b
    assert not out[b, 256 * t:].any()
