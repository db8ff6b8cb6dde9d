"""GPU: ``MultiResolutionSTFTLoss`` -- multi-resolution STFT loss with HIP forward and backward.

Yardstick: ``loss_ref64`` of tests/test_stft_loss_cpu.py (``torch.stft`` in fp64 on the CPU).  Bounds:
  values      relative error <= max(4 e32, 1e-6) and <= 1e-5, e32 the error of the fp32 unfold + matmul restatement on
              the CPU for the same input (an MFMA chain adds up to 2048 terms in sequence where the CPU GEMM blocks K)
  SC and log-magnitude gradients   relative L2 per utterance <= 1e-4 (GRAD_TOL of tests/test_gpu_mel_grads.py); the
              log-magnitude one only on inputs with no fragile bins
  full loss at the default eps      <g, v> against <g_ref64, v>, relative <= 1e-2
Every test prints what it measured.
"""
import pytest
import torch

from _cases import Case
from test_stft_loss_cpu import (DEFAULT_RES, audio, fragile_bins, grad_ref64, log_mag_inputs, loss_ref64, loss_unfold,
                                rel)
from waveglow_amd._lib import WgError
from waveglow_amd.model import WaveGlow
from waveglow_amd.stft_loss import MultiResolutionSTFTLoss

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
GRAD_TOL = 1e-4
DIR_TOL = 1e-2
SHAPES = [(1, 1025), (2, 2048), (3, 22050), (2, 16000)]


def _crit(res=DEFAULT_RES, **kw):
  return MultiResolutionSTFTLoss(*zip(*res), device=DEV, **kw)


def _inputs(B, N, silent):
  return audio(B, N, 100 + N, silent), audio(B, N, 150 + N, False)


def _check_values(crit, x, y, res, label, **kw):
  """sc, mag and loss of one module against loss_ref64; returns the worst relative error."""
  ref = [float(v) for v in loss_ref64(x, y, res, **kw)]
  e32 = [float(v) for v in loss_unfold(x, y, res, dtype=torch.float32, **kw)]
  with torch.no_grad():
    sc, mag = crit.terms(x.to(DEV), y.to(DEV))
    got = [float(sc), float(mag), float(crit(x.to(DEV), y.to(DEV)))]
  worst = 0.0
  for name, g, r, e in zip(("sc", "mag", "loss"), got, ref, e32):
    if r == 0.0:
      assert g == 0.0
      continue
    err, err32 = abs(g - r) / abs(r), abs(e - r) / abs(r)
    print(f"{label} {name}: {g:.8e} ref {r:.8e} rel err {err:.2e} (CPU fp32 restatement {err32:.2e})")
    assert err <= min(max(4 * err32, 1e-6), 1e-5), (label, name, err, err32)
    worst = max(worst, err)
  return worst


def _grad(crit, x, y):
  xg = x.to(DEV).requires_grad_(True)
  crit(xg, y.to(DEV)).backward()
  assert torch.isfinite(xg.grad).all()
  return xg.grad.cpu()


def _check_l2(crit, x, y, res, label, **kw):
  got, ref = _grad(crit, x, y), grad_ref64(x, y, res, **kw)
  errs = [rel(got[b], ref[b]) for b in range(x.shape[0])]
  print(f"{label}: gradient rel L2 per utterance {', '.join(f'{e:.2e}' for e in errs)}")
  assert max(errs) <= GRAD_TOL
  return max(errs)


@pytest.mark.parametrize("silent", [False, True])
@pytest.mark.parametrize("B,N", SHAPES)
def test_values_match_fp64(B, N, silent):
  """Measured on the MI355X over all shapes, terms and single resolutions: 4.3e-10 .. 2.3e-7 (CPU fp32 restatement
  2.1e-9 .. 3.4e-6, other geometries included)."""
  x, y = _inputs(B, N, silent)
  _check_values(_crit(), x, y, DEFAULT_RES, f"B={B} N={N} silent={silent} all")
  for r in DEFAULT_RES:
    if N > r[0] // 2:
      _check_values(_crit((r,)), x, y, (r,), f"B={B} N={N} silent={silent} {r}")


@pytest.mark.parametrize("silent", [False, True])
@pytest.mark.parametrize("B,N", SHAPES)
def test_sc_gradient_matches_fp64(B, N, silent):
  """Measured on the MI355X: 4.1e-7 .. 6.3e-7 per utterance."""
  x, y = _inputs(B, N, silent)
  _check_l2(_crit(factor_mag=0.0), x, y, DEFAULT_RES, f"SC B={B} N={N} silent={silent}", factor_mag=0.0)


@pytest.mark.parametrize("silent", [False, True])
@pytest.mark.parametrize("B,N", [(1, 1025), (2, 2048), (1, 4096)])
def test_log_magnitude_gradient_matches_fp64(B, N, silent):
  """Measured on the MI355X: 1.6e-6 .. 3.9e-6 per utterance."""
  x, y = log_mag_inputs(B, N, silent)
  bad, total = fragile_bins(x, y, eps=1e-2, tau=1e-5)
  assert bad == 0, f"{bad} of {total} bins are fragile: the inputs do not qualify"
  _check_l2(_crit(factor_sc=0.0, eps=1e-2), x, y, DEFAULT_RES, f"log-mag B={B} N={N} silent={silent}", eps=1e-2,
            factor_sc=0.0)


def _direction(g_ref, seed):
  """A fixed random direction v that is not nearly orthogonal to the reference gradient.  The error of <g, v> is about
  ||g - g_ref|| whatever v is, while |<g_ref, v>| = ||g_ref|| |z| with z ~ N(0, 1), so the relative error of the
  directional derivative is the relative L2 error times kappa = ||g_ref|| / |<g_ref, v>|; a draw with a small |z|
  measures the draw, not the kernel (seen: kappa = 17.8 at 2 x 16 000 with seed 7 + N, where the CPU fp32 restatement
  is off by 5.3e-3 and the second fp64 restatement by 5.4e-4; 0.4 .. 2.4 for the other shapes).  The seeds seed,
  seed + 1000, ... are tried in order and the first with kappa <= 4 (|z| >= 0.25, four draws in five) is used: a
  condition on the inputs, computed from the reference alone, like fragile_bins."""
  for k in range(16):
    v = torch.randn(g_ref.shape, generator=torch.Generator().manual_seed(seed + 1000 * k)).double()
    d = float((g_ref.double() * v).sum())
    kappa = float(g_ref.double().norm()) / abs(d)
    if kappa <= 4.0:
      return v, d, kappa
  raise AssertionError("no well-conditioned direction among 16 seeds")


@pytest.mark.parametrize("silent", [False, True])
@pytest.mark.parametrize("B,N", SHAPES)
def test_full_loss_directional_derivative(B, N, silent):
  """Measured on the MI355X: 7.9e-5 .. 1.3e-3 at kappa 0.4 .. 2.4 (CPU fp32 restatement 1.2e-6 .. 1.7e-3); 2 x 16 000
  dense uses its second seed."""
  x, y = _inputs(B, N, silent)
  got, ref = _grad(_crit(), x, y), grad_ref64(x, y)
  v, r, kappa = _direction(ref, 7 + N)
  a = float((got.double() * v).sum())
  err = abs(a - r) / abs(r)
  print(f"full loss B={B} N={N} silent={silent}: <g, v> = {a:.6e}, fp64 {r:.6e}, rel err {err:.2e}, kappa {kappa:.1f}")
  assert err <= DIR_TOL


def _sine_noise(B, N, seed):
  gen = torch.Generator(device=DEV).manual_seed(seed)
  t = torch.arange(N, device=DEV, dtype=torch.float32) / 22050.0
  f0 = 110.0 + 40.0 * torch.arange(B, device=DEV, dtype=torch.float32)[:, None] + 7.0 * seed
  return 0.25 * torch.sin(2 * torch.pi * f0 * t) + 0.05 * torch.randn(B, N, generator=gen, device=DEV)


def test_full_size():
  """B = 16 x 221 184 (configs[1] audio): values, SC gradient, <g, v> of the full loss, retain_graph, determinism and
  memory.  Measured on the MI355X: values 2.4e-8 .. 5.1e-8 (the CPU fp32 restatement's own norm is off by 1.6e-3
  here, so the floor of 1e-6 is what binds), SC gradient 1.3e-6, <g, v> 2.9e-3 at kappa 1.2, peak memory growth
  648.0 MiB against a workspace of 633.6 MiB."""
  B, N = 16, 221184
  x, y = _sine_noise(B, N, 3), _sine_noise(B, N, 4)
  xc, yc = x.cpu(), y.cpu()
  crit = _crit()
  _check_values(crit, xc, yc, DEFAULT_RES, "full size")

  sc_crit = _crit(factor_mag=0.0)
  xg = x.clone().requires_grad_(True)
  sc_crit(xg, y).backward()
  ref = grad_ref64(xc, yc, factor_mag=0.0)
  errs = [rel(xg.grad[b].cpu(), ref[b]) for b in range(B)]
  print(f"full size SC gradient rel L2 per utterance: max {max(errs):.2e}")
  assert max(errs) <= GRAD_TOL
  del sc_crit, ref

  xg = x.clone().requires_grad_(True)
  torch.cuda.synchronize()
  torch.cuda.reset_peak_memory_stats()
  before = torch.cuda.memory_allocated()
  loss = crit(xg, y)
  (g1,) = torch.autograd.grad(loss, xg, retain_graph=True)
  torch.cuda.synchronize()
  grown = torch.cuda.max_memory_allocated() - before
  budget = crit.workspace_bytes(B, N) + g1.numel() * 4 + 64 * 2 ** 20
  print(f"full size: peak memory growth {grown / 2 ** 20:.1f} MiB, workspace {crit.workspace_bytes(B, N) / 2 ** 20:.1f} MiB")
  assert grown <= budget
  (g2,) = torch.autograd.grad(loss, xg)
  assert torch.equal(g1, g2)
  loss2 = crit(x.clone().requires_grad_(True), y)
  assert torch.equal(loss.detach(), loss2.detach())
  v, r, kappa = _direction(grad_ref64(xc, yc), 9)
  a = float((g1.cpu().double() * v).sum())
  err = abs(a - r) / abs(r)
  print(f"full size: <g, v> = {a:.6e}, fp64 {r:.6e}, rel err {err:.2e}, kappa {kappa:.1f}")
  assert err <= DIR_TOL


@pytest.mark.parametrize("res", [((1024, 256, 1024), (512, 50, 240)), ((2048, 2048, 2048),)])
def test_dividing_and_non_dividing_hops(res):
  """Measured on the MI355X: values 2.6e-9 .. 6.3e-8, SC gradient 6.3e-7 .. 1.6e-6."""
  for silent in (False, True):
    x, y = _inputs(2, 16000, silent)
    _check_values(_crit(res), x, y, res, f"{res} silent={silent}")
    _check_l2(_crit(res, factor_mag=0.0), x, y, res, f"SC {res} silent={silent}", factor_mag=0.0)


def test_odd_geometries():
  """Smallest and awkward sizes the docstring promises: n_fft = 32 and 96, hop = 1, win = 1 and odd.
  Measured on the MI355X: values 2.6e-8 .. 1.2e-7, SC gradient 4.6e-7 .. 6.4e-7."""
  res = ((32, 1, 32), (96, 7, 33), (2048, 2047, 1), (160, 160, 159))
  x, y = _inputs(2, 2048, True)
  _check_values(_crit(res), x, y, res, f"{res}")
  _check_l2(_crit(res, factor_mag=0.0), x, y, res, f"SC {res}", factor_mag=0.0)


def test_loss_through_frozen_vocoder():
  """crit(vocoder(mel), target) on the c64 case: d mel through the library's loss against the same loss written with
  pad + unfold + matmul in torch on the GPU (factor_mag = 0; bound 1e-3 as the mel-cycle test).  With the default
  factors: runs, gradient finite.  Measured on the MI355X: 3.0e-4."""
  c = Case("c64")
  model = WaveGlow.remove_weightnorm(WaveGlow(c.hp))
  model.load_state_dict(c.sd)
  model = model.to(DEV).eval().requires_grad_(False)
  ze = [c.z_early[k].to(DEV) for k in sorted(c.z_early, reverse=True)]
  n = c.mel.shape[-1] * 256
  target = audio(c.mel.shape[0], n, 5, False).to(DEV) * 0.3

  def leg(loss_fn):
    mel = c.mel.to(DEV).requires_grad_(True)
    out = model.infer_differentiable(mel, c.sigma, z_init=c.z_init.to(DEV), z_early=ze)
    loss_fn(out, target[:, :out.shape[1]]).backward()
    assert bool(model.grad_finite)
    return mel.grad.detach().clone()

  g_lib = leg(_crit(factor_mag=0.0))
  g_ref = leg(lambda a, t: loss_unfold(a, t, DEFAULT_RES, 1e-7, 1.0, 0.0, dtype=torch.float32)[2])
  err = rel(g_lib, g_ref)
  print(f"vocoder: d mel rel L2 (SC only) {err:.2e}")
  assert torch.isfinite(g_lib).all() and err <= 1e-3
  g_full = leg(_crit())
  assert torch.isfinite(g_full).all()


def test_no_graph_paths():
  x, y = _inputs(2, 16000, True)
  x, y = x.to(DEV), y.to(DEV)
  crit = _crit()
  xg = x.clone().requires_grad_(True)
  with_graph = crit(xg, y)
  assert with_graph.grad_fn is not None and with_graph.dim() == 0 and with_graph.dtype == torch.float32
  sc, mag = crit.terms(xg, y)
  assert sc.grad_fn is not None and mag.grad_fn is not None
  with torch.no_grad():
    plain = crit(xg, y)
  assert plain.grad_fn is None and not plain.requires_grad and torch.equal(plain, with_graph.detach())
  plain = crit(x, y)
  assert plain.grad_fn is None and torch.equal(plain, with_graph.detach())
  psc, pmag = crit.terms(x, y)
  assert torch.equal(psc, sc.detach()) and torch.equal(pmag, mag.detach())
  # the two terms carry their own graphs: d (sc + mag) = d loss at unit factors
  (g_terms,) = torch.autograd.grad(sc + mag, xg)
  (g_loss,) = torch.autograd.grad(with_graph, xg)
  assert torch.equal(g_terms, g_loss)
  # a target that is a non-leaf without grad never receives one
  t = y.clone()
  crit(x.clone().requires_grad_(True), t).backward()
  assert t.grad is None


def test_errors():
  crit = _crit()
  x, y = _inputs(1, 4096, False)
  with pytest.raises(WgError):
    crit(x.requires_grad_(True), y.to(DEV))                                   # CPU tensor
  x = x.detach().to(DEV)
  y = y.to(DEV)
  with pytest.raises(WgError):
    crit(x.half(), y.half())                                                  # fp16
  with pytest.raises(WgError):
    crit(x, torch.zeros(1, 4097, device=DEV))                                 # [B, N] vs [B, N + 1]
  with pytest.raises(WgError):
    crit(torch.zeros(1, 1024, device=DEV), torch.zeros(1, 1024, device=DEV))  # N = max n_fft / 2
  with pytest.raises(WgError):
    crit(x, y.clone().requires_grad_(True))                                   # target.requires_grad
  with pytest.raises(WgError):
    MultiResolutionSTFTLoss((1000,), (100,), (600,), device=DEV)              # n_fft % 32 != 0
  with pytest.raises(WgError):
    MultiResolutionSTFTLoss((1024,) * 9, (120,) * 9, (600,) * 9, device=DEV)
  with pytest.raises(WgError):
    MultiResolutionSTFTLoss(device="cpu")
  assert crit.workspace_bytes(1, 1024) == 0 and crit.workspace_bytes(1, 4096) > 0


def test_non_default_stream():
  x, y = _inputs(2, 16000, True)
  x, y = x.to(DEV), y.to(DEV)
  crit = _crit()
  xg = x.clone().requires_grad_(True)
  loss = crit(xg, y)
  loss.backward()
  torch.cuda.synchronize()
  s = torch.cuda.Stream(device=DEV)
  xs = x.clone().requires_grad_(True)
  torch.cuda.synchronize()
  with torch.cuda.stream(s):
    loss_s = crit(xs, y)
    loss_s.backward()
  s.synchronize()
  assert torch.equal(loss_s.detach(), loss.detach()) and torch.equal(xs.grad, xg.grad)
