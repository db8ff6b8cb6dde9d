"""GPU: per-utterance lengths for the waveform losses -- ``MultiResolutionSTFTLoss(audio, target, lengths=...)`` and
``TacotronSTFT.mel_spectrogram_differentiable(y, lengths=...)``.

Exact bits, no tolerance: equal lengths against the dense call, NaN behind the lengths, repeated calls and a second
backward under retain_graph, the mel forward against ``mel_spectrogram_ragged_device`` and the mel backward against the
dense backward of every crop.
Against the fp64 crop reference of tests/_ragged_ref.py, with the bounds of tests/test_gpu_stft_loss.py: values
``min(max(4 e32, 1e-6), 1e-5)``, SC gradient relative L2 per utterance over its valid samples ``1e-4``, directional
derivative of the full loss ``1e-2`` with the ``_direction`` recipe.
A single utterance on a longer pitch against the dense call on its crop: the same partial sums added in another order
in fp64 and rounded once, so out3 within one fp32 ulp; the two gradient coefficients then differ by at most one ulp
(2^-24 = 6e-8 relative each, 1.2e-7 together in the worst case), bound 1e-6 relative L2.
Every test prints what it measured.
"""
import ctypes as C

import numpy as np
import pytest
import torch

from _ragged_ref import CASE_IDS, CASES, inputs, ragged_grad64, ragged_ref64, ragged_unfold
from test_gpu_stft_loss import DIR_TOL, GRAD_TOL, _direction
from test_stft_loss_cpu import DEFAULT_RES, audio, rel
from waveglow_amd._lib import WgError
from waveglow_amd.stft_loss import MultiResolutionSTFTLoss
from waveglow_amd.taco_stft import TacotronSTFT, TSTFTHParams

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
NAN = float("nan")
both_inputs = pytest.mark.parametrize("silent", [False, True])
all_cases = pytest.mark.parametrize("res,N,lens", CASES, ids=CASE_IDS)


def _crit(res=DEFAULT_RES, **kw):
  return MultiResolutionSTFTLoss(*zip(*res), device=DEV, **kw)


def _run(crit, x, y, lengths, g3=None):
  """(out3, audio.grad) of one forward + backward on the device; g3 weighs (sc, mag, loss), default the loss alone."""
  xg = x.detach().clone().requires_grad_(True)
  sc, mag = crit.terms(xg, y, lengths) if lengths is not None else crit.terms(xg, y)
  loss = crit(xg, y, lengths) if lengths is not None else crit(xg, y)
  out3 = torch.stack([sc, mag, loss]).detach()
  total = loss if g3 is None else g3[0] * sc + g3[1] * mag + g3[2] * loss
  total.backward()
  return out3, xg.grad


@both_inputs
@all_cases
def test_equal_lengths_give_the_dense_bits(res, N, lens, silent):
  x, y = (t.to(DEV) for t in inputs(N, lens, silent))
  crit = _crit(res)
  B = len(lens)
  for g3 in (None, (0.3, -1.7, 0.9)):
    out_d, g_d = _run(crit, x, y, None, g3)
    for lengths in ([N] * B, tuple([N] * B), torch.tensor([N] * B)):
      out_r, g_r = _run(crit, x, y, lengths, g3)
      assert torch.equal(out_r, out_d) and torch.equal(g_r, g_d)
  with torch.no_grad():
    assert torch.equal(crit(x, y, [N] * B), crit(x, y))
    assert all(torch.equal(a, b) for a, b in zip(crit.terms(x, y, [N] * B), crit.terms(x, y)))


@both_inputs
@all_cases
def test_nan_behind_the_lengths_changes_no_bit(res, N, lens, silent):
  x, y = (t.to(DEV) for t in inputs(N, lens, silent))
  crit = _crit(res)
  out, g = _run(crit, x, y, list(lens))
  xn, yn = x.clone(), y.clone()
  for b, n in enumerate(lens):
    xn[b, n:] = NAN
    yn[b, n:] = NAN
  out_n, g_n = _run(crit, xn, yn, list(lens))
  assert torch.isfinite(out).all() and torch.isfinite(g).all()
  assert torch.equal(out_n, out) and torch.equal(g_n, g)
  for b, n in enumerate(lens):
    assert not g[b, n:].any() and g[b, :n].abs().max() > 0
  with torch.no_grad():
    assert torch.equal(crit(xn, yn, list(lens)), out[2])


@all_cases
def test_repeatable_and_second_backward_under_retain_graph(res, N, lens):
  x, y = (t.to(DEV) for t in inputs(N, lens, True))
  crit = _crit(res)
  xg = x.clone().requires_grad_(True)
  loss = crit(xg, y, list(lens))
  (g1,) = torch.autograd.grad(loss, xg, retain_graph=True)
  other = crit(x.clone().requires_grad_(True), y, [N] * len(lens))      # another call in between, other lengths
  (g2,) = torch.autograd.grad(loss, xg)
  assert torch.equal(g1, g2)
  out, g = _run(crit, x, y, list(lens))
  assert torch.equal(out[2], loss.detach()) and torch.equal(g, g1)
  assert not torch.equal(other.detach(), loss.detach())


@both_inputs
@all_cases
def test_values_match_the_fp64_crop_reference(res, N, lens, silent):
  """Measured on the MI355X: 4.5e-9 .. 7.5e-8 (CPU fp32 restatement 1.4e-9 .. 7.2e-8)."""
  x, y = inputs(N, lens, silent)
  ref = [float(v) for v in ragged_ref64(x, y, lens, res)]
  e32 = [float(v) for v in ragged_unfold(x, y, lens, res, dtype=torch.float32)]
  crit = _crit(res)
  with torch.no_grad():
    sc, mag = crit.terms(x.to(DEV), y.to(DEV), list(lens))
    got = [float(sc), float(mag), float(crit(x.to(DEV), y.to(DEV), list(lens)))]
  for name, g, r, e in zip(("sc", "mag", "loss"), got, ref, e32):
    err, err32 = abs(g - r) / abs(r), abs(e - r) / abs(r)
    print(f"N={N} lens={lens} silent={silent} {name}: {g:.8e} ref {r:.8e} rel err {err:.2e} (CPU fp32 restatement "
          f"{err32:.2e})")
    assert err <= min(max(4 * err32, 1e-6), 1e-5), (name, err, err32)


@both_inputs
@all_cases
def test_sc_gradient_matches_the_fp64_crop_reference(res, N, lens, silent):
  """Measured on the MI355X: 1.4e-7 .. 1.8e-6 per utterance."""
  x, y = inputs(N, lens, silent)
  _, got = _run(_crit(res, factor_mag=0.0), x.to(DEV), y.to(DEV), list(lens))
  got, ref = got.cpu(), ragged_grad64(x, y, lens, res, factor_mag=0.0)
  errs = [rel(got[b, :n], ref[b, :n]) for b, n in enumerate(lens)]
  print(f"SC N={N} lens={lens} silent={silent}: gradient rel L2 per utterance {', '.join(f'{e:.2e}' for e in errs)}")
  assert torch.isfinite(got).all() and max(errs) <= GRAD_TOL
  for b, n in enumerate(lens):
    assert not got[b, n:].any()


@both_inputs
@all_cases
def test_full_loss_directional_derivative(res, N, lens, silent):
  """Measured on the MI355X: 8.3e-6 .. 3.2e-4 at kappa 0.5 .. 3.8."""
  x, y = inputs(N, lens, silent)
  _, got = _run(_crit(res), x.to(DEV), y.to(DEV), list(lens))
  ref = ragged_grad64(x, y, lens, res)
  v, r, kappa = _direction(ref, 7 + N)
  a = float((got.cpu().double() * v).sum())
  err = abs(a - r) / abs(r)
  print(f"full loss N={N} lens={lens} silent={silent}: <g, v> = {a:.6e}, fp64 {r:.6e}, rel err {err:.2e}, "
        f"kappa {kappa:.1f}")
  assert err <= DIR_TOL


@both_inputs
@all_cases
def test_single_utterance_on_a_longer_pitch(res, N, lens, silent):
  """Measured on the MI355X: 0 ulp and a bit-identical gradient in all twelve comparisons."""
  x, y = (t.to(DEV) for t in inputs(N, lens, silent))
  crit = _crit(res)
  for b, n in enumerate(lens):
    if n == N:
      continue
    out_r, g_r = _run(crit, x[b:b + 1], y[b:b + 1], [n])
    out_c, g_c = _run(crit, x[b:b + 1, :n].contiguous(), y[b:b + 1, :n].contiguous(), None)
    a, c = out_r.cpu().numpy(), out_c.cpu().numpy()
    ulps = np.abs(a - c) / np.spacing(np.maximum(np.abs(a), np.abs(c)))
    err = rel(g_r[0, :n], g_c[0])
    print(f"N={N} n={n} silent={silent}: out3 apart by {ulps} ulp, gradient rel L2 {err:.2e}")
    assert (ulps <= 1.0).all() and err <= 1e-6
    assert not g_r[0, n:].any()


def test_lengths_the_library_counts_as_zero():
  """The C ABI below the Python check: a length outside (max n_fft / 2, N] counts as 0 -- a zero gradient row, nothing
  else moves by a bit -- and when every length does, out3 and the gradient are zeros, not NaN."""
  res, N, lens = CASES[0]
  x, y = (t.to(DEV) for t in inputs(N, lens, True))
  crit = _crit(res)
  B = len(lens)
  nbytes = crit.workspace_bytes(B, N)

  def call(lens_host):
    ld = torch.tensor(lens_host, dtype=torch.int32).to(DEV)
    out = torch.full((3,), NAN, device=DEV)
    gx = torch.full((B, N), NAN, device=DEV)
    g3 = torch.tensor([0.0, 0.0, 1.0], device=DEV)
    ws = torch.empty(nbytes, dtype=torch.uint8, device=DEV)
    stream = C.c_void_p(torch.cuda.current_stream(DEV).cuda_stream)
    assert crit.lib.wg_stftloss_forward(crit._h, x.data_ptr(), y.data_ptr(), ld.data_ptr(), 1.0, 1.0, out.data_ptr(), B, N,
                                        1, ws.data_ptr(), nbytes, stream) == 0
    assert crit.lib.wg_stftloss_backward(crit._h, g3.data_ptr(), ld.data_ptr(), 1.0, 1.0, gx.data_ptr(), B, N,
                                         ws.data_ptr(), nbytes, stream) == 0
    return out, gx

  for bad in ([0, 1024, N + 1], [-1, -(2 ** 31), 2 ** 31 - 1]):
    out, gx = call(bad)
    assert not out.any() and not gx.any()
  out, gx = call([lens[0], 1024, lens[2]])
  assert torch.isfinite(out).all() and torch.isfinite(gx).all() and out.abs().min() > 0
  assert not gx[1].any() and gx[0].abs().max() > 0 and gx[2].abs().max() > 0
  keep = [0, 2]
  out2, g2 = _run(crit, x[keep], y[keep], [lens[0], lens[2]])
  ulps = np.abs(out.cpu().numpy() - out2.cpu().numpy()) / np.spacing(np.abs(out2.cpu().numpy()))
  print(f"batch with a refused utterance against the batch without it: out3 apart by {ulps} ulp")
  assert (ulps <= 1.0).all() and rel(gx[keep], g2) <= 1e-6


def test_bad_lengths_raise_before_any_launch():
  crit = _crit()
  x, y = (t.to(DEV) for t in inputs(4099, (1025, 2500, 4099), False))
  for bad in ([1024, 2500, 4099], [1025, 2500, 4100], [1025, 2500], [1025, 2500.0, 4099], torch.tensor([1025, 0, 4099]),
              torch.tensor([1025, 2500, 4099], device=DEV)):
    with pytest.raises(WgError):
      crit(x, y, bad)
    with pytest.raises(WgError):
      crit.terms(x.clone().requires_grad_(True), y, bad)
  taco = TacotronSTFT(TSTFTHParams(), DEV)
  for bad in ([512, 2500, 4099], [1025, 2500, 4100], [1025, 2500]):
    with pytest.raises(WgError):
      taco.mel_spectrogram_differentiable(x, bad)
    with pytest.raises(WgError):
      taco.mel_spectrogram_differentiable(x.clone().requires_grad_(True), bad)


# ---- mel gradients -----------------------------------------------------------------------------------------------------

MEL_N, MEL_LENS = 20000, (513, 8191, 20000, 9000)


@pytest.fixture(scope="module")
def taco():
  return TacotronSTFT(TSTFTHParams(), DEV)


def _mel_inputs(seed=11):
  y = audio(len(MEL_LENS), MEL_N, seed).to(DEV)
  g = torch.randn(len(MEL_LENS), 80, MEL_N // 256 + 1, generator=torch.Generator().manual_seed(seed + 1)).to(DEV)
  return y, g


def _mel_run(taco, y, g, lengths):
  yg = y.detach().clone().requires_grad_(True)
  mel = taco.mel_spectrogram_differentiable(yg, lengths) if lengths is not None else \
      taco.mel_spectrogram_differentiable(yg)
  assert mel.grad_fn is not None
  mel.backward(g)
  return mel.detach(), yg.grad


def test_mel_forward_is_the_ragged_front_end(taco):
  y, _ = _mel_inputs()
  ref, frames, _ = taco.mel_spectrogram_ragged_device(y, list(MEL_LENS))
  assert frames == [n // 256 + 1 for n in MEL_LENS]
  yg = y.clone().requires_grad_(True)
  out = taco.mel_spectrogram_differentiable(yg, list(MEL_LENS))
  assert out.grad_fn is not None and out.shape == (len(MEL_LENS), 80, MEL_N // 256 + 1)
  assert torch.equal(out.detach(), ref)
  for b, f in enumerate(frames):
    assert not out[b, :, f:].any()
  with torch.no_grad():
    plain = taco.mel_spectrogram_differentiable(yg, torch.tensor(MEL_LENS))
  assert plain.grad_fn is None and torch.equal(plain, ref)
  plain = taco.mel_spectrogram_differentiable(y, MEL_LENS)
  assert plain.grad_fn is None and torch.equal(plain, ref)


def test_mel_backward_is_the_dense_backward_of_every_crop(taco):
  y, g = _mel_inputs()
  mel, grad = _mel_run(taco, y, g, list(MEL_LENS))
  assert torch.isfinite(grad).all()
  for b, n in enumerate(MEL_LENS):
    f = n // 256 + 1
    mel_c, grad_c = _mel_run(taco, y[b:b + 1, :n].contiguous(), g[b:b + 1, :, :f].contiguous(), None)
    assert torch.equal(mel[b:b + 1, :, :f], mel_c)
    assert torch.equal(grad[b:b + 1, :n], grad_c) and grad_c.abs().max() > 0
    assert not grad[b, n:].any()
  full = [MEL_N] * len(MEL_LENS)
  mel_f, grad_f = _mel_run(taco, y, g, full)
  mel_d, grad_d = _mel_run(taco, y, g, None)
  assert torch.equal(mel_f, mel_d) and torch.equal(grad_f, grad_d)


def test_mel_nan_behind_the_lengths_changes_no_bit_and_retain_graph(taco):
  y, g = _mel_inputs()
  mel, grad = _mel_run(taco, y, g, list(MEL_LENS))
  yn, gn = y.clone(), g.clone()
  for b, n in enumerate(MEL_LENS):
    yn[b, n:] = NAN
    gn[b, :, n // 256 + 1:] = NAN
  mel_n, grad_n = _mel_run(taco, yn, gn, list(MEL_LENS))
  assert torch.equal(mel_n, mel) and torch.equal(grad_n, grad) and torch.isfinite(grad_n).all()
  yg = yn.clone().requires_grad_(True)
  out = taco.mel_spectrogram_differentiable(yg, list(MEL_LENS))
  (g1,) = torch.autograd.grad(out, yg, gn, retain_graph=True)
  (g2,) = torch.autograd.grad(out, yg, gn)
  assert torch.equal(g1, grad) and torch.equal(g2, grad)


def test_non_default_stream(taco):
  res, N, lens = CASES[0]
  x, y = (t.to(DEV) for t in inputs(N, lens, True))
  crit = _crit(res)
  ym, gm = _mel_inputs()
  out, g = _run(crit, x, y, list(lens))
  mel, grad = _mel_run(taco, ym, gm, list(MEL_LENS))
  torch.cuda.synchronize()
  s = torch.cuda.Stream(device=DEV)
  with torch.cuda.stream(s):
    out_s, g_s = _run(crit, x, y, list(lens))
    mel_s, grad_s = _mel_run(taco, ym, gm, list(MEL_LENS))
  s.synchronize()
  assert torch.equal(out_s, out) and torch.equal(g_s, g)
  assert torch.equal(mel_s, mel) and torch.equal(grad_s, grad)
