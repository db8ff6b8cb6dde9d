"""GPU: per-cell and per-sample bounds for ``MultiScaleMelLoss`` and ``MultiResolutionSTFTLoss`` at the seams of the
conv-STFT core (tests/_loss_cells.py has the statistics, the cases and the yardsticks; tests/test_loss_cells_cpu.py their
CPU side).

The transform rows and the linear mels are read from the ``spectra`` and ``mels`` buffers of the C ABI, at the layouts
include/waveglow_amd.h documents.  Bounds: ``BOUND_FACTOR`` (4) times the yardstick Y of the quantity, and for every
transform cell the derived cap; the per-utterance L2 bound of the local differences is the one of
tests/test_gpu_mel_loss.py.  Every test prints what it measured next to its yardstick.
"""
import ctypes as C
import functools

import pytest
import torch

import _dirty as D
import _loss_cells as L
import _mel_loss_oracle as O
from test_gpu_mel_loss import GRAD_TOL
from waveglow_amd.mel_loss import MultiScaleMelLoss
from waveglow_amd.stft_loss import MultiResolutionSTFTLoss

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
F4 = L.BOUND_FACTOR
PLANE_CASES = list(L.CASES)
LOCAL = [(n, w) for n in L.SINGLE for w in L.case(n).intervals()]


@functools.lru_cache(maxsize=None)
def _mel_crit(name):
  c = L.case(name)
  return MultiScaleMelLoss(O.SR, *zip(*c.scales), device=DEV, mel_bases=[W.numpy() for W in c.banks()])


@functools.lru_cache(maxsize=None)
def _stft_crit(name, term):
  fs, fm, eps = L.STFT_TERMS[term]
  return MultiResolutionSTFTLoss(*zip(*L.case(name).res), factor_sc=fs, factor_mag=fm, eps=eps, device=DEV)


def _filled(n, pattern):
  """n floats on the device whose bytes are all ``pattern``."""
  t = torch.empty(n, dtype=torch.float32, device=DEV)
  D.raw(t).fill_(pattern)
  return t


def _forward(crit, scales, x, y, lengths, pattern=D.FINITE):
  """wg_melloss_forward at unit factors with caller-owned buffers that start from ``pattern``: (out3, spectra, mels, lens)."""
  B, N = x.shape
  spec, mel, tail, ns, nm = L.layout(scales, B, N)
  assert crit.lib.wg_melloss_spectra_elems(crit._h, B, N) == ns and crit.lib.wg_melloss_mels_elems(crit._h, B, N) == nm
  xd, yd = x.to(DEV).contiguous(), y.to(DEV).contiguous()
  ld = None if lengths is None else torch.tensor(lengths, dtype=torch.int32).to(DEV)
  out = torch.empty(3, dtype=torch.float32, device=DEV)
  spectra, mels = _filled(ns, pattern), _filled(nm, pattern)
  stream = C.c_void_p(torch.cuda.current_stream(DEV).cuda_stream)
  assert crit.lib.wg_melloss_forward(crit._h, xd.data_ptr(), yd.data_ptr(), None if ld is None else ld.data_ptr(), 1.0, 1.0,
                                     out.data_ptr(), spectra.data_ptr(), mels.data_ptr(), B, N, stream) == 0
  torch.cuda.synchronize()
  return out, spectra, mels, ld


def _backward(crit, spectra, mels, ld, B, N):
  gx = torch.full((B, N), float("nan"), device=DEV)
  g3 = torch.tensor([0.0, 0.0, 1.0], device=DEV)
  stream = C.c_void_p(torch.cuda.current_stream(DEV).cuda_stream)
  assert crit.lib.wg_melloss_backward(crit._h, g3.data_ptr(), None if ld is None else ld.data_ptr(), 1.0, 1.0,
                                      spectra.data_ptr(), mels.data_ptr(), gx.data_ptr(), B, N, stream) == 0
  torch.cuda.synchronize()
  return gx


@functools.lru_cache(maxsize=None)
def _planes(name, swap):
  """(spectra, mels) on the CPU of the case's plane inputs, with audio and target exchanged under ``swap`` (the buffer holds
  the prediction's transform only)."""
  c = L.case(name)
  x, y = c.plane_inputs()
  if swap:
    x, y = y, x
  _, spectra, mels, _ = _forward(_mel_crit(name), c.scales, x, y, c.lengths)
  return spectra.cpu(), mels.cpu()


def _bin_stat(rows, ref, cap):
  """Device rows [n_fft, F_b] per utterance, de-interleaved as the header says, against (a)'s (re, im): the worst cell as
  (e, (utterance, row, frame, ...)), and the largest |got - ref| / cap over the cells."""
  n_fft = rows[0].shape[0]
  K = n_fft // 2 + 1
  held = torch.ones(2 * K, dtype=torch.bool)                # the imaginary parts of bins 0 and n_fft / 2 have no row
  held[K] = held[2 * K - 1] = False
  got = [torch.cat(L.deinterleave(r))[held] for r in rows]
  want = [torch.cat(r)[held] for r in ref]
  caps = [torch.cat(L.deinterleave(k))[held] for k in cap]
  e, (b, i, f, end, seam) = L.cell_stat(got, want)
  part, k = divmod(int(torch.nonzero(held).flatten()[i]), K)
  use = max(float(((g - w).abs() / k_.clamp_min(1e-300)).max()) for g, w, k_ in zip(got, want, caps))
  return e, (b, L.row_of(part, k, n_fft), f, end, seam), use


@pytest.mark.parametrize("swap", [False, True], ids=["prediction", "target"])
@pytest.mark.parametrize("name", PLANE_CASES)
def test_transform_cells(name, swap):
  """Every cell of the transform of every case, the target's through a second call with audio and target exchanged.
  Measured on the MI355X: 1.0e-6 .. 1.1e-5 of the plane's RMS, 0.57 .. 2.66 Y (the largest at g1024) and at most 0.13 of the
  cap.  g2048 takes its Y from restatement (c): the device is at 9.9e-6 / 1.1e-5 (prediction / target) against a Y of (b)
  of 2.5e-6 (3.94 / 4.46 Y) and a Y of (c) of 1.41e-5 (0.70 / 0.79 Y) -- its chain of 1024 pairs of products, which the CPU
  GEMM of (b) blocks.  At g32 and g288 the device's worst cell is (c)'s, to the last digit printed."""
  c = L.case(name)
  spectra, _ = _planes(name, swap)
  spec, _, _, _, _ = L.layout(c.scales, c.B, c.N)
  for i, (s, (at, shape)) in enumerate(zip(c.scales, spec)):
    rows = L.crop_planes(L.block(spectra, at, shape), c.Fb(i))
    e, pos, use = _bin_stat(rows, L.ref_spec(name, i, swap), L.ref_cap(name, i, swap))
    y, yb, yc = L.yard_rows(name, i), L.yard_rows(name, i, "b"), L.yard_rows(name, i, "c")
    print(f"{name} {s} {'target' if swap else 'prediction'}: worst cell {e:.3e}, Y {y:.3e} (ratio {e / y:.2f}; Y of (b) {yb:.3e}, "
          f"of (c) {yc:.3e}), {use:.4f} of the cap, at {L.describe_cell(pos, L.geometry(s)['MTf'])}")
    assert use <= 1.0, (name, i, use)
    assert e <= F4 * y, (name, i, e, y, pos)


@pytest.mark.parametrize("name", PLANE_CASES)
def test_mel_cells(name):
  """The prediction's and the target's linear mels per cell against W M of (a) -- the Slaney banks, the bank with empty
  rows and the dense bank -- and the fp64 cell counts behind the last scale, exact.  Measured on the MI355X: 4.3e-7 .. 5.5e-6
  of the plane's RMS, 0.46 .. 4.09 Y of (b).  The largest is g2048 (5.5e-6 against a Y of (b) of 1.34e-6), which inherits the
  transform's longer chain and therefore takes its Y from (c)'s transform (6.3e-6: 0.87 Y, the target's mels 0.95 Y)."""
  c = L.case(name)
  _, mels = _planes(name, False)
  _, mel, tail, _, _ = L.layout(c.scales, c.B, c.N)
  for i, (s, (ax, ay, shape)) in enumerate(zip(c.scales, mel)):
    y = L.yard_mels(name, i)
    for at, swap in ((ax, False), (ay, True)):
      e, pos = L.cell_stat(L.crop_planes(L.block(mels, at, shape), c.Fb(i)), L.ref_mels(name, i, swap))
      print(f"{name} {s} {'target' if swap else 'prediction'}: worst mel cell {e:.3e}, Y {y:.3e} (ratio {e / y:.2f}; Y of (b) "
            f"{L.yard_mels(name, i, 'b'):.3e}, from (c)'s transform {L.yard_mels(name, i, 'c'):.3e}) at {L.describe_cell(pos)}")
      assert e <= F4 * y, (name, i, swap, e, y, pos)
  counts = mels[tail:tail + 16].view(torch.float64)
  want = [float(s[3] * sum(c.Fb(i))) for i, s in enumerate(c.scales)] + [0.0] * (8 - len(c.scales))
  assert counts.tolist() == want, (counts.tolist(), want)


@pytest.mark.parametrize("pattern", [D.ONES, D.FINITE])
@pytest.mark.parametrize("name", ["g64", "g64r", "g544r", "multi", "full64"])
def test_untouched_columns(name, pattern):
  """Columns f >= F_b and every float of block padding keep the bytes they held, every cell f < F_b is written, and the
  backward leaves both buffers byte-identical."""
  c = L.case(name)
  x, y = c.plane_inputs()
  crit = _mel_crit(name)
  out, spectra, mels, ld = _forward(crit, c.scales, x, y, c.lengths, pattern)
  ms, mm = L.written_mask(c.scales, c.B, c.N, c.lens)
  word = _filled(1, pattern).view(torch.int32).item()
  for what, buf, mask in (("spectra", spectra, ms), ("mels", mels, mm)):
    same = buf.cpu().view(torch.int32) == word
    assert bool(same[~mask].all()), f"{what}: {int((~same[~mask]).sum())} floats outside the written cells changed"
    assert not bool(same[mask].any()), f"{what}: {int(same[mask].sum())} cells were not written"
    assert int((~mask).sum()) > 0 or name == "full64" and what == "spectra"
  assert torch.isfinite(out).all()
  before = spectra.clone(), mels.clone()
  gx = _backward(crit, spectra, mels, ld, c.B, c.N)
  D.same_bytes(spectra, before[0], "spectra after the backward")
  D.same_bytes(mels, before[1], "mels after the backward")
  assert torch.isfinite(gx).all()
  for b, n in enumerate(c.lens):
    assert gx[b, :n].any() and not gx[b, n:].any()


def _device_grad(name, loss, term, x, y):
  c = L.case(name)
  if loss == "mel":
    crit = _mel_crit(name)
    crit.factor_log, crit.factor_lin = L.MEL_TERMS[term]
  else:
    crit = _stft_crit(name, term)
  xg = x.to(DEV).requires_grad_(True)
  crit(xg, y.to(DEV), lengths=c.lengths).backward()
  return xg.grad.cpu()


WHOLE = [(n, loss, t) for n in L.SINGLE for loss, terms in (("mel", L.MEL_TERMS), ("stft", L.STFT_TERMS)) for t in terms] + \
        [("multi", "mel", "both")]


@pytest.mark.parametrize("name,loss,term", WHOLE)
def test_gradient_per_sample(name, loss, term):
  """The whole-signal gradient of both losses per sample, on inputs without fragile cells or bins
  (tests/test_loss_cells_cpu.py); exact zeros behind a length.  Measured on the MI355X, worst sample (in Y): mel log
  1.6e-6 .. 3.6e-4 (0.07 .. 1.33), lin 4.7e-7 .. 8.7e-6 (0.43 .. 1.92), both 9.2e-7 .. 3.4e-4 (0.06 .. 1.36); STFT loss
  spectral convergence 7.7e-7 .. 7.7e-6 (0.55 .. 2.81), log-magnitude at eps 1e-2 1.0e-6 .. 1.3e-4 (0.22 .. 1.91)."""
  c = L.case(name)
  x, y = c.inputs()
  got, ref = _device_grad(name, loss, term, x, y), L.ref_grad(name, loss, term)
  e, pos = L.sample_stat(got, ref, c.lens, c.scales[0][1])
  yard = L.yard_grad(name, loss, term)
  print(f"{name} {loss} {term}: worst sample {e:.3e}, Y {yard:.3e} (ratio {e / yard:.2f}) at {L.describe_sample(pos)}")
  assert e <= F4 * yard, (e, yard, pos)
  for b, n in enumerate(c.lens):
    assert not got[b, n:].any(), b


@pytest.mark.parametrize("loss,term", L.LOCAL_TERMS)
@pytest.mark.parametrize("name,where", LOCAL)
def test_gradient_of_a_local_difference(name, where, loss, term):
  """The target equals the prediction except on a short interval at an utterance's first or last samples or across a frame
  tile seam: the gradient is made of the frames that touch the interval alone.  Per sample over the support, exact zeros
  outside it, and the per-utterance L2 bound of the existing tests.  Measured on the MI355X over the 32 cases of each loss,
  exact zeros outside the support in all of them: mel loss, worst sample 4.3e-7 .. 1.8e-4 of the support's RMS
  (0.08 .. 1.76 Y), per-utterance L2 1.4e-7 .. 5.4e-5; STFT loss (spectral convergence) 8.8e-7 .. 1.7e-5 (0.43 .. 2.75 Y),
  L2 2.4e-7 .. 2.4e-6.  While ``wgsc::power`` was contracted to an fma in the target's forward kernel alone, the STFT loss left
  1e-11 .. 6e-9 on nearly every sample outside the support (g32, first interval: 1 975 samples, 6.4e-9 at most against 4.2e-2
  inside)."""
  c = L.case(name)
  x, y = c.local_inputs(where)
  got, ref = _device_grad(name, loss, term, x, y), L.ref_grad(name, loss, term, where)
  sup = c.support(where)
  e, pos = L.sample_stat(got, ref, c.lens, c.scales[0][1])
  yard = L.yard_grad(name, loss, term, where)
  l2, g32 = L.l2_per_utterance(got, ref, c.lens), L.l2_b32(name, loss, term, where)
  print(f"{name} {where} {loss}: worst sample {e:.3e}, Y {yard:.3e} (ratio {e / yard:.2f}) at {L.describe_sample(pos)}; "
        f"rel L2 per utterance {l2} (CPU fp32 restatement {g32})")
  assert e <= F4 * yard, (e, yard, pos)
  for b, (err, err32) in enumerate(zip(l2, g32)):
    if err32 is not None:
      assert err <= max(F4 * err32, L.L2_FLOOR) and err <= GRAD_TOL, (b, err, err32)
  out = got[~sup]
  assert not out.any(), (f"{int((out != 0).sum())} non-zero samples outside the support, largest {float(out.abs().max()):.2e} "
                         f"against {float(got[sup].abs().max()):.2e} inside")


def test_instances_agree():
  """The arithmetic of a tile depends neither on the module's other scales nor on the batch the utterance is in: g64's scale
  alone and as the first of three scales gives the same spectra bytes, and an utterance's cells are the same bytes at B = 1
  and in its row of a batch of 3, dense and ragged."""
  c, m = L.case("g64r"), L.case("multi")
  x, y = c.plane_inputs()
  alone = _mel_crit("g64")
  spec = L.layout(c.scales, c.B, c.N)
  n0, shape = spec[3], spec[0][0][1]
  _, sp1, _, _ = _forward(alone, c.scales, x, y, None)
  _, sp3, _, _ = _forward(_mel_crit("multi"), m.scales, x, y, None)
  D.same_bytes(sp1, sp3[:n0], "g64 alone against the first of three scales")
  for lengths in (None, c.lengths):
    if lengths is not None:
      _, sp1, _, _ = _forward(alone, c.scales, x, y, lengths)
    batch = L.block(sp1, 0, shape)
    for b in range(c.B):
      n = c.N if lengths is None else lengths[b]
      _, one, _, _ = _forward(alone, c.scales, x[b:b + 1], y[b:b + 1], None if lengths is None else [n])
      Fb = L.frames_of(n, c.scales[0][1])
      D.same_bytes(L.block(one, 0, (1,) + shape[1:])[0, :, :Fb].contiguous(), batch[b, :, :Fb].contiguous(),
                   f"utterance {b} at B = 1 against its row of the batch, lengths {lengths}")


@pytest.mark.parametrize("name", ["g64", "g544r", "g2048"])
def test_equal_signals_give_exact_zeros_in_the_stft_loss(name):
  """A target equal to the prediction: the two forward kernels of the STFT loss form M(y) and M(x) from equal (re, im), so
  M(y) - M(x) and log M(y) - log M(x) are exact zeros in every bin and both terms are exactly 0 (``wgsc::power`` keeps one
  rounding per operation in every kernel; while the target's kernel alone contracted it to an fma, they were not)."""
  c = L.case(name)
  x = c.plane_inputs()[0].to(DEV)
  for term in L.STFT_TERMS:
    crit = _stft_crit(name, term)
    xg = x.clone().requires_grad_(True)
    sc, mag = crit.terms(xg, x.clone(), lengths=c.lengths)
    print(f"{name} {term}: sc {float(sc):.3e}, mag {float(mag):.3e}")
    assert float(sc) == 0.0 and float(mag) == 0.0
    (sc + mag).backward()
    assert torch.isfinite(xg.grad).all()
