"""CPU: the yardsticks of MultiScaleMelLoss (tests/_mel_loss_oracle.py) against each other, and everything of the C ABI and
the Python layer that needs no device: prototypes against the binding, buffer sizes against the documented layouts, and
every refusal.  Finite differences are a yardstick only where the loss is smooth: ``gradcheck`` runs on one small case
away from the kinks."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

import _mel_loss_oracle as O
from waveglow_amd import _lib, build
from waveglow_amd.mel_loss import DAC_N_FFTS, DAC_N_MELS, MultiScaleMelLoss, check_scales

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
TERMS = (dict(factor_log=1.0, factor_lin=0.0), dict(factor_log=0.0, factor_lin=1.0), dict(factor_log=1.0, factor_lin=1.0))


@pytest.mark.parametrize("B,N", O.SHAPES[:3])
def test_two_fp64_restatements_agree(B, N):
  """Values to 1e-8 and gradients to 1e-5 per utterance (measured 3.9e-8 .. 3.4e-6), dense and ragged.  The fp32 rounding
  of the packed basis (2^-24 per entry) is all that separates the two.  It moves (re, im) of a bin by about
  6e-8 * sum |w x| whatever the bin holds, so the direction (re, im) / M that the gradient of M carries moves most where M
  is small -- the frames at the edges of the silent stretch -- and the log term weighs those cells by 1 / mel.  The
  linear term alone agrees to 2e-7."""
  scales = O.scales_for(N)
  x, y = O.inputs(B, N, O.SEEDS[(B, N)])
  for lens in (None, O.RAGGED.get((B, N))):
    a = O.loss_stft(x, y, scales, factor_lin=1.0, lengths=lens)
    b = O.loss_unfold(x, y, scales, factor_lin=1.0, lengths=lens)
    for u, v in zip(a, b):
      assert abs(float(u) - float(v)) <= 1e-8 * abs(float(u)), (lens, float(u), float(v))
    for kw in TERMS:
      ga = O.grad_of(O.loss_stft, x, y, scales, lengths=lens, **kw)
      gb = O.grad_of(O.loss_unfold, x, y, scales, lengths=lens, **kw)
      for bb in range(B):
        n = N if lens is None else lens[bb]
        assert O.rel(gb[bb, :n], ga[bb, :n]) <= 1e-5, (lens, kw, bb)
        assert not ga[bb, n:].any() and not gb[bb, n:].any()


def test_gradcheck_of_the_stft_restatement():
  """(a) against finite differences at the smallest case: one scale of n_fft = 32, 5 mels, 40 samples, both terms."""
  scales = ((32, 8, 32, 5),)
  x, y = O.inputs(1, 40, 3, silent=False)
  assert O.fragile_cells(x, y, scales) == 0
  fn = lambda t: O.loss_stft(t, y, scales, factor_log=1.0, factor_lin=1.0)[2]
  assert torch.autograd.gradcheck(fn, (x.double().requires_grad_(True),), eps=1e-6, atol=1e-7, rtol=1e-5)


def test_conventions_of_the_restatements():
  """sign(0) = 0, nothing under the clamp, and a zero gradient (not NaN) at silent bins, in both restatements."""
  scales = O.scales_for(2048)
  x, y = O.inputs(2, 2048, 1)
  z = torch.zeros_like(x)
  for fn in (O.loss_stft, O.loss_unfold):
    assert not O.grad_of(fn, x, x.clone(), scales, factor_lin=1.0).any()            # equal to the target
    g = O.grad_of(fn, z, y, scales, factor_lin=1.0)                                   # silent prediction
    assert torch.isfinite(g).all() and not g.any()
    g = O.grad_of(fn, x, y, scales, factor_lin=1.0)
    assert torch.isfinite(g).all() and g.abs().max() > 0


@pytest.mark.parametrize("B,N", O.SHAPES)
def test_the_seeds_give_inputs_without_fragile_cells(B, N):
  x, y = O.inputs(B, N, O.SEEDS[(B, N)])
  scales = O.scales_for(N)
  assert O.fragile_cells(x, y, scales) == 0
  if (B, N) in O.RAGGED:
    assert O.fragile_cells(x, y, scales, lengths=O.RAGGED[(B, N)]) == 0


def test_fragile_cells_counts_both_kinds():
  scales = O.scales_for(2048)
  x, y = O.inputs(1, 2048, 0, silent=False)
  cells = sum(s[3] * (2048 // s[1] + 1) for s in scales)
  assert O.fragile_cells(x, x.clone(), scales) == cells                               # every log difference is 0
  assert O.fragile_cells(torch.zeros(1, 2048), y, scales) == 0                         # all under the clamp, none near it
  # a prediction scaled so that one cell's mel lies on the clamp
  s = ((64, 16, 64, 10),)
  m = O.mels(O.mag_stft, x, s[0], O.bank(s[0]), None, torch.float64)
  assert O.fragile_cells(x * (O.CLAMP / float(m[3, 7])), y, s) >= 1


def test_ragged_lengths_cover_the_three_kinds():
  for (B, N), lens in O.RAGGED.items():
    scales = O.scales_for(N)
    need = max(s[0] for s in scales) // 2
    assert len(lens) == B and min(lens) == need + 1 and max(lens) == N
    assert any(all(n % s[1] for s in scales) for n in lens)
    assert set(scales) == set(O.SCALES)


def test_a_scale_with_empty_rows_has_them():
  W = O.bank(O.EMPTY_ROWS)
  assert int((W.abs().sum(1) == 0).sum()) >= 1
  for s in O.SCALES:
    assert int((O.bank(s).abs().sum(1) == 0).sum()) == 0


# ---- the C ABI without a device

@pytest.fixture(scope="module")
def lib():
  build.build_library()
  return _lib.load()


def _prototypes():
  text = open(os.path.join(ROOT, "include", "waveglow_amd.h")).read()
  text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
  return {n: (ret.strip(), [a.strip() for a in args.split(",")])
          for ret, n, args in re.findall(r"\b(int|size_t)\s+(wg_melloss_[a-z_]+)\s*\(([^;{}]*?)\)\s*;", text, flags=re.S)}


def test_prototypes_match_the_binding_argument_by_argument():
  protos = _prototypes()
  assert sorted(protos) == sorted(n for n in _lib.SIGNATURES if n.startswith("wg_melloss_")) and len(protos) == 6
  scalar = {"int32_t": C.c_int32, "float": C.c_float, "size_t": C.c_size_t, "int": C.c_int}
  for name, (ret, args) in protos.items():
    restype, argtypes = _lib.SIGNATURES[name]
    assert restype is scalar[ret], name
    assert len(args) == len(argtypes), name
    for decl, ct in zip(args, argtypes):
      if "*" in decl:
        assert ct is C.c_void_p or issubclass(ct, C._Pointer), (name, decl)
        if issubclass(ct, C._Pointer) and ct._type_ is C.c_int32:
          assert "int32_t" in decl, (name, decl)
      else:
        assert ct is scalar[decl.split()[0]], (name, decl)
  # no workspace or saved argument: the table of tests/_dirty.py does not list these calls, the new GPU test file covers them
  for name, (_, args) in protos.items():
    assert not [a for a in args if re.search(r"\bvoid\s*\*\s*(workspace|saved)\b", a)], name


def _create(lib, scales, clamp=1e-5, n=None):
  n = len(scales) if n is None else n
  cols = list(zip(*scales)) if scales else [(), (), (), ()]
  arr = lambda v: (C.c_int32 * max(len(v), 1))(*v)
  h = C.c_void_p()
  rc = lib.wg_melloss_create(n, arr(cols[0]), arr(cols[1]), arr(cols[2]), arr(cols[3]), None, None, clamp, -1, C.byref(h))
  return rc, h


def _up64(n):
  return (n + 63) // 64 * 64


def test_planning_handle_sizes_are_the_documented_layouts(lib):
  dac = tuple(zip(DAC_N_FFTS, (n // 4 for n in DAC_N_FFTS), DAC_N_FFTS, DAC_N_MELS))
  for scales in (O.SCALES, dac, ((512, 120, 400, 64),)):
    rc, h = _create(lib, scales)
    assert rc == 0
    for B, N in ((1, 1025), (2, 2048), (3, 16000), (16, 221184)):
      spectra = mels = 0
      for n_fft, hop, _, n_mels in scales:
        Fp = _up64(N // hop + 1)
        spectra += _up64(B * n_fft * Fp)
        mels += 2 * _up64(B * n_mels * Fp)
      mels += 64
      assert lib.wg_melloss_spectra_elems(h, B, N) == spectra, (scales, B, N)
      assert lib.wg_melloss_mels_elems(h, B, N) == mels, (scales, B, N)
    need = max(s[0] for s in scales) // 2
    for B, N in ((1, need), (0, 4096), (-1, 4096), (65536, 4096), (1, 0)):
      assert lib.wg_melloss_spectra_elems(h, B, N) == 0 and lib.wg_melloss_mels_elems(h, B, N) == 0, (B, N)
    assert lib.wg_melloss_spectra_elems(h, 1, need + 1) > 0
    assert lib.wg_melloss_destroy(h) == 0
  assert lib.wg_melloss_spectra_elems(None, 1, 4096) == 0 and lib.wg_melloss_mels_elems(None, 1, 4096) == 0


def test_every_invalid_argument_is_refused_on_a_planning_handle(lib):
  ok = (1024, 256, 1024, 80)
  for scale, word in (((1023, 256, 1023, 80), b"n_fft"), ((1000, 250, 1000, 80), b"n_fft"), ((4096, 256, 1024, 80), b"n_fft"),
                      ((0, 1, 1, 1), b"n_fft"), ((1024, 0, 1024, 80), b"hop"), ((1024, 1025, 1024, 80), b"hop"),
                      ((1024, 256, 0, 80), b"win"), ((1024, 256, 1025, 80), b"win"), ((1024, 256, 1024, 0), b"n_mels"),
                      ((1024, 256, 1024, 514), b"n_mels"), ((32, 8, 32, 18), b"n_mels")):
    rc, _ = _create(lib, (ok, scale))
    assert rc == -1 and word in lib.wg_last_error(), scale
  rc, _ = _create(lib, (ok,), n=0)
  assert rc == -1 and b"scales" in lib.wg_last_error()
  rc, _ = _create(lib, (ok,) * 9)
  assert rc == -1 and b"scales" in lib.wg_last_error()
  for clamp in (0.0, -1.0, float("inf"), float("nan")):
    rc, _ = _create(lib, (ok,), clamp=clamp)
    assert rc == -1 and b"clamp" in lib.wg_last_error(), clamp
  h = C.c_void_p()
  one = (C.c_int32 * 1)(32)
  assert lib.wg_melloss_create(1, None, one, one, one, None, None, 1e-5, -1, C.byref(h)) == -1
  assert lib.wg_melloss_create(1, one, one, one, None, None, None, 1e-5, -1, C.byref(h)) == -1
  assert lib.wg_melloss_create(1, one, one, one, one, None, None, 1e-5, -1, None) == -1
  assert lib.wg_melloss_create(1, one, (C.c_int32 * 1)(8), one, (C.c_int32 * 1)(5), None, None, 1e-5, 0, C.byref(h)) == -1
  assert b"null" in lib.wg_last_error()                                            # a device handle needs both bases
  rc, h = _create(lib, (ok, (32, 8, 32, 17)))                                        # n_mels = n_fft / 2 + 1 is the top
  assert rc == 0

  dummy = (C.c_char * 64)()
  p = C.addressof(dummy)
  fwd = lambda **kw: lib.wg_melloss_forward(*[{**dict(h=h, audio=p, target=p, lens=None, fl=1.0, fn=0.0, out=p, spectra=p,
                                                       mels=p, B=1, N=4096, stream=None), **kw}[k]
                                              for k in ("h", "audio", "target", "lens", "fl", "fn", "out", "spectra", "mels",
                                                        "B", "N", "stream")])
  bwd = lambda **kw: lib.wg_melloss_backward(*[{**dict(h=h, g=p, lens=None, fl=1.0, fn=0.0, spectra=p, mels=p, out=p, B=1,
                                                        N=4096, stream=None), **kw}[k]
                                               for k in ("h", "g", "lens", "fl", "fn", "spectra", "mels", "out", "B", "N",
                                                         "stream")])
  for kw in (dict(h=None), dict(audio=None), dict(target=None), dict(out=None)):
    assert fwd(**kw) == -1 and b"null" in lib.wg_last_error(), kw
  for kw in (dict(spectra=None), dict(mels=None)):
    assert fwd(**kw) == -1 and b"together" in lib.wg_last_error(), kw
  for kw in (dict(h=None), dict(g=None), dict(spectra=None), dict(mels=None), dict(out=None)):
    assert bwd(**kw) == -1 and b"null" in lib.wg_last_error(), kw
  for call in (fwd, bwd):
    for kw in (dict(B=0), dict(B=65536), dict(N=512), dict(N=0), dict(N=-5)):
      assert call(**kw) == -1 and b"n_samples" in lib.wg_last_error(), kw
    assert call() == -2 and b"planning" in lib.wg_last_error()                       # sizes are fine: the handle cannot compute
  assert fwd(spectra=None, mels=None) == -2                                          # values only is a legal call
  assert lib.wg_melloss_destroy(h) == 0 and lib.wg_melloss_destroy(None) == 0


# ---- the Python layer without a device

def test_python_refusals_that_need_no_device():
  W = _lib.WgError
  with pytest.raises(W, match="GPU library only"):
    MultiScaleMelLoss(device="cpu")
  for kw, word in ((dict(n_ffts=(1000,), n_mels=(80,)), "n_fft"), (dict(n_ffts=(4096,), n_mels=(80,)), "n_fft"),
                   (dict(n_ffts=(1024,), n_mels=(80, 40)), "same length"), (dict(n_ffts=(1024,), n_mels=(514,)), "n_mels"),
                   (dict(n_ffts=(1024,), n_mels=(0,)), "n_mels"), (dict(n_ffts=(1024,), n_mels=(80,), hop_sizes=(0,)), "hop"),
                   (dict(n_ffts=(1024,), n_mels=(80,), hop_sizes=(256, 256)), "same length"),
                   (dict(n_ffts=(1024,), n_mels=(80,), win_lengths=(1025,)), "win_length"),
                   (dict(n_ffts=(64,) * 9, n_mels=(10,) * 9), "resolutions"), (dict(n_ffts=(), n_mels=()), "resolutions"),
                   (dict(clamp=0.0), "clamp"), (dict(clamp=float("inf")), "clamp"), (dict(clamp=float("nan")), "clamp"),
                   (dict(n_ffts=(64,), n_mels=(10,), mel_bases=[]), "mel_bases"),
                   (dict(n_ffts=(64,), n_mels=(10,), mel_bases=[np.zeros((10, 32), np.float32)]), "shape"),
                   (dict(n_ffts=(64,), n_mels=(10,), mel_bases=[np.full((10, 33), np.nan, np.float32)]), "non-finite")):
    with pytest.raises(W, match=word):
      MultiScaleMelLoss(**kw)
  check_scales(DAC_N_FFTS, tuple(n // 4 for n in DAC_N_FFTS), DAC_N_FFTS, DAC_N_MELS)
  import waveglow_amd
  assert waveglow_amd.MultiScaleMelLoss is MultiScaleMelLoss
