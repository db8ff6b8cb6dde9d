"""CPU: the fp64 yardstick of MultiResolutionSTFTLoss (tests/test_gpu_stft_loss.py) and host-only C-ABI checks.

``loss_ref64`` states the loss with ``torch.stft`` in float64; ``loss_unfold`` states it a second time, independently,
by reflect padding + ``unfold`` + a matmul with the windowed Fourier basis of ``denoiser.stft_bases`` (the basis the
library packs), in any dtype.  The two agree to 1e-8 in value and 1e-6 in the spectral-convergence gradient, which pins
the library's basis to ``torch.stft``.  Finite differences are no yardstick for this loss (L1 kinks, 1 / M at small
bins).  ``fragile_bins`` counts the bins whose sign or clamp an fp32 computation may flip; tests that bound the
log-magnitude gradient in L2 require it to be 0 for their inputs.
"""
import ctypes as C
import functools

import numpy as np
import pytest
import torch
import torch.nn.functional as Fn

from waveglow_amd import _lib, build
from waveglow_amd.denoiser import stft_bases

DEFAULT_RES = ((1024, 120, 600), (2048, 240, 1200), (512, 50, 240))


def audio(B, N, seed, silent=True):
  """``_audio`` of tests/test_gpu_mel_grads.py: uniform noise under a slow envelope, optionally with a silent stretch."""
  gen = torch.Generator().manual_seed(seed)
  y = (torch.rand(B, N, generator=gen) * 1.6 - 0.8) * torch.linspace(0.3, 1.0, N)[None, :]
  if silent:
    a, n = (N // 4, 2600) if N >= 8000 else (N // 5, N // 3)
    y[:, a:a + n] = 0.0
  return y


@functools.lru_cache(maxsize=None)
def basis32(n_fft, hop, win):
  """forward basis [2 * (n_fft / 2 + 1), n_fft] of denoiser.stft_bases, fp32 tensor."""
  return torch.from_numpy(stft_bases(n_fft, hop, win)[0])


def power_stft64(x, n_fft, hop, win):
  X = torch.stft(x, n_fft, hop, win, torch.hann_window(win, dtype=x.dtype), center=True, pad_mode="reflect",
                 return_complex=True)
  return X.real ** 2 + X.imag ** 2                                    # [B, K, F]


def power_unfold(x, n_fft, hop, win, dtype=None):
  dtype = dtype or x.dtype
  fwd = basis32(n_fft, hop, win).to(device=x.device, dtype=dtype)
  xp = Fn.pad(x.to(dtype)[:, None, :], (n_fft // 2, n_fft // 2), mode="reflect")[:, 0]
  fr = xp.unfold(1, n_fft, hop)                                        # [B, F, n_fft]
  X = torch.matmul(fr, fwd.t())                                        # [B, F, 2K]
  K = n_fft // 2 + 1
  return (X[..., :K] ** 2 + X[..., K:] ** 2).transpose(1, 2)


def terms_from_power(px, py, eps):
  mx, my = torch.clamp(px, min=eps).sqrt(), torch.clamp(py, min=eps).sqrt()
  sc = torch.linalg.norm((my - mx).reshape(-1)) / torch.linalg.norm(my.reshape(-1))
  mag = (my.log() - mx.log()).abs().mean()
  return sc, mag


def _loss(power_fn, x, y, resolutions, eps, factor_sc, factor_mag):
  sc = mag = 0.0
  for n_fft, hop, win in resolutions:
    s, m = terms_from_power(power_fn(x, n_fft, hop, win), power_fn(y, n_fft, hop, win), eps)
    sc, mag = sc + s, mag + m
  sc, mag = sc / len(resolutions), mag / len(resolutions)
  return sc, mag, factor_sc * sc + factor_mag * mag


def loss_ref64(x, y, resolutions=DEFAULT_RES, eps=1e-7, factor_sc=1.0, factor_mag=1.0):
  """(sc, mag, loss) in float64 with torch.stft; differentiable in x."""
  return _loss(power_stft64, x.double(), y.double(), resolutions, eps, factor_sc, factor_mag)


def loss_unfold(x, y, resolutions=DEFAULT_RES, eps=1e-7, factor_sc=1.0, factor_mag=1.0, dtype=torch.float64):
  """The same loss by pad + unfold + matmul with the library's fp32 basis, computed in ``dtype`` on x's device."""
  return _loss(functools.partial(power_unfold, dtype=dtype), x, y, resolutions, eps, factor_sc, factor_mag)


def grad_ref64(x, y, resolutions=DEFAULT_RES, eps=1e-7, factor_sc=1.0, factor_mag=1.0, fn=loss_ref64, **kw):
  xg = x.detach().clone().requires_grad_(True)
  (g,) = torch.autograd.grad(fn(xg, y, resolutions, eps, factor_sc, factor_mag, **kw)[2], xg)
  return g


def fragile_bins(x, y, resolutions=DEFAULT_RES, eps=1e-7, tau=1e-5, frames=None):
  """(fragile, total) in fp64: bins above the clamp whose log-magnitude difference is within tau of 0, plus bins whose
  power is within tau (relative) of eps.  A condition on the inputs, computed from the reference alone.  ``frames``:
  None, or per resolution the frame indices to which the count is restricted (tests/_loss_cells.py)."""
  bad = total = 0
  for i, (n_fft, hop, win) in enumerate(resolutions):
    px, py = power_stft64(x.double(), n_fft, hop, win), power_stft64(y.double(), n_fft, hop, win)
    if frames is not None:
      px, py = px[..., frames[i]], py[..., frames[i]]
    mx, my = torch.clamp(px, min=eps).sqrt(), torch.clamp(py, min=eps).sqrt()
    bad += int(((px > eps) & ((my.log() - mx.log()).abs() < tau)).sum())
    bad += int(((px / eps - 1).abs() < tau).sum())
    total += px.numel()
  return bad, total


def rel(a, b):
  return float((a.double() - b.double()).norm() / b.double().norm())


def log_mag_inputs(B, N, silent):
  return audio(B, N, 100 + N, silent), audio(B, N, 150 + N, False)


SMALL = [(1, 1025), (2, 2048), (1, 4096)]


@pytest.mark.parametrize("B,N", SMALL)
@pytest.mark.parametrize("silent", [False, True])
def test_two_fp64_restatements_agree(B, N, silent):
  """Values to 1e-8 and SC gradient to 1e-6 (measured 1e-11 .. 1.4e-9 and 2.2e-8 .. 3.6e-8) at eps = 1e-2, where these
  inputs have no bin near the clamp.  At the default eps = 1e-7 the spectral convergence still agrees to 1e-8, but the
  log-magnitude term is ill-conditioned in near-empty bins: the fp32 rounding of the basis (2^-24 per entry) moves
  (re, im) of such a bin by up to 6e-8 * sum |w x| ~ 1e-5 against M >= sqrt(eps) = 3e-4, i.e. its log by up to 3e-2,
  and one such bin among 15 139 with a mean |log M(y) - log M(x)| near 1 moves the mean by 2e-6.  Bound there: 1e-5
  (measured 3.0e-10 .. 2.0e-8)."""
  x, y = audio(B, N, 100 + N, silent).double(), audio(B, N, 150 + N, False).double()
  a, b = loss_ref64(x, y, eps=1e-2), loss_unfold(x, y, eps=1e-2)
  for u, v in zip(a, b):
    assert abs(float(u) - float(v)) <= 1e-8 * abs(float(u))
  a, b = loss_ref64(x, y), loss_unfold(x, y)
  assert abs(float(a[0]) - float(b[0])) <= 1e-8 * abs(float(a[0]))
  assert abs(float(a[1]) - float(b[1])) <= 1e-5 * abs(float(a[1]))
  ga = grad_ref64(x, y, factor_mag=0.0)
  gb = grad_ref64(x, y, factor_mag=0.0, fn=loss_unfold)
  assert rel(gb, ga) <= 1e-6


def test_single_resolutions_and_dividing_hop_agree():
  x, y = audio(2, 2048, 3, True).double(), audio(2, 2048, 4, False).double()
  for res in (((1024, 256, 1024),), ((512, 50, 240),), ((2048, 2048, 2048),), ((1024, 256, 1024), (512, 50, 240))):
    a, b = loss_ref64(x, y, res, eps=1e-2), loss_unfold(x, y, res, eps=1e-2)
    for u, v in zip(a, b):
      assert abs(float(u) - float(v)) <= 1e-8 * abs(float(u))


@pytest.mark.parametrize("B,N", SMALL)
@pytest.mark.parametrize("silent", [False, True])
def test_log_magnitude_inputs_have_no_fragile_bins(B, N, silent):
  x, y = log_mag_inputs(B, N, silent)
  bad, total = fragile_bins(x, y, eps=1e-2, tau=1e-5)
  assert total == sum(B * (n // 2 + 1) * (N // h + 1) for n, h, _ in DEFAULT_RES)
  assert bad == 0


def test_fragile_bins_counts_both_kinds():
  x = audio(1, 2048, 1, False)
  bad, total = fragile_bins(x, x.clone(), eps=1e-7)          # every bin has log M(y) - log M(x) = 0
  assert bad >= total - 16
  z = torch.zeros(1, 2048)
  bad, _ = fragile_bins(z, x, eps=1e-7)                        # all clamped, none near the clamp: nothing fragile
  assert bad == 0


def test_silent_prediction_has_finite_gradient():
  x, y = audio(1, 6000, 7, True).double(), audio(1, 6000, 8, False).double()
  g = grad_ref64(x, y)
  assert torch.isfinite(g).all()


def test_library_basis_is_the_denoisers():
  from waveglow_amd.stft_loss import forward_basis
  for n_fft, hop, win in ((512, 50, 240), (1024, 256, 1024), (96, 7, 33)):
    assert np.array_equal(forward_basis(n_fft, win), stft_bases(n_fft, hop, win)[0])


@pytest.fixture(scope="module")
def lib():
  build.build_library()
  return _lib.load()


def _create(lib, n_fft, hop, win, eps=1e-7, n=None):
  n = len(n_fft) if n is None else n
  arr = lambda v: (C.c_int32 * max(len(v), 1))(*v)
  h = C.c_void_p()
  rc = lib.wg_stftloss_create(n, arr(n_fft), arr(hop), arr(win), None, eps, -1, C.byref(h))
  return rc, h


def test_entry_points_validate_arguments_without_a_gpu(lib):
  """Argument checks run before any device work; device_id < 0 gives a planning handle that sizes workspaces."""
  for n_fft, hop, win, word in (((1023,), (120,), (600,), b"n_fft"), ((1000,), (120,), (600,), b"n_fft"),
                                ((4096,), (120,), (600,), b"n_fft"), ((1024,), (0,), (600,), b"hop"),
                                ((1024,), (1025,), (600,), b"hop"), ((1024,), (120,), (1025,), b"win"),
                                ((1024,), (120,), (0,), b"win")):
    rc, _ = _create(lib, n_fft, hop, win)
    assert rc == -1 and word in lib.wg_last_error(), (n_fft, hop, win)
  rc, _ = _create(lib, (1024,), (120,), (600,), n=0)
  assert rc == -1 and b"resolutions" in lib.wg_last_error()
  rc, _ = _create(lib, (1024,) * 9, (120,) * 9, (600,) * 9)
  assert rc == -1 and b"resolutions" in lib.wg_last_error()
  rc, _ = _create(lib, (1024,), (120,), (600,), eps=0.0)
  assert rc == -1 and b"eps" in lib.wg_last_error()

  rc, h = _create(lib, *zip(*DEFAULT_RES))
  assert rc == 0
  assert lib.wg_stftloss_workspace_bytes(h, 1, 1024, 1) == 0            # N <= max n_fft / 2
  assert lib.wg_stftloss_workspace_bytes(h, 0, 4096, 1) == 0
  one, two = (lib.wg_stftloss_workspace_bytes(h, b, 4096, 1) for b in (1, 2))
  assert 0 < one < two
  assert 0 < lib.wg_stftloss_workspace_bytes(h, 2, 4096, 0) < two       # values only: no saved transform
  # the saved state alone: (re, im) [B, n_fft, F] and M(y) [B, K, F] per resolution
  floor = sum(4 * 2 * (n + n // 2 + 1) * (4096 // hp + 1) for n, hp, _ in DEFAULT_RES)
  assert floor <= two
  dummy = (C.c_char * 64)()
  p = C.addressof(dummy)
  assert lib.wg_stftloss_forward(h, p, p, None, 1.0, 1.0, p, 1, 4096, 0, p, 1 << 40, None) == -2    # planning handle
  assert lib.wg_stftloss_forward(h, None, p, None, 1.0, 1.0, p, 1, 4096, 1, p, 1 << 40, None) == -1
  assert b"null" in lib.wg_last_error()
  assert lib.wg_stftloss_backward(h, p, None, 1.0, 1.0, None, 1, 4096, p, 1 << 40, None) == -1
  assert lib.wg_stftloss_destroy(h) == 0
  # the Python surface refuses the same geometries before it touches a device
  from waveglow_amd.stft_loss import check_geometry
  with pytest.raises(_lib.WgError):
    check_geometry((1000,), (100,), (600,))
  with pytest.raises(_lib.WgError):
    check_geometry((1024,) * 9, (120,) * 9, (600,) * 9)
  check_geometry(*zip(*DEFAULT_RES))
