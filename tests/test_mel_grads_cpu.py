"""CPU: the fp64 yardstick of TacotronSTFT.mel_spectrogram_differentiable (tests/test_gpu_mel_grads.py).

``mel_ref64`` restates the front-end in torch float64 from the library's own constants (``denoiser.stft_bases``, the
fp32 windowed Fourier basis, and ``slaney_mel_filterbank``): reflect padding (stft.py:141-147), the conv-STFT
(stft.py:150-158), the magnitude with a masked sqrt (a zero magnitude gets a zero gradient, where plain torch gives
NaN), the mel projection and log(clamp(., 1e-5)) (taco_stft.py:10-16, :99-104).  It is checked here against central
finite differences and against the values of oracle/stft_oracle.mel_spectrogram.
"""
import os

import numpy as np
import torch
import torch.nn.functional as Fn

from waveglow_amd import _lib
from waveglow_amd.denoiser import stft_bases
from waveglow_amd.taco_stft import slaney_mel_filterbank

FL, HOP = 1024, 256


def constants64(n_mel=80, sr=22050, fmin=0.0, fmax=8000.0):
  """(forward basis [1026, 1024], mel basis [n_mel, 513]) as float64 tensors of the fp32 values the library uses."""
  fwd, _, _ = stft_bases(FL, HOP, FL)
  basis = slaney_mel_filterbank(sr, FL, n_mel, fmin, fmax)
  return torch.from_numpy(fwd).double(), torch.from_numpy(basis).double()


def mel_ref64(y, fwd, basis):
  """y [B, N] float64 (N > 512) -> log-mel [B, n_mel, N // 256 + 1], differentiable in y."""
  yp = Fn.pad(y[:, None, :], (FL // 2, FL // 2), mode="reflect")
  X = Fn.conv1d(yp, fwd[:, None, :], stride=HOP)                     # [B, 1026, F]
  cut = FL // 2 + 1
  p = X[:, :cut] ** 2 + X[:, cut:] ** 2
  nz = p > 0
  mag = torch.where(nz, torch.where(nz, p, torch.ones_like(p)).sqrt(), torch.zeros_like(p))
  A = torch.matmul(basis, mag)
  return torch.log(torch.clamp(A, min=1e-5))


def mel_grad_ref64(y, g, fwd, basis):
  """d <g, mel_ref64(y)> / d y in float64, for y [B, N] and g [B, n_mel, F] (any float dtype)."""
  y = y.detach().double().requires_grad_(True)
  (gy,) = torch.autograd.grad((mel_ref64(y, fwd, basis) * g.double()).sum(), y)
  return gy


def test_values_match_numpy_oracle():
  from oracle import stft_oracle as S
  fwd, basis = constants64()
  rng = np.random.default_rng(11)
  for B, N in ((1, 513), (2, 3000)):
    x = rng.uniform(-0.7, 0.7, size=(B, N))
    ours = mel_ref64(torch.from_numpy(x), fwd, basis).numpy()
    ref = S.mel_spectrogram(x, basis.numpy().astype(np.float32))
    assert ours.shape == ref.shape == (B, 80, N // HOP + 1)
    # the oracle builds its basis in fp64, ours is the library's fp32 basis: agreement at fp32 rounding
    assert np.abs(ours - ref).max() <= 1e-4


def test_gradient_matches_central_differences():
  fwd, basis = constants64()
  gen = torch.Generator().manual_seed(5)
  y = (torch.rand(1, 700, generator=gen, dtype=torch.float64) - 0.5)
  g = torch.randn(1, 80, 700 // HOP + 1, generator=gen, dtype=torch.float64)
  assert torch.autograd.gradcheck(lambda t: (mel_ref64(t, fwd, basis) * g).sum(), (y.requires_grad_(True),),
                                  eps=1e-6, atol=1e-6, rtol=1e-4)
  # directional derivatives at a length where both reflect edges and the interior are present
  y = (torch.rand(2, 2600, generator=gen, dtype=torch.float64) - 0.5) * 0.6
  g = torch.randn(2, 80, 2600 // HOP + 1, generator=gen, dtype=torch.float64)
  gy = mel_grad_ref64(y, g, fwd, basis)
  for seed in range(3):
    v = torch.randn(y.shape, generator=torch.Generator().manual_seed(100 + seed), dtype=torch.float64)
    h = 1e-6
    fd = ((mel_ref64(y + h * v, fwd, basis) - mel_ref64(y - h * v, fwd, basis)) * g).sum() / (2 * h)
    assert abs(float(fd) - float((gy * v).sum())) <= 1e-6 * abs(float(fd))


def test_silent_stretch_gives_finite_gradient():
  """An exactly silent frame has |X| = 0 and a clamped mel: both masks give 0, the gradient stays finite."""
  fwd, basis = constants64()
  gen = torch.Generator().manual_seed(7)
  y = (torch.rand(1, 6000, generator=gen, dtype=torch.float64) - 0.5)
  y[:, 1000:4500] = 0.0
  g = torch.randn(1, 80, 6000 // HOP + 1, generator=gen, dtype=torch.float64)
  gy = mel_grad_ref64(y, g, fwd, basis)
  assert torch.isfinite(gy).all()
  mel = mel_ref64(y, fwd, basis)
  assert (mel[0, :, 10] == float(np.log(1e-5))).all()          # frame 10 covers padded 2560..3583: all silent


def test_entry_points_are_declared_and_bound():
  root = os.path.dirname(os.path.dirname(os.path.abspath(_lib.__file__)))
  with open(os.path.join(root, "include", "waveglow_amd.h")) as f:
    header = f.read()
  for name in ("wg_stft_mel_grad_workspace_bytes", "wg_stft_mel_forward_saved", "wg_stft_mel_backward"):
    assert name in _lib.SIGNATURES and f" {name}(" in header
