"""GPU: the per-utterance lengths of the STFT calls are a nullable pointer of ONE symbol, so "every length equal to
n_samples gives the bits of a null pointer" is a promise of that symbol with itself.  Checked through ctypes at B = 2,
every output pre-filled with NaN, whole buffers compared byte for byte: ``wg_stft_mel``, the
``wg_stft_mel_forward_saved`` / ``wg_stft_mel_backward`` pair, ``wg_stft_denoise``, and ``wg_stftloss_forward`` /
``wg_stftloss_backward`` with ``saved`` = 0 and 1.  (The same promise at the Python layer and at working sizes:
tests/test_gpu_ragged_losses.py::test_equal_lengths_give_the_dense_bits.)

Sizes: N = 1280 for the mel calls (above the 512-sample floor, a multiple of 256: the last frame starts on the last
sample); N = 2048 for the denoiser (a multiple of 256, at least 1024); N = 1280 with the one resolution (64, 16, 48) for
the STFT loss.
"""
import ctypes as C

import pytest
import torch

import _dirty as D
from waveglow_amd import _lib
from waveglow_amd.stft_loss import MultiResolutionSTFTLoss
from waveglow_amd.taco_stft import TacotronSTFT, TSTFTHParams

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
B = 2
NAN = float("nan")


def _audio(N, seed):
  gen = torch.Generator().manual_seed(seed)
  return (0.3 * torch.randn(B, N, generator=gen)).to(DEV)


def _nan(*shape):
  return torch.full(shape, NAN, dtype=torch.float32, device=DEV)


def _lens(N):
  return torch.tensor([N] * B, dtype=torch.int32).to(DEV)


def _both(N, call):
  """call(lens pointer or None) -> dict of outputs; the dict with all-full lengths against the one with a null pointer."""
  ld = _lens(N)
  full, null = call(ld.data_ptr()), call(None)
  torch.cuda.synchronize()
  for name, t in null.items():
    assert bool(torch.isfinite(t).all()) and bool(t.any()), name
  D.same_outputs(full, null, f"lens = [{N}] * {B} against lens = NULL")


@pytest.fixture(scope="module")
def taco():
  return TacotronSTFT(TSTFTHParams(), DEV)


def test_mel_front_end(taco):
  N, M, F = 1280, taco.n_mel_channels, 1280 // 256 + 1
  y = _audio(N, 1)
  nbytes = taco.lib.wg_stft_mel_workspace_bytes(taco._h, B, N)
  assert nbytes > 0

  def call(lens):
    mel, ws = _nan(B, M, F), torch.empty(nbytes, dtype=torch.uint8, device=DEV)
    _lib.check(taco.lib.wg_stft_mel(taco._h, taco.mel_basis.data_ptr(), M, y.data_ptr(), lens, mel.data_ptr(), B, N,
                                    ws.data_ptr(), nbytes, None))
    return {"mel": mel}

  _both(N, call)


def test_mel_front_end_gradient(taco):
  N, M, F = 1280, taco.n_mel_channels, 1280 // 256 + 1
  y = _audio(N, 2)
  g = torch.randn(B, M, F, generator=torch.Generator().manual_seed(3)).to(DEV)
  nbytes = taco.lib.wg_stft_mel_grad_workspace_bytes(taco._h, B, N)
  assert nbytes > 0

  def call(lens):
    mel, gy, ws = _nan(B, M, F), _nan(B, N), torch.empty(nbytes, dtype=torch.uint8, device=DEV)
    _lib.check(taco.lib.wg_stft_mel_forward_saved(taco._h, taco.mel_basis.data_ptr(), M, y.data_ptr(), lens,
                                                  mel.data_ptr(), B, N, ws.data_ptr(), nbytes, None))
    _lib.check(taco.lib.wg_stft_mel_backward(taco._h, taco.mel_basis.data_ptr(), M, g.data_ptr(), lens, gy.data_ptr(), B,
                                             N, ws.data_ptr(), nbytes, None))
    return {"mel": mel, "d audio": gy}

  _both(N, call)


def test_denoiser(taco):
  """The mel front-end's handle is a wg_stft handle: it serves wg_stft_denoise as well."""
  N = 2048
  x = _audio(N, 4)
  bias = torch.rand(513, generator=torch.Generator().manual_seed(5)).to(DEV)
  nbytes = taco.lib.wg_stft_workspace_bytes(taco._h, B, N)
  assert nbytes > 0

  def call(lens):
    out, mag0, ws = _nan(B, N), _nan(B, 513), torch.empty(nbytes, dtype=torch.uint8, device=DEV)
    _lib.check(taco.lib.wg_stft_denoise(taco._h, x.data_ptr(), lens, bias.data_ptr(), 0.1, out.data_ptr(), mag0.data_ptr(),
                                        B, N, ws.data_ptr(), nbytes, None))
    return {"audio": out, "mag0": mag0}

  _both(N, call)


@pytest.mark.parametrize("saved", [0, 1])
def test_stft_loss(saved):
  N = 1280
  crit = MultiResolutionSTFTLoss((64,), (16,), (48,), device=DEV)
  x, y = _audio(N, 6), _audio(N, 7)
  g3 = torch.tensor([0.3, -1.7, 0.9], device=DEV)
  nbytes = crit.lib.wg_stftloss_workspace_bytes(crit._h, B, N, saved)
  assert nbytes > 0

  def call(lens):
    out3, gx, ws = _nan(3), _nan(B, N), torch.empty(nbytes, dtype=torch.uint8, device=DEV)
    _lib.check(crit.lib.wg_stftloss_forward(crit._h, x.data_ptr(), y.data_ptr(), lens, 1.0, 1.0, out3.data_ptr(), B, N,
                                            saved, ws.data_ptr(), nbytes, None))
    if not saved:
      return {"out3": out3}
    _lib.check(crit.lib.wg_stftloss_backward(crit._h, g3.data_ptr(), lens, 1.0, 1.0, gx.data_ptr(), B, N, ws.data_ptr(),
                                             nbytes, None))
    return {"out3": out3, "d audio": gx}

  _both(N, call)
