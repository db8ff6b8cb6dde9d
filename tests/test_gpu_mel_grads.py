"""GPU: ``TacotronSTFT.mel_spectrogram_differentiable`` -- the mel front-end with an audio gradient.

Yardsticks: ``mel_spectrogram`` itself (values, bit for bit), the fp64 torch restatement of tests/test_mel_grads_cpu.py
(gradients, ``||g - g_ref|| <= 1e-4 ||g_ref||`` per utterance), the library's own forward at full size (central
difference of a directional derivative), and a torch composition on the GPU behind the frozen vocoder (d mel).
"""
import pytest
import torch

from _cases import Case
from test_mel_grads_cpu import constants64, mel_grad_ref64, mel_ref64
from waveglow_amd._lib import WgError
from waveglow_amd.model import WaveGlow
from waveglow_amd.taco_stft import TacotronSTFT, TSTFTHParams

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
GRAD_TOL = 1e-4
SHAPES = [(1, 513), (2, 1024), (3, 22050), (2, 16000)]


@pytest.fixture(scope="module")
def taco():
  return TacotronSTFT(TSTFTHParams(), DEV)


def _audio(B, N, seed, silent=True):
  """Uniform noise under a slow envelope, in [-0.8, 0.8], with an exactly silent stretch: at the longer lengths whole
  frames are silent (|X| = 0, mel clamped), at the short ones part of every window is."""
  gen = torch.Generator().manual_seed(seed)
  y = (torch.rand(B, N, generator=gen) * 1.6 - 0.8) * torch.linspace(0.3, 1.0, N)[None, :]
  if silent:
    a, n = (N // 4, 2600) if N >= 8000 else (N // 5, N // 3)
    y[:, a:a + n] = 0.0
  return y


def _rel(g, ref):
  return float((g.double() - ref.double()).norm() / ref.double().norm())


@pytest.mark.parametrize("B,N", SHAPES)
def test_values_bit_identical_to_mel_spectrogram(taco, B, N):
  y = _audio(B, N, seed=N).to(DEV)
  ref = taco.mel_spectrogram(y)
  yg = y.clone().requires_grad_(True)
  out = taco.mel_spectrogram_differentiable(yg)
  assert out.requires_grad and out.grad_fn is not None
  assert out.shape == (B, 80, N // 256 + 1) and torch.equal(out.detach(), ref)
  with torch.no_grad():
    plain = taco.mel_spectrogram_differentiable(yg)
  assert plain.grad_fn is None and not plain.requires_grad and torch.equal(plain, ref)
  plain = taco.mel_spectrogram_differentiable(y)
  assert plain.grad_fn is None and torch.equal(plain, ref)


def _check_grads(taco, y, g, label):
  fwd, basis = constants64()
  yg = y.to(DEV).requires_grad_(True)
  (taco.mel_spectrogram_differentiable(yg) * g.to(DEV)).sum().backward()
  ref = mel_grad_ref64(y, g, fwd, basis)
  got = yg.grad.cpu()
  assert torch.isfinite(got).all()
  errs = [_rel(got[b], ref[b]) for b in range(y.shape[0])]
  print(f"{label}: rel L2 err per utterance {', '.join(f'{e:.2e}' for e in errs)}")
  assert max(errs) <= GRAD_TOL


@pytest.mark.parametrize("B,N", SHAPES)
def test_gradient_matches_fp64(taco, B, N):
  """Measured on the MI355X: rel L2 5.9e-7 .. 4.2e-6 per utterance with weights on every frame, 4.8e-7 .. 7.3e-7 with
  weights on frames 0 and F-1 only."""
  y = _audio(B, N, seed=10 + N)
  F = N // 256 + 1
  gen = torch.Generator().manual_seed(N)
  _check_grads(taco, y, torch.randn(B, 80, F, generator=gen), f"B={B} N={N} all frames")
  g = torch.zeros(B, 80, F)
  g[:, :, 0] = torch.randn(B, 80, generator=gen)
  g[:, :, F - 1] = torch.randn(B, 80, generator=gen)
  _check_grads(taco, y, g, f"B={B} N={N} frames 0 and F-1")


def test_full_size_directional_derivative_and_retain_graph(taco):
  """B = 16 x 221 184 (configs[1] audio): <d L / d y, v> against the central difference of the library's own forward,
  L = <r, mel>.  Measured relative error 5.8e-3 (tolerance 1e-2); the two backwards are bit-identical."""
  B, N = 16, 221184
  gen = torch.Generator(device=DEV).manual_seed(3)
  t = torch.arange(N, device=DEV, dtype=torch.float32) / 22050.0
  f0 = 110.0 + 40.0 * torch.arange(B, device=DEV, dtype=torch.float32)[:, None]
  y = 0.25 * torch.sin(2 * torch.pi * f0 * t) + 0.05 * torch.randn(B, N, generator=gen, device=DEV)
  r = torch.randn(B, 80, N // 256 + 1, generator=gen, device=DEV)
  v = torch.randn(B, N, generator=gen, device=DEV)
  yg = y.clone().requires_grad_(True)
  loss = (taco.mel_spectrogram_differentiable(yg) * r).sum()
  (g1,) = torch.autograd.grad(loss, yg, retain_graph=True)
  (g2,) = torch.autograd.grad(loss, yg)
  assert torch.equal(g1, g2)
  h = 1e-3
  with torch.no_grad():
    lp = (taco.mel_spectrogram_differentiable(y + h * v).double() * r.double()).sum()
    lm = (taco.mel_spectrogram_differentiable(y - h * v).double() * r.double()).sum()
  fd = float((lp - lm) / (2 * h))
  an = float((g1.double() * v.double()).sum())
  err = abs(an - fd) / abs(fd)
  print(f"full size: <g, v> = {an:.6e}, central difference {fd:.6e}, rel err {err:.2e}")
  assert err <= 1e-2


def test_mel_loss_through_frozen_vocoder():
  """L1(mel(vocoder(mel)), mel) on the c64 case: d mel through this front-end vs through a torch composition on the
  GPU (reflect pad, conv1d, sqrt, matmul, clamp, log).  Both legs share infer_differentiable's backward.
  Measured: d mel rel L2 2.3e-5, mel_hat max abs difference 2.4e-7."""
  c = Case("c64")
  model = WaveGlow.remove_weightnorm(WaveGlow(c.hp))
  model.load_state_dict(c.sd)
  model = model.to(DEV).eval().requires_grad_(False)
  taco = TacotronSTFT(TSTFTHParams(n_mel_channels=c.hp.n_mel_channels), DEV)
  fwd, basis = constants64(c.hp.n_mel_channels)
  fwd, basis = fwd.float().to(DEV), basis.float().to(DEV)
  T = c.mel.shape[-1]

  def leg(mel_fn):
    mel = c.mel.to(DEV).requires_grad_(True)
    ze = [c.z_early[k].to(DEV) for k in sorted(c.z_early, reverse=True)]
    audio = model.infer_differentiable(mel, c.sigma, z_init=c.z_init.to(DEV), z_early=ze)
    mel_hat = mel_fn(audio)[..., :T]
    (mel_hat - mel).abs().mean().backward()
    assert bool(model.grad_finite)
    return mel.grad.detach().clone(), mel_hat.detach()

  g_lib, hat_lib = leg(taco.mel_spectrogram_differentiable)
  g_ref, hat_ref = leg(lambda a: mel_ref64(a, fwd, basis))
  err, herr = _rel(g_lib, g_ref), float((hat_lib - hat_ref).abs().max())
  print(f"vocoder cycle: d mel rel L2 {err:.2e}, mel_hat max abs diff {herr:.2e}")
  assert torch.isfinite(g_lib).all() and err <= 1e-3


def test_errors(taco):
  y = _audio(1, 2048, seed=1)
  with pytest.raises(WgError):
    taco.mel_spectrogram_differentiable(y.requires_grad_(True))                           # CPU tensor
  with pytest.raises(WgError):
    taco.mel_spectrogram_differentiable(y.detach().to(DEV).half().requires_grad_(True))   # fp16
  with pytest.raises(WgError):
    taco.mel_spectrogram_differentiable(torch.zeros(1, 512, device=DEV, requires_grad=True))  # too short
  wide = TacotronSTFT(TSTFTHParams(n_mel_channels=129), DEV)
  with pytest.raises(WgError):
    wide.mel_spectrogram_differentiable(y.detach().to(DEV).requires_grad_(True))
  with pytest.raises(WgError):
    wide.mel_spectrogram_differentiable(y.detach().to(DEV))
