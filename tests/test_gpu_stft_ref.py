"""GPU: the HIP conv-STFT, denoiser and mel front-end against outputs of the REFERENCE's own classes.

tests/golden/stft_ref.npz (tests/golden/make_golden_stft.py, contents: tests/_stft_ref.py) holds what the reference's
``STFT``, ``TacotronSTFT`` and ``Denoiser`` gave on the CPU.  The bars are the ones the kernels are held to against
oracle/stft_oracle.py elsewhere in the suite (2e-5 denoised audio, 1e-4 magnitudes, 2e-4 log-mel, 1e-3 rms flow audio);
tests/test_stft_ref_cpu.py holds that oracle to a tenth of each against the same fixture.  Nothing outside tests/golden/
is read.  Not pinned: the values of the mel filter bank (the project's on both sides of the fixture).
"""
import ast
import ctypes as C

import numpy as np
import pytest
import torch

import _stft_ref as R
from _cases import rms
from test_gpu_mel_grads import GRAD_TOL
from test_gpu_parity import RMS_TOL, build_model
from test_mel_grads_cpu import constants64, mel_grad_ref64
from waveglow_amd import _lib, synthetic
from waveglow_amd.denoiser import stft_bases
from waveglow_amd.hparams import HParams
from waveglow_amd.taco_stft import TacotronSTFT, TSTFTHParams

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
AUDIO_TOL, MAG_TOL, MEL_TOL = 2e-5, 1e-4, 2e-4


@pytest.fixture(scope="module")
def fx():
  return R.fixture()


class _Stft:
  """A wg_stft handle and the two denoiser entry points on numpy arrays."""

  def __init__(self):
    self.lib = _lib.load()
    fwd, inv, wsq = stft_bases()
    self.h = C.c_void_p()
    _lib.check(self.lib.wg_stft_create(fwd.ctypes.data, inv.ctypes.data, wsq.ctypes.data, 1024, 256, 0, C.byref(self.h)))

  def close(self):
    self.lib.wg_stft_destroy(self.h)

  def _workspace(self, B, N):
    nbytes = self.lib.wg_stft_workspace_bytes(self.h, B, N)
    assert nbytes > 0
    return torch.empty(nbytes, dtype=torch.uint8, device=DEV)

  def denoise(self, x, bias, strength):
    """(out [B, N], mag0 [B, 513]); both buffers start as NaN."""
    B, N = x.shape
    xd, bd = torch.from_numpy(x).to(DEV), torch.from_numpy(bias).to(DEV)
    out = torch.full_like(xd, float("nan"))
    mag0 = torch.full((B, 513), float("nan"), dtype=torch.float32, device=DEV)
    ws = self._workspace(B, N)
    _lib.check(self.lib.wg_stft_denoise(self.h, xd.data_ptr(), None, bd.data_ptr(), float(strength), out.data_ptr(),
                                        mag0.data_ptr(), B, N, ws.data_ptr(), ws.numel(), None))
    torch.cuda.synchronize()
    return out.cpu().numpy(), mag0.cpu().numpy()

  def denoise_ragged(self, x, lens, bias, strength):
    B, N = x.shape
    xd, bd = torch.from_numpy(x).to(DEV), torch.from_numpy(bias).to(DEV)
    ld = torch.tensor(lens, dtype=torch.int32).to(DEV)
    out = torch.full_like(xd, float("nan"))
    ws = self._workspace(B, N)
    _lib.check(self.lib.wg_stft_denoise(self.h, xd.data_ptr(), ld.data_ptr(), bd.data_ptr(), float(strength),
                                        out.data_ptr(), None, B, N, ws.data_ptr(), ws.numel(), None))
    torch.cuda.synchronize()
    return out.cpu().numpy()


@pytest.fixture(scope="module")
def stft():
  s = _Stft()
  yield s
  s.close()


@pytest.mark.parametrize("name,T,B,strength,kind", R.denoise_cases(), ids=[c[0] for c in R.denoise_cases()])
def test_denoise_matches_reference(fx, stft, name, T, B, strength, kind):
  """wg_stft_denoise at every stored case.  Measured on the MI355X: audio max abs 1.9e-6 ... 3.5e-6 (2.5e-8 for silence
  at s = -0.1, exact zeros where the reference has them), mag0 <= 2.5e-5 abs at values up to 22."""
  x = fx.denoise_input(name, T, B, kind)
  ref, ref_is_zero = fx.denoise_expected(name, T, B, strength, kind)
  mag0_ref = fx.denoise_mag0(T, B, kind)
  out, mag0 = stft.denoise(x, fx.denoise_bias(), strength)
  assert out.shape == ref.shape == (B, 256 * T) and np.isfinite(out).all() and np.isfinite(mag0).all()
  err = float(np.abs(out.astype(np.float64) - ref).max())
  print(f"{name}: max abs err vs reference {err:.2e} (reference max {float(np.abs(ref).max()):.3f}); "
        f"mag0 max abs err {float(np.abs(mag0.astype(np.float64) - mag0_ref).max()):.2e} at max {float(mag0_ref.max()):.1f}")
  if ref_is_zero:
    assert not out.any()                     # s = 1e4 (every bin clamps) and silence: exact zeros
  else:
    assert float(np.abs(ref).max()) > 1e-2
  assert err <= AUDIO_TOL
  np.testing.assert_allclose(mag0, mag0_ref, rtol=MAG_TOL, atol=MAG_TOL)
  if kind == "zeros":
    assert not mag0.any()


def test_denoise_ragged_rows_match_reference(fx, stft):
  """The five lengths as ONE wg_stft_denoise call with lengths (the longest not first): every row is bit for bit its single call
  and therefore within the same bar of the reference; zeros behind every utterance."""
  assert sorted(R.RAGGED_ORDER) == sorted(R.DENOISE_T) and R.RAGGED_ORDER[0] != max(R.RAGGED_ORDER)
  lens = [256 * T for T in R.RAGGED_ORDER]
  N = max(lens)
  x = np.full((len(lens), N), 0.7, dtype=np.float32)          # behind an utterance: must not matter
  for b, T in enumerate(R.RAGGED_ORDER):
    x[b, :lens[b]] = fx.denoise_input(f"T{T}_s0.1", T, 1, "randn")[0]
  bias = fx.denoise_bias()
  out = stft.denoise_ragged(x, lens, bias, 0.1)
  for b, T in enumerate(R.RAGGED_ORDER):
    single, _ = stft.denoise(np.ascontiguousarray(x[b:b + 1, :lens[b]]), bias, 0.1)
    ref, _ = fx.denoise_expected(f"T{T}_s0.1", T, 1, 0.1, "randn")
    err = float(np.abs(out[b, :lens[b]].astype(np.float64) - ref[0]).max())
    print(f"ragged row {b} (T = {T}): max abs err vs reference {err:.2e}")
    assert np.array_equal(out[b, :lens[b]], single[0]), f"row {b} (T = {T}) differs from its single call"
    assert not out[b, lens[b]:].any(), f"row {b}: not zero behind its end"
    assert err <= AUDIO_TOL


@pytest.fixture(scope="module")
def tacos():
  made = {}

  def get(n_mel):
    if n_mel not in made:
      made[n_mel] = TacotronSTFT(TSTFTHParams(n_mel_channels=n_mel), DEV)
    return made[n_mel]
  return get


@pytest.mark.parametrize("N,n_mel", R.mel_cases())
def test_mel_matches_reference(fx, tacos, N, n_mel):
  """TacotronSTFT.mel_spectrogram at every stored length and row count.  Measured on the MI355X: max abs 4.8e-7 ... 3.8e-6."""
  ref = fx.mel_expected(N, n_mel)
  mel = tacos(n_mel).mel_spectrogram(torch.from_numpy(fx.mel_input(N))).cpu().numpy()
  assert mel.shape == ref.shape == (1, n_mel, N // 256 + 1)
  err = float(np.abs(mel.astype(np.float64) - ref).max())
  floor = np.float32(np.log(np.float32(1e-5)))
  print(f"mel N={N} n_mel={n_mel}: max abs err vs reference {err:.2e}; {100 * float((ref == floor).mean()):.1f} % of the "
        f"reference at log 1e-5")
  assert np.isfinite(mel).all() and err <= MEL_TOL


@pytest.mark.parametrize("n_mel", R.MEL_ROWS_EXTRA)
def test_mel_gradient_at_other_row_counts(fx, tacos, n_mel):
  """mel_spectrogram_differentiable's backward at 1, 5, 127 and 128 mel rows (tests/test_gpu_mel_grads.py runs 80 only):
  N = 16128, weights on every frame, against the fp64 torch restatement.  Measured on the MI355X: rel L2 1.8e-6, 1.3e-6, 1.0e-6, 8.1e-7."""
  N = 16128
  y = torch.from_numpy(fx.mel_input(N))
  F = N // 256 + 1
  g = torch.randn(1, n_mel, F, generator=torch.Generator().manual_seed(n_mel))
  fwd, basis = constants64(n_mel)
  taco = tacos(n_mel)
  yg = y.to(DEV).requires_grad_(True)
  mel = taco.mel_spectrogram_differentiable(yg)
  assert mel.shape == (1, n_mel, F) and torch.equal(mel.detach(), taco.mel_spectrogram(y))
  (mel * g.to(DEV)).sum().backward()
  ref = mel_grad_ref64(y, g, fwd, basis)
  got = yg.grad.cpu()
  assert got.shape == ref.shape and torch.isfinite(got).all()
  err = float((got.double() - ref).norm() / ref.norm())
  print(f"mel gradient n_mel={n_mel}: rel L2 err {err:.2e} (|g_ref| {float(ref.norm()):.3e})")
  assert float(ref.norm()) > 0 and err <= GRAD_TOL


@pytest.fixture(scope="module")
def cls(fx):
  """(model, waveglow_amd.Denoiser) on the c64 weights the reference Denoiser of the fixture was built on."""
  from waveglow_amd import Denoiser
  hp = HParams(**dict(ast.literal_eval(str(fx.raw("cls/hp_json")))))
  model = build_model(hp, synthetic.make_state_dict(hp, seed=int(fx.raw("cls/weight_seed"))))
  return model, Denoiser(model, TSTFTHParams(), "zeros", DEV)


def test_denoiser_bias_chain_matches_reference(fx, cls):
  """Denoiser.__init__ link by link: infer(zeros, sigma 0) against the reference's bias audio at the flow's bar;
  bias_spec against the fp64 oracle magnitude of the GPU's own bias audio; the library transform of the REFERENCE's bias
  audio against the reference's bias_spec.  Measured on the MI355X: bias audio 1.4e-5 rms (signal 0.040); bias_spec vs the
  oracle of the GPU's own audio 1.3e-5 abs at 11.9; library transform of the reference's audio 2.7e-7 abs.  (End to end the
  GPU's bias_spec is 3.1e-3 abs from the reference's: the flow's error through a 1024-tap transform.)"""
  from oracle import stft_oracle as S
  model, den = cls
  ref_audio, ref_spec = fx.f32("cls/bias_audio"), fx.f32("cls/bias_spec")
  with torch.no_grad():
    bias_audio = model.infer(torch.zeros(1, 80, 88, device=DEV), sigma=0.0).float()
  torch.cuda.synchronize()
  assert bias_audio.shape == (1, 256 * 88) and torch.isfinite(bias_audio).all()
  err = rms(bias_audio.cpu() - torch.from_numpy(ref_audio))
  print(f"bias audio: rms err vs reference {err:.3e} (signal rms {rms(ref_audio):.4f})")
  assert err <= RMS_TOL
  assert den.bias_spec.shape == ref_spec.shape == (1, 513, 1)
  own = S.bias_spectrum(bias_audio.cpu().numpy(), S.bases()[0])
  got = den.bias_spec.cpu().numpy()[0, :, 0]
  print(f"bias_spec vs oracle of the GPU's bias audio: max abs {float(np.abs(got - own).max()):.2e}; "
        f"vs the reference's bias_spec: max abs {float(np.abs(got - ref_spec[0, :, 0]).max()):.2e} at max {float(ref_spec.max()):.2f}")
  np.testing.assert_allclose(got, own, rtol=MAG_TOL, atol=MAG_TOL)
  mag0 = torch.full((1, 513), float("nan"), dtype=torch.float32, device=DEV)
  den._run(torch.from_numpy(ref_audio).to(DEV), None, 0.0, None, mag0)
  torch.cuda.synchronize()
  print(f"library transform of the reference's bias audio vs its bias_spec: max abs "
        f"{float(np.abs(mag0.cpu().numpy()[0] - ref_spec[0, :, 0]).max()):.2e}")
  np.testing.assert_allclose(mag0.cpu().numpy()[0], ref_spec[0, :, 0], rtol=MAG_TOL, atol=MAG_TOL)


def test_denoiser_forward_matches_reference(fx, cls):
  """infer_with_noise of the stored mel and noise, then Denoiser.forward at both strengths, against the reference's
  Denoiser.forward of its own audio.  Measured on the MI355X: 1.2e-4 rms for the flow audio and for both denoised
  outputs; at s = 0.05 the output is 1.8e-3 from the reference's undenoised audio."""
  model, den = cls
  T = R.CLS_T
  mel = synthetic.make_mel(1, T, seed=int(fx.raw("cls/mel_seed"))).to(DEV)
  z_init = torch.from_numpy(fx.f32("cls/z_init")).to(DEV)
  z_early = [torch.from_numpy(fx.f32(f"cls/z_early_{k}")).to(DEV) for k in (4, 2)]
  with torch.no_grad():
    audio = model.infer_with_noise(mel, z_init, z_early, float(fx.raw("cls/sigma")))
  ref_audio = torch.from_numpy(fx.f32("cls/audio"))
  err = rms(audio.cpu() - ref_audio)
  print(f"flow audio: rms err vs reference {err:.3e} (signal rms {rms(ref_audio):.3f})")
  assert audio.shape == (1, 256 * T) and err <= RMS_TOL
  for s in R.CLS_STRENGTHS:
    out = den(audio, s)
    torch.cuda.synchronize()
    ref = torch.from_numpy(fx.cls_denoised(s))
    assert out.shape == ref.shape == (1, 1, 256 * T) and torch.isfinite(out).all()
    err_d, to_raw = rms(out.cpu() - ref), rms(out.cpu() - ref_audio[:, None, :])
    print(f"Denoiser.forward s={s}: rms err vs reference {err_d:.3e}; distance to the reference's undenoised audio "
          f"{to_raw:.3e} (the reference moved it by {rms(ref - ref_audio[:, None, :]):.3e})")
    assert err_d <= RMS_TOL
    if s == 0.05:
      assert err_d < to_raw            # nearer to what the reference's denoiser gave than to what it was given
