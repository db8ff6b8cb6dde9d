"""CPU: oracle/stft_oracle.py and ``waveglow_amd.denoiser.stft_bases`` answer to the reference.

tests/golden/stft_ref.npz (tests/golden/make_golden_stft.py, contents: tests/_stft_ref.py) holds outputs of the
reference's own ``STFT``, ``TacotronSTFT`` and ``Denoiser`` classes.  The fp64 oracle -- the yardstick of every GPU test of
the conv-STFT, the denoiser and the mel front-end -- must reproduce every one of them within ONE TENTH of the bar the GPU
tests hold the kernels to for the same quantity (tests/test_gpu_stft_ref.py), so that the two yardsticks of the GPU tests
cannot drift apart unnoticed:

  denoised audio, reconstruction           2e-6 max abs          (GPU bar 2e-5)
  log-mel                                  2e-5 max abs          (GPU bar 2e-4)
  mag[:, :, 0], bias_spec                  rtol = atol = 1e-5    (GPU bar 1e-4)
  Denoiser.forward on the flow audio       1e-5 max abs

Exact zeros of the reference are exact zeros of the oracle.  Not pinned by any of this: the values of the mel filter bank
(the fixture was made with the project's ``slaney_mel_filterbank`` in place of ``librosa.filters.mel``).

Measured (reference fp32 on the CPU vs the fp64 oracle): denoised audio <= 4.8e-7, log-mel <= 2.7e-6, mag[:, :, 0]
<= 2.0e-5 abs at values up to 22, bias_spec 3.7e-6 abs at 11.9, Denoiser.forward <= 1.3e-6; stft_bases rows within
0.77 x 2^-23 max|row|.  The two planted faults of DESIGN.md section 8 (bias from frame 1; a wrong window sum under the
first 512 output samples) fail test_bias_spec_matches_reference and test_denoise_matches_reference here.
"""
import numpy as np
import pytest
import torch

import _stft_ref as R
from oracle import stft_oracle as S

AUDIO_CAP, MEL_CAP, MAG_TOL, FORWARD_CAP = 2e-6, 2e-5, 1e-5, 1e-5


@pytest.fixture(scope="module")
def fx():
  return R.fixture()


@pytest.fixture(scope="module")
def bases():
  return S.bases()


def test_fixture_says_what_it_does_not_pin(fx):
  notes = str(fx.raw("notes"))
  assert "slaney_mel_filterbank" in notes and "RESTATEMENT" in notes
  assert tuple(int(r) for r in fx.raw("basis/rows")) == R.BASIS_ROWS


@pytest.mark.parametrize("name,T,B,strength,kind", R.denoise_cases(), ids=[c[0] for c in R.denoise_cases()])
def test_denoise_matches_reference(fx, bases, name, T, B, strength, kind):
  x = fx.denoise_input(name, T, B, kind).astype(np.float64)
  bias = fx.denoise_bias().astype(np.float64)
  ref, ref_is_zero = fx.denoise_expected(name, T, B, strength, kind)
  assert x.shape == ref.shape == (B, 256 * T)
  out = S.denoise(x, bias, strength, *bases)
  err = float(np.abs(out - ref).max())
  re, im = S.transform(x, bases[0])
  mag0 = np.sqrt(re ** 2 + im ** 2)[:, :, 0]
  mag0_ref = fx.denoise_mag0(T, B, kind)
  print(f"{name}: oracle vs reference max abs {err:.2e} (reference max {np.abs(ref).max():.3f}); "
        f"mag0 max abs {float(np.abs(mag0 - mag0_ref).max()):.2e} at max {float(mag0_ref.max()):.1f}")
  if ref_is_zero:
    assert not out.any()
  else:
    assert ref.any()
  assert err <= AUDIO_CAP
  np.testing.assert_allclose(mag0, mag0_ref, rtol=MAG_TOL, atol=MAG_TOL)
  if kind == "zeros":
    assert not mag0_ref.any() and not mag0.any()


@pytest.mark.parametrize("N,n_mel", R.mel_cases())
def test_mel_matches_reference(fx, N, n_mel):
  from waveglow_amd.taco_stft import slaney_mel_filterbank
  ref = fx.mel_expected(N, n_mel)
  out = S.mel_spectrogram(fx.mel_input(N), slaney_mel_filterbank(22050, 1024, n_mel, 0.0, 8000.0))
  assert out.shape == ref.shape == (1, n_mel, N // 256 + 1)
  err = float(np.abs(out - ref).max())
  floor = np.float32(np.log(np.float32(1e-5)))
  at_floor = ref == floor
  print(f"mel N={N} n_mel={n_mel}: oracle vs reference max abs {err:.2e}; {100 * at_floor.mean():.1f} % at log 1e-5")
  assert err <= MEL_CAP
  assert np.array_equal(at_floor, out == np.log(1e-5))        # the clamp branch is taken at the same places
  if N >= 16127:
    assert at_floor[:, :, 18:24].all() and 0.05 < at_floor.mean() < 0.2


def test_stft_bases_match_reference_rows(fx):
  """The reference rounds basis and window to fp32 and multiplies in fp32; the project multiplies in fp64 and rounds
  once: four half-ulp roundings in all, so each row agrees within 2^-23 of its largest value."""
  from waveglow_amd.denoiser import stft_bases
  fwd, inv, wsq = stft_bases()
  assert fwd.shape == inv.shape == (1026, 1024) and fwd.dtype == inv.dtype == wsq.dtype == np.float32
  assert fwd.flags.c_contiguous and inv.flags.c_contiguous
  rows = fx.raw("basis/rows")
  worst = 0.0
  for ours, key in ((fwd, "basis/forward"), (inv, "basis/inverse")):
    ref = fx.f32(key)
    assert ref.shape == (len(rows), 1024)
    for i, r in enumerate(rows):
      top = float(np.abs(ref[i]).max())
      err = float(np.abs(ours[r].astype(np.float64) - ref[i]).max())
      worst = max(worst, err / top) if top > 0 else worst
      assert err <= 2.0 ** -23 * top, (key, int(r), err, top)     # an all-zero row (sin(0 n)) must be all zero here too
  print(f"stft_bases rows vs reference: worst {worst / 2.0 ** -23:.2f} x 2^-23 max|row|")
  # the squared window (stft.py:45-95 builds it apart from the bases): the reference's fp32 window_sumsquare of one frame
  from scipy.signal import get_window
  assert np.array_equal(wsq, (get_window("hann", 1024, fftbins=True) ** 2).astype(np.float32))


def _bias_audio_oracle(fx):
  from _cases import oracle_cfg_from_hp
  from oracle import torch_oracle as O
  from waveglow_amd import synthetic
  from waveglow_amd.hparams import HParams
  import ast
  import zlib
  hp = HParams(**dict(ast.literal_eval(str(fx.raw("cls/hp_json")))))
  sd = synthetic.make_state_dict(hp, seed=int(fx.raw("cls/weight_seed")))
  crc = 0
  for key in sorted(sd):
    crc = zlib.crc32(sd[key].numpy().tobytes(), crc)
  assert crc == int(fx.raw("cls/weights_crc32"))
  L = 32 * 88
  z_early = {k: torch.zeros(1, hp.n_early_size, L) for k in range(hp.n_flows) if k % hp.n_early_every == 0 and k > 0}
  with torch.no_grad():
    return O.infer_ref(sd, torch.zeros(1, 80, 88), torch.zeros(1, 4, L), z_early, 0.0, oracle_cfg_from_hp(hp))


def test_bias_audio_matches_reference_bitwise(fx):
  """``infer(zeros[1, 80, 88], sigma=0)``: oracle/torch_oracle.infer_ref against the reference's, bit for bit like
  tests/test_oracle_golden.py::test_infer_matches_reference_bitwise."""
  torch.set_num_threads(8)
  audio = _bias_audio_oracle(fx)
  ref = torch.from_numpy(fx.f32("cls/bias_audio"))
  assert audio.shape == ref.shape == (1, 256 * 88)
  assert torch.equal(audio, ref), float((audio - ref).abs().max())


def test_bias_spec_matches_reference(fx, bases):
  """``Denoiser.bias_spec``: frame 0 of the transform of the bias audio (denoiser.py:45-49)."""
  ref = fx.f32("cls/bias_spec")
  assert ref.shape == (1, 513, 1)
  mag = S.bias_spectrum(fx.f32("cls/bias_audio"), bases[0])
  print(f"bias_spec: oracle vs reference max abs {float(np.abs(mag - ref[0, :, 0]).max()):.2e} at max {float(ref.max()):.2f}")
  np.testing.assert_allclose(mag, ref[0, :, 0], rtol=MAG_TOL, atol=MAG_TOL)


@pytest.mark.parametrize("strength", R.CLS_STRENGTHS)
def test_denoiser_forward_matches_reference(fx, bases, strength):
  """``Denoiser.forward`` on the flow's audio, the oracle's bias spectrum taken from the stored bias audio."""
  audio = fx.f32("cls/audio")
  ref = fx.cls_denoised(strength)
  assert audio.shape == (1, 256 * R.CLS_T) and ref.shape == (1, 1, 256 * R.CLS_T)
  bias = S.bias_spectrum(fx.f32("cls/bias_audio"), bases[0])
  out = S.denoise(audio.astype(np.float64), bias, strength, *bases)
  err = float(np.abs(out - ref[:, 0]).max())
  moved = float(np.sqrt(np.mean((ref[0, 0].astype(np.float64) - audio[0]) ** 2)))
  print(f"Denoiser.forward s={strength}: oracle vs reference max abs {err:.2e} (audio rms "
        f"{float(np.sqrt(np.mean(audio.astype(np.float64) ** 2))):.2f}, the reference moved it by {moved:.2e} rms)")
  assert err <= FORWARD_CAP
  assert moved > 0


def test_class_case_inputs_replay(fx):
  """The stored noise is what ``torch.manual_seed`` + the reference's draw order give here, and the stored audio is the
  oracle's ``infer_ref`` of the stored mel seed and noise, bit for bit: the GPU test injects the same tensors."""
  import ast
  from _cases import oracle_cfg_from_hp
  from oracle import torch_oracle as O
  from waveglow_amd import synthetic
  from waveglow_amd.hparams import HParams
  hp = HParams(**dict(ast.literal_eval(str(fx.raw("cls/hp_json")))))
  T, L = R.CLS_T, 32 * R.CLS_T
  assert (int(fx.raw("cls/mel_seed")), int(fx.raw("cls/noise_seed")), float(fx.raw("cls/sigma"))) == \
      (R.CLS_MEL_SEED, R.CLS_NOISE_SEED, R.CLS_SIGMA)
  z_init = torch.from_numpy(fx.f32("cls/z_init"))
  z_early = {k: torch.from_numpy(fx.f32(f"cls/z_early_{k}")) for k in (4, 2)}
  assert z_init.shape == (1, 4, L) and all(z.shape == (1, hp.n_early_size, L) for z in z_early.values())
  torch.set_num_threads(8)
  with torch.no_grad():
    audio = O.infer_ref(synthetic.make_state_dict(hp, seed=int(fx.raw("cls/weight_seed"))),
                        synthetic.make_mel(1, T, seed=R.CLS_MEL_SEED), z_init, z_early, R.CLS_SIGMA, oracle_cfg_from_hp(hp))
  assert torch.equal(audio, torch.from_numpy(fx.f32("cls/audio")))
