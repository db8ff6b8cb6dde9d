"""The resampler without a GPU: the definition (tests/_resample_oracle.py) against ``scipy.signal.resample_poly``, the plan,
the C entry points' argument checks, the parser's new flags, and that nothing changes where the feature is not asked for."""
import ctypes as C

import numpy as np
import pytest
import torch

import _resample_oracle as oracle
from waveglow_amd import _lib, build
from waveglow_amd import resample as rs

LENGTHS = (1, 3, 513, 1499)


@pytest.fixture(scope="module")
def lib():
  build.build_library()
  return _lib.load()


@pytest.mark.parametrize("up,down", oracle.RATIOS)
def test_oracle_equals_resample_poly(up, down):
  """Within 1e-12 max|x| of scipy on fp64 input (the summation orders may differ); the output lengths are equal."""
  from scipy.signal import resample_poly
  rng = np.random.default_rng(100 * up + down)
  for n in LENGTHS:
    x = rng.uniform(-0.9, 0.9, n).astype(np.float32)
    ref = resample_poly(x.astype(np.float64), up, down)
    got = oracle.resample(x, up, down)
    assert got.shape == ref.shape == (oracle.out_len(n, up, down),)
    err = float(np.max(np.abs(got - ref)))
    print(f"{up}/{down} n={n}: max |oracle - scipy| = {err:.3e}")
    assert err <= 1e-12 * float(np.max(np.abs(x)))


@pytest.mark.parametrize("up,down", [(147, 320), (320, 147), (441, 320)])
def test_impulse_returns_the_taps_bit_for_bit(up, down):
  from scipy.signal import resample_poly
  m0, n_in = 137, 300
  x = np.zeros(n_in)
  x[m0] = 1.0
  half, h = oracle.taps(up, down)
  idx = half + np.arange(oracle.out_len(n_in, up, down)) * down - m0 * up
  want = np.where((idx >= 0) & (idx <= 2 * half), h[np.clip(idx, 0, 2 * half)], 0.0)
  assert np.array_equal(oracle.resample(x, up, down), want)
  assert np.array_equal(resample_poly(x, up, down), want)


def test_plan():
  up, down, half, taps = rs.resample_plan(48000, 22050)
  assert (up, down, half) == (147, 320, 3200) and taps.shape == (6401,) and taps.dtype == np.float64
  assert np.array_equal(taps, oracle.taps(147, 320)[1])
  assert rs.resample_plan(48000, 22050)[3] is taps                               # cached per ratio
  assert rs.resample_plan(96000, 44100)[3] is taps
  assert rs.resample_plan(22050, 48000)[:3] == (320, 147, 3200)
  up, down, half, taps = rs.resample_plan(22050, 22050)
  assert (up, down, half) == (1, 1, 0) and taps.tolist() == [1.0]
  for r in (8000, 11025, 16000, 24000, 32000, 44100, 48000, 88200, 96000):
    rs.resample_plan(r, 22050)
    rs.resample_plan(22050, r)
  for bad in ((192000, 22050), (22050, 192000), (0, 22050), (22050, 0), (-48000, 22050), (22050.5, 48000),
              (48000, "22050"), (None, 22050), (True, 22050)):
    with pytest.raises(_lib.WgError):
      rs.resample_plan(*bad)


def test_polyphase_table_holds_every_tap_once():
  up, down, half, taps = rs.resample_plan(16000, 22050)
  table = rs.polyphase_table(up, half, taps)
  K = -(-(2 * half + 1) // up)
  assert table.shape == (up, K) and table.dtype == np.float64 and table.flags.c_contiguous
  for p in (0, 1, up - 1):
    for j in (0, 1, K - 1):
      i = p + (K - 1 - j) * up
      assert table[p, j] == (taps[i] if i <= 2 * half else 0.0)


def test_out_len():
  assert rs.out_len(0, 147, 320) == 0
  assert rs.out_len(320, 147, 320) == 147 and rs.out_len(640, 147, 320) == 294          # multiples
  assert rs.out_len(321, 147, 320) == 148 and rs.out_len(1, 147, 320) == 1 and rs.out_len(319, 147, 320) == 147
  assert rs.out_len(147, 320, 147) == 320 and rs.out_len(1, 320, 147) == 3 and rs.out_len(100, 320, 147) == 218
  assert rs.out_len(7, 1, 1) == 7 and rs.out_len(7, 1, 2) == 4 and rs.out_len(7, 2, 1) == 14
  for up, down in oracle.RATIOS:
    for n in (0, 1, 2, 513, 1499, 2 ** 26):
      assert rs.out_len(n, up, down) == oracle.out_len(n, up, down)


def test_entry_points_validate_arguments_without_a_gpu(lib):
  """wg_resample's argument checks run before any device work: bad ratios and sizes are reported, not crashed on."""
  n_out, K, tile, staged = C.c_int32(), C.c_int32(), C.c_int32(), C.c_int32()
  assert lib.wg_resample_plan(147, 320, 3200, 48000, C.byref(n_out), C.byref(K), C.byref(tile), C.byref(staged)) == 0
  assert (n_out.value, K.value, tile.value, staged.value) == (22050, 44, rs.TILE, 1)
  assert lib.wg_resample_plan(1, 1, 0, 5, C.byref(n_out), C.byref(K), None, None) == 0 and (n_out.value, K.value) == (5, 1)
  assert lib.wg_resample_plan(147, 1280, 12800, 48000, None, None, None, None) == -1 and b"1024" in lib.wg_last_error()
  # the variant follows the ratio: 1023 down / up + K + 1 samples of a tile against the 8192 that are staged
  assert rs.kernel_plan(96000, 22050) == (88, rs.TILE, True) and rs.kernel_plan(7, 1)[2] is True       # 147/640, 1/7
  assert rs.kernel_plan(8, 1) == (161, rs.TILE, False) and rs.kernel_plan(16, 1) == (321, rs.TILE, False)
  assert rs.kernel_plan(1, 16)[2] is True and rs.kernel_plan(22050, 22050) == (1, rs.TILE, False)
  dummy = (C.c_char * 64)()
  p = C.addressof(dummy)

  def call(in_=p, dtype=_lib.WG_PCM_F32, lens=p, out=p, taps=p, up=147, down=320, half=3200, flags=0, B=1, n_in=320,
           n_out=147):
    return lib.wg_resample(in_, dtype, lens, out, taps, up, down, half, flags, B, n_in, n_out, None)

  for kw, word in (({"in_": None}, b"null"), ({"lens": None}, b"null"), ({"out": None}, b"null"), ({"taps": None}, b"null"),
                   ({"dtype": 2}, b"in_dtype"), ({"flags": 2}, b"flags"), ({"B": 0}, b"B >= 1"),
                   ({"up": 0}, b"up >= 1"), ({"down": 0}, b"down >= 1"), ({"up": -147}, b"up >= 1"),
                   ({"up": 294, "down": 640}, b"gcd"), ({"up": 147, "down": 1280, "half": 10240}, b"1024"),
                   ({"up": 1025, "down": 1}, b"1024"), ({"half": -1}, b"half"), ({"half": 10241}, b"half"),
                   ({"n_in": 0}, b"n_in"), ({"n_in": 2 ** 26 + 1}, b"n_in"), ({"n_out": 146}, b"n_out"),
                   ({"n_out": 2 ** 31 - 1}, b"n_out"), ({"n_out": 2 ** 31 - 1024}, b"n_out"),
                   ({"up": 1024, "down": 1, "half": 10240, "n_in": 2 ** 26, "n_out": 2 ** 31 - 1}, b"31 bits")):
    assert call(**kw) == -1, kw
    assert word in lib.wg_last_error(), (kw, lib.wg_last_error())


def test_python_surface_refuses_without_a_gpu():
  x = torch.zeros((2, 100))
  with pytest.raises(_lib.WgError, match="GPU"):
    rs.resample(x, None, 48000, 22050)
  with pytest.raises(_lib.WgError, match="GPU"):
    rs.resample_enqueue(x, torch.zeros(2, dtype=torch.int32), 48000, 22050)
  assert rs.check_lengths(None, 2, 100) == [100, 100]
  assert rs.check_lengths(torch.tensor([0, 100]), 2, 100) == [0, 100] and rs.check_lengths((5, 6), 2, 100) == [5, 6]
  for bad in ([101, 5], [-1, 5], [5], [5, 6, 7], [5.0, 6], torch.tensor([5.0, 6.0]), 5, np.array([5, 6])):
    with pytest.raises(_lib.WgError):
      rs.check_lengths(bad, 2, 100)
  import waveglow_amd
  assert waveglow_amd.resample_plan is rs.resample_plan and waveglow_amd.out_len is rs.out_len
  assert waveglow_amd.resample_enqueue is rs.resample_enqueue and waveglow_amd.resample.resample is rs.resample


def test_without_the_flag_a_48k_file_is_still_refused(tmp_path):
  from scipy.io.wavfile import write
  from waveglow_amd.device_data import DeviceWavPool
  from waveglow_amd.hparams import HParams
  from waveglow_amd.taco_stft import TacotronSTFT
  from waveglow_amd.training import Entry
  path = tmp_path / "a.wav"
  write(path, 48000, (np.arange(2000) % 100 * 50).astype(np.int16))
  hp = HParams()
  with pytest.raises(ValueError, match="48000Hz"):
    DeviceWavPool([Entry("a", "a.wav", path)], hp, "cuda:0")
  taco = TacotronSTFT.__new__(TacotronSTFT)                  # the constructor needs the GPU; the rate check does not
  torch.nn.Module.__init__(taco)
  taco.sampling_rate, taco.resample_inputs = hp.sampling_rate, False
  with pytest.raises(ValueError, match="48000Hz"):
    taco.get_wav_tensor_from_file(path)
  import inspect
  from waveglow_amd.device_data import DeviceBatchLoader
  from waveglow_amd.synthesizer import Synthesizer
  from waveglow_amd.training import train
  from waveglow_amd.validation import validate
  for fn in (TacotronSTFT.__init__, DeviceWavPool.__init__, DeviceBatchLoader.__init__, train, validate):
    assert inspect.signature(fn).parameters["resample_inputs"].default is False
  assert inspect.signature(Synthesizer.infer_batch_pcm).parameters["output_sampling_rate"].default is None


def test_cli_knows_the_new_flags_and_they_default_to_off():
  from waveglow_amd.cli import build_parser
  p = build_parser()
  for cmd in (["synthesize-wav", "c.pt", "d"], ["validate", "c", "o", "d"], ["train", "a", "b", "c"],
              ["continue-train", "a", "b", "c"]):
    assert p.parse_args(cmd).resample_inputs is False
    assert p.parse_args(cmd + ["--resample-inputs"]).resample_inputs is True
  for cmd in (["synthesize", "c.pt", "d"], ["synthesize-wav", "c.pt", "d"]):
    assert p.parse_args(cmd).output_sampling_rate is None
    assert p.parse_args(cmd + ["--output-sampling-rate", "16000"]).output_sampling_rate == 16000
