"""The cases of tests/golden/stft_ref.npz (written by tests/golden/make_golden_stft.py from the reference's own ``STFT``,
``TacotronSTFT`` and ``Denoiser`` classes) and its reader, shared by the generator, tests/test_stft_ref_cpu.py and
tests/test_gpu_stft_ref.py.

Keys of the fixture (fp32 arrays are stored as byte planes: tests/_corners.py pack_f32, lossless):

  notes                          what the fixture pins and what it does not
  basis/rows, basis/forward, basis/inverse
                                 16 rows of the reference's ``forward_basis`` / ``inverse_basis`` buffers
  den/bias                       the bias magnitudes [513], 1 + 5 |randn|: one for every case
  den/in/<input>/x_q             int16 input, x = q / 32768 (exact in fp32); absent for the all-zero inputs.  One input
                                 serves every strength of a (T, B)
  den/in/<input>/mag0            ``mag[:, :, 0]`` [B, 513]
  den/<case>/strength            fp64 scalar
  den/<case>/out                 ``stft.inverse(clamp(mag - bias * s, 0), phase)`` [B, 1, N]; absent where it is exactly 0
  den/<case>/out_is_zero         the reference's output was exactly 0 everywhere (then ``out`` is not stored)
  mel/x_q                        int16 buffer of MEL_LENGTHS[-1] samples; every mel input is a prefix of it
  mel/N<N>/m<n_mel>              ``TacotronSTFT.mel_spectrogram`` [1, n_mel, N // 256 + 1]
  cls/...                        the reference ``Denoiser`` on the c64 model (see make_golden_stft.py)

Three kinds of output are almost another array of the fixture and are stored as their bits XOR that array's (pack_xor;
lossless whatever the values are, and most bytes come out zero): the reconstructions (s = 0) against their input, the 80-row
log-mels of the shorter lengths against the leading frames of the longest's, ``Denoiser.forward`` against its input audio.
"""
import os

import numpy as np

from _corners import pack_f32, unpack_f32

FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "stft_ref.npz")

# rows of the [1026, 1024] bases: 0 DC real, 512 Nyquist real, 513 DC imaginary, 1025 Nyquist imaginary, both sides of the
# real | imaginary boundary at 512 | 513, and a spread of ordinary rows of both halves
BASIS_ROWS = (0, 1, 2, 255, 256, 257, 511, 512, 513, 514, 515, 769, 770, 1023, 1024, 1025)

# frames T (audio 256 T, F = T + 1): 4 the minimum (the reflected ends meet), 28 / 29 -> F + 3 = 32 / 33 (the inverse
# kernel's tile edge), 32 -> F = 33 (the forward kernel's; 31 is in test_gpu_ragged_post.py), 64 -> F = 65
DENOISE_T = (4, 28, 29, 32, 64)
DENOISE_T_EXTRA = (4, 32)       # also: s = 0, s = 1e4, silence at s = 0.1 and s = -0.1
RAGGED_ORDER = (28, 64, 4, 32, 29)   # the one ragged call: the longest is not first

MEL_LENGTHS = (513, 16127, 16128, 16383, 16384)     # F = 3, 63, 64, 64, 65: the 64-frame block edge, both hop remainders
MEL_ROWS_EXTRA = (1, 5, 127, 128)                   # the four-way split of mel rows with a remainder, and its limit
MEL_LENGTHS_EXTRA = (513, 16128)

CLS_STRENGTHS = (0.0005, 0.05)
CLS_T, CLS_SIGMA, CLS_MEL_SEED, CLS_NOISE_SEED = 23, 0.8, 3, 4321 + 23


def denoise_cases():
  """[(name, T, B, strength, input kind)] in the fixture's order; kind is "randn", "zeros" or "gap"."""
  out = []
  for T in DENOISE_T:
    out.append((f"T{T}_s0.1", T, 1, 0.1, "randn"))
    if T in DENOISE_T_EXTRA:
      out.append((f"T{T}_s0", T, 1, 0.0, "randn"))
      out.append((f"T{T}_s1e4", T, 1, 1e4, "randn"))
      out.append((f"T{T}_zeros_s0.1", T, 1, 0.1, "zeros"))
      out.append((f"T{T}_zeros_s-0.1", T, 1, -0.1, "zeros"))
  out.append(("T16_gap_s0.02", 16, 1, 0.02, "gap"))       # samples 1000 ... 3099 are zero
  out.append(("T5_b3_s0.1", 5, 3, 0.1, "randn"))          # the one batched case: the batch stride
  return out


def mel_cases():
  """[(N, n_mel)]"""
  out = [(N, 80) for N in MEL_LENGTHS]
  out += [(N, m) for N in MEL_LENGTHS_EXTRA for m in MEL_ROWS_EXTRA]
  return out


def denoise_input_key(T, B, kind):
  return f"den/in/T{T}_b{B}_{kind}"


def denoise_out_is_xor(strength, kind):
  return strength == 0.0 and kind == "randn"


def mel_is_xor(N, n_mel):
  return n_mel == 80 and N != MEL_LENGTHS[-1]


def pack_xor(a, base):
  """fp32 ``a`` as byte planes of its bits XOR those of ``base`` (broadcast to a's shape); unpack_xor undoes it."""
  a = np.ascontiguousarray(a, dtype=np.float32)
  base = np.ascontiguousarray(np.broadcast_to(np.asarray(base, dtype=np.float32), a.shape))
  return pack_f32((a.view(np.uint32) ^ base.view(np.uint32)).view(np.float32))


def unpack_xor(u, base):
  d = unpack_f32(u)
  base = np.ascontiguousarray(np.broadcast_to(np.asarray(base, dtype=np.float32), d.shape))
  return (d.view(np.uint32) ^ base.view(np.uint32)).view(np.float32)


class Fixture:
  def __init__(self, path=FIXTURE):
    self.z = np.load(path, allow_pickle=False)

  def __contains__(self, key):
    return key in self.z.files

  def raw(self, key):
    return self.z[key]

  def f32(self, key):
    return unpack_f32(self.z[key])

  def audio(self, key):
    """int16 -> fp32, exactly q / 32768."""
    q = self.z[key]
    assert q.dtype == np.int16
    return q.astype(np.float32) / np.float32(32768.0)

  def denoise_input(self, name, T, B, kind):
    if kind == "zeros":
      return np.zeros((B, 256 * T), dtype=np.float32)
    return self.audio(f"{denoise_input_key(T, B, kind)}/x_q")

  def denoise_bias(self):
    return self.f32("den/bias")

  def denoise_mag0(self, T, B, kind):
    return self.f32(f"{denoise_input_key(T, B, kind)}/mag0")

  def denoise_expected(self, name, T, B, strength, kind):
    """(out [B, 256 T] fp32, whether the reference's output was exactly zero)."""
    assert float(self.z[f"den/{name}/strength"]) == strength
    if bool(self.z[f"den/{name}/out_is_zero"]):
      return np.zeros((B, 256 * T), dtype=np.float32), True
    if denoise_out_is_xor(strength, kind):
      return unpack_xor(self.z[f"den/{name}/out"], self.denoise_input(name, T, B, kind)[:, None, :])[:, 0, :], False
    return self.f32(f"den/{name}/out")[:, 0, :], False

  def mel_input(self, N):
    return self.audio("mel/x_q")[None, :N]

  def mel_expected(self, N, n_mel):
    """[1, n_mel, N // 256 + 1]"""
    u = self.z[f"mel/N{N}/m{n_mel}"]
    if mel_is_xor(N, n_mel):
      return unpack_xor(u, self.mel_expected(MEL_LENGTHS[-1], 80)[:, :, :N // 256 + 1])
    return unpack_f32(u)

  def cls_denoised(self, strength):
    """``Denoiser.forward(cls/audio, strength)`` [1, 1, 5888]"""
    return unpack_xor(self.z[f"cls/den_s{strength}"], self.f32("cls/audio")[:, None, :])


_fx = None


def fixture():
  global _fx
  if _fx is None:
    _fx = Fixture()
  return _fx
