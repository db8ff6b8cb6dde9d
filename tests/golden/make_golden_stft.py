"""Golden vectors of the denoiser, the conv-STFT and the mel front-end from the REFERENCE's own classes (build
container only).

  python tests/golden/make_golden_stft.py

The reference's ``waveglow.stft`` imports four librosa names and librosa is not installed here.  ``_ref_import.
import_reference_stft`` puts functional stand-ins in their place (our own code, restated from librosa's documented
behaviour) and then imports the reference's own ``STFT`` (stft.py:98-203), ``TacotronSTFT`` (taco_stft.py:53-125) and
``Denoiser`` (denoiser.py:14-57), which run here on the CPU:

  pad_center(data, size=)        zero padding, (size - n) // 2 on the left; at the reference's hyper-parameters
                                 size == n, so it pads nothing
  tiny(x)                        np.finfo(x.dtype).tiny
  normalize(S, norm=None)        the identity
  filters.mel(sr=, n_fft=, n_mels=, fmin=, fmax=)
                                 waveglow_amd.taco_stft.slaney_mel_filterbank -- THE PROJECT'S RESTATEMENT

So the fixture pins everything the reference's classes compute -- the windowed bases, reflect padding, magnitude and
atan2 phase, ``window_sumsquare`` with its ``tiny`` threshold, the hop-ratio scale and the crop, the clamp of the
spectral subtraction, the bias from frame 0 of ``infer(zeros[1, 80, 88], sigma=0)``, ``dynamic_range_compression`` on the
detached magnitudes -- EXCEPT the values of the mel filter bank, which are the project's on both sides.  The same words
are stored in the fixture (``notes``).

Contents of tests/golden/stft_ref.npz: tests/_stft_ref.py.  Data only (inputs, and outputs of the reference's classes);
the archive is written with fixed time stamps, so two runs give the same bytes.
"""
import io
import os
import sys
import zipfile
import zlib

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.abspath(os.path.join(HERE, "..")))
sys.path.insert(0, os.path.abspath(os.path.join(HERE, "..", "..")))
from _ref_import import import_reference, import_reference_stft  # noqa: E402
import _stft_ref as R  # noqa: E402
from _corners import pack_f32, unpack_f32  # noqa: E402
from waveglow_amd.hparams import HParams  # noqa: E402
from waveglow_amd import synthetic  # noqa: E402

ref_model, ref_hparams, _ = import_reference()
ref_stft, ref_taco, ref_denoiser = import_reference_stft()
CPU = torch.device("cpu")
SIZE_LIMIT = os.path.getsize(os.path.join(HERE, "flow_corners.npz"))   # the largest fixture committed so far

NOTES = ("Outputs of the reference's own STFT, TacotronSTFT and Denoiser classes on the CPU (torch fp32), with functional "
         "stand-ins for librosa.util.pad_center / tiny / normalize(norm=None) and with librosa.filters.mel replaced by "
         "waveglow_amd.taco_stft.slaney_mel_filterbank: the mel basis is the PROJECT'S RESTATEMENT.  Pinned: everything "
         "these classes compute except the values of the mel filter bank.")


def quantise(x):
  """fp64 / fp32 samples in (-1, 1) -> int16 q with x' = q / 32768 exactly representable in fp32."""
  q = np.clip(np.rint(np.asarray(x, dtype=np.float64) * 32768.0), -32768, 32767).astype(np.int16)
  return q, torch.from_numpy(q.astype(np.float32) / np.float32(32768.0))


def denoise(stft, x, bias, strength):
  """denoiser.py:51-57 with a given bias; (out [B, 1, N], mag[:, :, 0])."""
  with torch.no_grad():
    mag, phase = stft.transform(x)
    out = stft.inverse(torch.clamp(mag - bias[None, :, None] * strength, 0.0), phase)
  return out.numpy(), mag[:, :, 0].numpy()


def denoise_part(out):
  stft = ref_stft.STFT(CPU, filter_length=1024, hop_length=256, win_length=1024)
  fb, ib = stft.forward_basis.numpy()[:, 0, :], stft.inverse_basis.numpy()[:, 0, :]
  assert fb.shape == ib.shape == (1026, 1024) and fb.dtype == np.float32
  rows = np.array(R.BASIS_ROWS)
  out["basis/rows"], out["basis/forward"], out["basis/inverse"] = rows, pack_f32(fb[rows]), pack_f32(ib[rows])
  # one bias for every case, so that the five lengths can also go through one ragged call (which takes one bias)
  bias = (1.0 + np.abs(np.random.default_rng(999).standard_normal(513)) * 5.0).astype(np.float32)
  out["den/bias"] = pack_f32(bias)
  stored = set()
  for name, T, B, strength, kind in R.denoise_cases():
    rng = np.random.default_rng(1000 + 10 * T + B)       # one input per (T, B): shared by its strengths
    q, x = quantise(0.3 * rng.standard_normal((B, 256 * T)))
    if kind == "zeros":
      x = torch.zeros_like(x)
    elif kind == "gap":
      q[:, 1000:3100] = 0
      x[:, 1000:3100] = 0.0
    y, mag0 = denoise(stft, x, torch.from_numpy(bias), strength)
    assert y.shape == (B, 1, 256 * T) and np.isfinite(y).all()
    src = R.denoise_input_key(T, B, kind)
    if src not in stored:                                # input and mag[:, :, 0] once per input
      stored.add(src)
      if kind != "zeros":
        out[f"{src}/x_q"] = q
      out[f"{src}/mag0"] = pack_f32(mag0)
    assert np.array_equal(unpack_f32(out[f"{src}/mag0"]), mag0)
    key = f"den/{name}"
    out[f"{key}/strength"] = np.array(strength, dtype=np.float64)
    is_zero = not y.any()
    out[f"{key}/out_is_zero"] = np.array(is_zero)
    if not is_zero:
      # the reconstruction is the input up to rounding: stored as its bits XOR the input's
      out[f"{key}/out"] = R.pack_xor(y, x.numpy()[:, None, :]) if R.denoise_out_is_xor(strength, kind) else pack_f32(y)
    # the reference gives exact zeros where every bin clamps (s = 1e4 with this bias) and for silence at s > 0, only there
    assert is_zero == (strength == 1e4 or (kind == "zeros" and strength > 0)), name
    print(f"{name}: out max abs {np.abs(y).max():.4f} rms {np.sqrt(np.mean(y.astype(np.float64) ** 2)):.4f}"
          f"{'  EXACT ZEROS' if is_zero else ''}")


def mel_part(out):
  N = R.MEL_LENGTHS[-1]
  rng = np.random.default_rng(7)
  x = rng.uniform(-0.8, 0.8, N) * np.linspace(0.2, 1.0, N)
  x[4000:6600] = 0.0                              # frames 18 ... 23 see silence only: |X| = 0, mel clamped at 1e-5
  q, x = quantise(x)
  out["mel/x_q"] = q
  floor = np.float32(np.log(np.float32(1e-5)))
  longest = None
  for n_mel in (80,) + R.MEL_ROWS_EXTRA:
    taco = ref_taco.TacotronSTFT(ref_taco.TSTFTHParams(n_mel_channels=n_mel), CPU)
    for n, m in sorted(R.mel_cases(), reverse=True):     # the longest first: the shorter ones are stored against it
      if m != n_mel:
        continue
      with torch.no_grad():
        mel = taco.mel_spectrogram(x[None, :n]).numpy()
      assert mel.shape == (1, n_mel, n // 256 + 1) and mel.dtype == np.float32
      if R.mel_is_xor(n, n_mel):
        out[f"mel/N{n}/m{n_mel}"] = R.pack_xor(mel, longest[:, :, :mel.shape[2]])
      else:
        out[f"mel/N{n}/m{n_mel}"] = pack_f32(mel)
        if (n, n_mel) == (R.MEL_LENGTHS[-1], 80):
          longest = mel
      print(f"mel N={n} n_mel={n_mel}: frames {mel.shape[2]}, {100.0 * np.mean(mel <= floor):.1f} % at log 1e-5, "
            f"max {mel.max():.3f}")


def class_part(out):
  """The reference Denoiser on the reference c64 model with the weights of tests/golden/c64.npz (make_golden.py)."""
  over = dict(n_channels=64, n_layers=4, n_flows=6, n_early_every=2)
  hp = HParams(**over)
  wseed = 5
  sd = synthetic.make_state_dict(hp, seed=wseed)
  crc = 0
  for key in sorted(sd):
    crc = zlib.crc32(sd[key].numpy().tobytes(), crc)
  c64 = np.load(os.path.join(HERE, "c64.npz"), allow_pickle=False)
  assert crc == int(c64["weights_crc32"]) and wseed == int(c64["weight_seed"])
  model = ref_model.WaveGlow.remove_weightnorm(ref_model.WaveGlow(ref_hparams.HParams(**over)))
  model.load_state_dict(sd)
  model = model.eval()
  torch.manual_seed(0)                   # sigma = 0 still draws: the noise only decides the sign of zeros
  den = ref_denoiser.Denoiser(model, ref_taco.TSTFTHParams(), "zeros", CPU)
  with torch.no_grad():
    torch.manual_seed(0)
    bias_audio = model.infer(torch.zeros(1, 80, ref_denoiser.BIAS_MEL_LENGTH), sigma=0.0)
    T, L = R.CLS_T, 32 * R.CLS_T
    mel = synthetic.make_mel(1, T, seed=R.CLS_MEL_SEED)
    # seed the global CPU RNG, let the reference draw, then replay the draws (make_golden.py)
    torch.manual_seed(R.CLS_NOISE_SEED)
    audio = model.infer(mel, sigma=R.CLS_SIGMA)
    torch.manual_seed(R.CLS_NOISE_SEED)
    out["cls/z_init"] = pack_f32(torch.FloatTensor(1, synthetic.flow_channels(hp)[-1], L).normal_().numpy())
    for k in reversed(range(hp.n_flows)):
      if k % hp.n_early_every == 0 and k > 0:
        out[f"cls/z_early_{k}"] = pack_f32(torch.FloatTensor(1, hp.n_early_size, L).normal_().numpy())
    assert den.bias_spec.shape == (1, 513, 1) and bias_audio.shape == (1, 256 * 88) and audio.shape == (1, 256 * T)
    out["cls/bias_spec"] = pack_f32(den.bias_spec.numpy())
    out["cls/bias_audio"] = pack_f32(bias_audio.numpy())
    out["cls/audio"] = pack_f32(audio.numpy())
    for s in R.CLS_STRENGTHS:
      y = den(audio, s).numpy()
      assert y.shape == (1, 1, 256 * T)
      out[f"cls/den_s{s}"] = R.pack_xor(y, audio.numpy()[:, None, :])     # bits XOR the undenoised audio's
      moved = np.sqrt(np.mean((y[0, 0].astype(np.float64) - audio[0].double().numpy()) ** 2))
      print(f"Denoiser.forward s={s}: moved the signal by {moved:.3e} rms (audio rms {float(audio.pow(2).mean().sqrt()):.3f})")
  out["cls/hp_json"] = np.array(repr(sorted(over.items())))
  out["cls/weight_seed"], out["cls/weights_crc32"] = np.array(wseed), np.array(crc, dtype=np.uint32)
  out["cls/sigma"], out["cls/mel_seed"] = np.array(R.CLS_SIGMA, dtype=np.float64), np.array(R.CLS_MEL_SEED)
  out["cls/noise_seed"] = np.array(R.CLS_NOISE_SEED)
  print(f"bias_spec max {float(den.bias_spec.max()):.3f}, bias audio rms {float(bias_audio.pow(2).mean().sqrt()):.4f}")


def write_npz(path, arrays):
  """np.savez_compressed with a fixed time stamp on every member: the same arrays give the same bytes."""
  with zipfile.ZipFile(path, "w", zipfile.ZIP_DEFLATED, compresslevel=9) as zf:
    for name, a in arrays.items():
      buf = io.BytesIO()
      np.lib.format.write_array(buf, np.asanyarray(a), allow_pickle=False)
      info = zipfile.ZipInfo(name + ".npy", date_time=(1980, 1, 1, 0, 0, 0))
      info.compress_type = zipfile.ZIP_DEFLATED
      info.external_attr = 0o644 << 16
      zf.writestr(info, buf.getvalue(), compresslevel=9)


if __name__ == "__main__":
  torch.set_num_threads(8)
  everything = {"notes": np.array(NOTES)}
  denoise_part(everything)
  mel_part(everything)
  class_part(everything)
  write_npz(R.FIXTURE, everything)
  size = os.path.getsize(R.FIXTURE)
  print("wrote", R.FIXTURE, size, "bytes (limit", SIZE_LIMIT, ")")
  assert size <= SIZE_LIMIT
