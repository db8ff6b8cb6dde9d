"""The device resampler (``wg_resample``, waveglow_amd/resample.py) and what is built on it: the opt-in input side of the
mel front-end and the wav pool, the output rate of ``infer_batch_pcm`` and the CLI flags.

Against ``scipy.signal.resample_poly`` on the fp64 copy of the crop the bound is
    |y_dev - y_ref| <= 2^-24 |y_ref| + 1e-12 max|x| L,
L the largest polyphase branch's L1 norm (1.6 .. 2.3 here).  The first term is the one fp32 rounding the device makes; the
second is about 50 times the bound K 2^-53 sum|x h| on the difference of two fp64 summation orders of K <= 88 terms.  Both
are derived, not measured.  Everything else in this file is bit for bit: against tests/_resample_oracle.py, whose sum runs
in the kernel's order, between a row of a batch and its own call, and between the layers built on the resampler and the
resampler itself."""
import functools

import numpy as np
import pytest
import torch

import _resample_oracle as oracle
from waveglow_amd import _lib, synthetic
from waveglow_amd import resample as rs
from waveglow_amd.audio import convert_wav, normalize_wav
from waveglow_amd.hparams import HParams
from waveglow_amd.model import WaveGlow

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
RAGGED = (1, 700, 1023, 1500)
PITCH = 1500
SR = 22050


def _rates(up, down):
  """sampling rates (sr_in, sr_out) whose reduced ratio is up / down"""
  return 100 * down, 100 * up


@functools.lru_cache(maxsize=None)
def _noise():
  return np.random.default_rng(42).uniform(-0.9, 0.9, PITCH).astype(np.float32)


def _batch(x, lens, pitch, fill=np.nan):
  out = np.full((len(lens), pitch), fill, np.float32)
  for b, n in enumerate(lens):
    out[b, :n] = x[:n]
  return torch.from_numpy(out).to(DEV)


@functools.lru_cache(maxsize=None)
def _ragged(up, down):
  """the ragged batch of the noise through up / down, computed once: (device result on the host, output lengths)"""
  out, lens = rs.resample(_batch(_noise(), RAGGED, PITCH), list(RAGGED), *_rates(up, down))
  return out.cpu().numpy(), lens


@pytest.mark.parametrize("up,down", oracle.RATIOS)
def test_ragged_batch_against_scipy(up, down):
  from scipy.signal import resample_poly
  x = _noise()
  got, lens = _ragged(up, down)
  assert got.dtype == np.float32 and got.shape == (4, oracle.out_len(PITCH, up, down))
  assert lens == [oracle.out_len(n, up, down) for n in RAGGED]
  assert not np.isnan(got).any()
  L = oracle.branch_l1(up, down)
  assert 1.6 <= L <= 2.3
  for b, n in enumerate(RAGGED):
    ref = resample_poly(x[:n].astype(np.float64), up, down)
    assert ref.shape == (lens[b],)
    tol = 2.0 ** -24 * np.abs(ref) + 1e-12 * float(np.max(np.abs(x[:n]))) * L
    y = got[b, :lens[b]].astype(np.float64)
    emu = oracle.resample_device(x[:n], up, down)
    print(f"{up}/{down} len {n}: max |dev - scipy| / tol = {float(np.max(np.abs(y - ref) / tol)):.3f}, "
          f"|oracle - scipy| / tol = {float(np.max(np.abs(emu.astype(np.float64) - ref) / tol)):.3f}, "
          f"dev != oracle at {int(np.count_nonzero(emu != got[b, :lens[b]]))} samples")
    assert np.all(np.abs(y - ref) <= tol)
    assert np.all(np.abs(emu.astype(np.float64) - ref) <= tol)
    assert np.array_equal(got[b, :lens[b]], emu)                     # the oracle's emulation: a difference of 0
    assert not got[b, lens[b]:].any()                                # exactly 0 behind out_len


@pytest.mark.parametrize("up,down", [(147, 320), (320, 147), (441, 320)])
def test_impulse_returns_the_taps_bit_for_bit(up, down):
  m0, n_in = 137, 300
  x = np.zeros((1, n_in), np.float32)
  x[0, m0] = 1.0
  out, lens = rs.resample(torch.from_numpy(x).to(DEV), None, *_rates(up, down))
  half, h = oracle.taps(up, down)
  idx = half + np.arange(lens[0]) * down - m0 * up
  want = np.where((idx >= 0) & (idx <= 2 * half), h[np.clip(idx, 0, 2 * half)], 0.0).astype(np.float32)
  assert lens == [oracle.out_len(n_in, up, down)] and np.count_nonzero(want) >= 20
  assert np.array_equal(out.cpu().numpy()[0], want)


def _len_for(n_out, up, down):
  """the smallest input length with out_len == n_out"""
  n = (n_out * down) // up
  while oracle.out_len(n, up, down) < n_out:
    n += 1
  while n > 0 and oracle.out_len(n - 1, up, down) >= n_out:
    n -= 1
  assert oracle.out_len(n, up, down) == n_out
  return n


@pytest.mark.parametrize("up,down", [(147, 320), (5, 4)])
def test_tile_edges_and_refused_lengths(up, down):
  """out_len of TILE - 1, TILE, TILE + 1 and 2 TILE + 1, a row of length 0, and device-side lengths of -1 and n_in + 1.
  The up-sampling ratio is 5 / 4, which reaches all four (from 818, 819, 820 and 1639 samples); 320 / 147 skips 1023 and
  1025."""
  T = rs.TILE
  assert rs.kernel_plan(*_rates(up, down))[1:] == (T, True)
  lens = [_len_for(n, up, down) for n in (T - 1, T, T + 1, 2 * T + 1)] + [0]
  N = max(lens)
  x = np.random.default_rng(7).uniform(-0.9, 0.9, N).astype(np.float32)
  audio = _batch(x, lens, N)
  out, out_lens = rs.resample(audio, lens, *_rates(up, down))
  out = out.cpu().numpy()
  assert out_lens == [T - 1, T, T + 1, 2 * T + 1, 0]
  assert not np.isnan(out).any()
  for b, n in enumerate(lens):
    if n:
      assert np.array_equal(out[b, :out_lens[b]], oracle.resample_device(x[:n], up, down)), b
      single, single_len = rs.resample(audio[b:b + 1, :n].contiguous(), None, *_rates(up, down))
      assert single_len == [out_lens[b]] and np.array_equal(single.cpu().numpy()[0], out[b, :out_lens[b]])
    assert not out[b, out_lens[b]:].any()
  bad = torch.tensor([-1, N + 1, lens[2], lens[3], 0], dtype=torch.int32).to(DEV)
  got = rs.resample_enqueue(audio, bad, *_rates(up, down)).cpu().numpy()
  assert got.shape == out.shape and not got[0].any() and not got[1].any() and not got[4].any()
  assert np.array_equal(got[2], out[2]) and np.array_equal(got[3], out[3])


@pytest.mark.parametrize("up,down", [(1, 8), (1, 16)])
def test_samples_read_through_the_cache(up, down):
  """Ratios with down / up of 8 and more do not stage their samples in LDS (asserted through ``kernel_plan``): the same
  ragged batch, fp32 with NaN and int16 with full-scale samples behind every length.  Bit for bit against the oracle and
  each row's own B = 1 call, and within the file's bound against scipy -- with K = 161 / 321 terms the summation-order
  term K 2^-53 sum|x h| <= 321 * 1.1e-16 max|x| L = 3.6e-14 max|x| L is still 28 times below 1e-12 max|x| L."""
  from scipy.signal import resample_poly
  rates = _rates(up, down)
  K, tile, staged = rs.kernel_plan(*rates)
  assert (K, tile, staged) == (20 * down + 1, rs.TILE, False)
  assert rs.kernel_plan(100 * 7, 100)[2] is True                     # 1 / 7 is the last ratio of this kind that stages
  pcm = np.random.default_rng(5).integers(-29491, 29492, PITCH).astype(np.int16)      # peak 0.9
  x = pcm.astype(np.float32) / np.float32(32768)
  audio = _batch(x, RAGGED, PITCH)
  padded = np.full((len(RAGGED), PITCH), 32767, np.int16)
  for b, n in enumerate(RAGGED):
    padded[b, :n] = pcm[:n]
  got, lens = rs.resample(audio, list(RAGGED), *rates)
  got16, lens16 = rs.resample(torch.from_numpy(padded).to(DEV), list(RAGGED), *rates)
  got, got16 = got.cpu().numpy(), got16.cpu().numpy()
  assert lens == lens16 == [oracle.out_len(n, up, down) for n in RAGGED]
  assert got.shape == (4, oracle.out_len(PITCH, up, down)) and not np.isnan(got).any()
  assert np.array_equal(got16, got)
  L = oracle.branch_l1(up, down)
  for b, n in enumerate(RAGGED):
    y = got[b, :lens[b]]
    assert np.array_equal(y, oracle.resample_device(x[:n], up, down)), (b, "oracle")
    assert not got[b, lens[b]:].any()
    ref = resample_poly(x[:n].astype(np.float64), up, down)
    tol = 2.0 ** -24 * np.abs(ref) + 1e-12 * float(np.max(np.abs(x[:n]))) * L
    print(f"{up}/{down} len {n}: max |dev - scipy| / tol = {float(np.max(np.abs(y.astype(np.float64) - ref) / tol)):.3f}")
    assert ref.shape == y.shape and np.all(np.abs(y.astype(np.float64) - ref) <= tol)
    for src in (audio[b:b + 1, :n], torch.from_numpy(padded[b:b + 1, :n]).to(DEV)):
      single, sl = rs.resample(src.contiguous(), None, *rates)
      assert sl == [lens[b]] and np.array_equal(single.cpu().numpy()[0], y), (b, src.dtype)


def test_determinism_rows_int16_and_identity():
  up, down = 147, 320
  first, lens = _ragged(up, down)
  audio = _batch(_noise(), RAGGED, PITCH)
  again, _ = rs.resample(audio, torch.tensor(RAGGED), *_rates(up, down))
  assert np.array_equal(again.cpu().numpy(), first)                  # the same bits twice
  for b, n in enumerate(RAGGED):                                     # every row: its own B = 1, n_in = len call
    single, sl = rs.resample(audio[b:b + 1, :n].contiguous(), None, *_rates(up, down))
    assert sl == [lens[b]] and single.shape == (1, lens[b])
    assert np.array_equal(single.cpu().numpy()[0], first[b, :lens[b]])
  pcm = np.random.default_rng(3).integers(-32768, 32768, (2, PITCH)).astype(np.int16)
  pcm[0, :4] = (-32768, 32767, 0, -1)
  as_float = (pcm.astype(np.float32) / np.float32(32768))
  for ratio in ((147, 320), (320, 147), (1, 1)):
    a, la = rs.resample(torch.from_numpy(pcm).to(DEV), [PITCH, 777], *_rates(*ratio))
    f, lf = rs.resample(torch.from_numpy(as_float).to(DEV), [PITCH, 777], *_rates(*ratio))
    assert la == lf and np.array_equal(a.cpu().numpy(), f.cpu().numpy())
  # 1 / 1: the input bits (-0 and a NaN behind the length included) and zeros behind the length
  x = _noise().copy()
  x[5] = -0.0
  same, ls = rs.resample(_batch(x, (PITCH, 700), PITCH), (PITCH, 700), SR, SR)
  same = same.cpu().numpy()
  assert ls == [PITCH, 700] and same.shape == (2, PITCH)
  assert np.array_equal(same[0].view(np.uint32), x.view(np.uint32))
  assert np.array_equal(same[1, :700].view(np.uint32), x[:700].view(np.uint32)) and not same[1, 700:].any()
  with pytest.raises(_lib.WgError):
    rs.resample(torch.zeros((2, 100)), None, 48000, SR)                               # a CPU tensor
  for bad in (torch.zeros((2, 100), dtype=torch.float64, device=DEV), torch.zeros(100, device=DEV),
              torch.zeros((1, 2, 100), device=DEV)):
    with pytest.raises(_lib.WgError):
      rs.resample(bad, None, 48000, SR)
  with pytest.raises(_lib.WgError):
    rs.resample(torch.zeros((2, 100), device=DEV), [100, 101], 48000, SR)
  with pytest.raises(_lib.WgError):
    rs.resample(torch.zeros((2, 100), device=DEV), None, 192000, SR)


def test_clip_is_np_clip_of_the_unclipped_result():
  n = 1470
  square = np.where((np.arange(n) // 37) % 2 == 0, 1.0, -1.0).astype(np.float32)
  x = torch.from_numpy(square[None]).to(DEV)
  plain, lens = rs.resample(x, None, 14700, 32000)                                    # 320 / 147
  clipped, lens_c = rs.resample(x, None, 14700, 32000, clip=True)
  plain, clipped = plain.cpu().numpy(), clipped.cpu().numpy()
  print(f"full-scale square wave through 320/147: min {plain.min():.4f} max {plain.max():.4f}")
  assert lens == lens_c == [3200]
  assert plain.max() > 1.0 and plain.min() < -1.0
  assert clipped.max() == 1.0 and clipped.min() == -1.0
  assert np.array_equal(clipped, np.clip(plain, np.float32(-1), np.float32(1)))


# ---------------------------------------------------------------- what is built on the resampler
FILES = (("a_48k", 48000, 6000), ("b_22k", SR, 3000), ("c_16k", 16000, 2500))      # sorted by name: rates in mixed order


@pytest.fixture(scope="module")
def wav_folder(tmp_path_factory):
  from scipy.io.wavfile import write
  folder = tmp_path_factory.mktemp("resample_wavs")
  rng = np.random.default_rng(11)
  data = {}
  for name, sr, n in FILES:
    data[name] = rng.integers(-30000, 30001, n).astype(np.int16)
    write(folder / f"{name}.wav", sr, data[name])
  return folder, data


@pytest.fixture(scope="module")
def resampled(wav_folder):
  """per file, what the resampler alone makes of it: (fp32 [1, n] on the device, n)"""
  _, data = wav_folder
  out = {}
  for name, sr, _ in FILES:
    y, lens = rs.resample(torch.from_numpy(data[name][None]).to(DEV), None, sr, SR, clip=True)
    out[name] = (y, lens[0])
  return out


def test_input_side_mel_front_end(wav_folder, resampled, tmp_path):
  from waveglow_amd.taco_stft import TacotronSTFT
  folder, data = wav_folder
  hp = HParams()
  assert hp.sampling_rate == SR
  taco = TacotronSTFT(hp, DEV, resample_inputs=True)
  paths = [folder / f"{name}.wav" for name, _, _ in FILES]
  mel, frames, audio, lens = taco.get_mel_and_wav_tensors_from_files(paths)
  mel2, frames2 = taco.get_mel_tensors_from_files(paths)
  assert frames2 == frames and torch.equal(mel2, mel)
  lens = lens.cpu().tolist()
  assert lens == [resampled[name][1] for name, _, _ in FILES] == [2757, 3000, 3446]
  assert audio.dtype == torch.float32 and audio.shape == (3, max(lens)) and mel.shape == (3, 80, max(lens) // 256 + 1)
  for b, (name, sr, _) in enumerate(FILES):
    y, n = resampled[name]
    assert torch.equal(audio[b, :n], y[0]) and not audio[b, n:].any()
    own, own_frames, _ = taco.mel_spectrogram_ragged_device(y, [n])
    assert frames[b] == own_frames[0] == n // 256 + 1
    assert torch.equal(mel[b, :, :frames[b]], own[0]), name
    assert not mel[b, :, frames[b]:].any()
    assert torch.equal(taco.get_wav_tensor_from_file(paths[b]), audio[b, :n].cpu()), name
  # the file at the model's rate: the bits it gives today
  today = TacotronSTFT(hp, DEV)
  mel_t, frames_t, audio_t, _ = today.get_mel_and_wav_tensors_from_files(paths[1:2])
  assert frames_t == [frames[1]] and torch.equal(mel_t[0], mel[1, :, :frames[1]]) and torch.equal(audio_t[0], audio[1, :3000])
  assert torch.equal(audio_t[0].cpu(), torch.from_numpy(convert_wav(data["b_22k"], np.float32)))
  with pytest.raises(ValueError, match="48000Hz"):
    today.get_mel_tensors_from_files(paths)
  # a resampled utterance of 512 samples or fewer is refused like a short file
  from scipy.io.wavfile import write
  short = tmp_path / "short_48k.wav"
  write(short, 48000, data["a_48k"][:1114])                                            # -> 512 samples
  with pytest.raises(_lib.WgError, match="too short"):
    taco.get_mel_tensors_from_files([paths[0], short])


def test_input_side_wav_pool(wav_folder, resampled):
  from waveglow_amd.device_data import DeviceWavPool
  from waveglow_amd.training import Entry
  folder, _ = wav_folder
  hp = HParams()
  entries = [Entry(name, f"{name}.wav", folder / f"{name}.wav") for name, _, _ in FILES]
  with pytest.raises(ValueError, match="48000Hz"):
    DeviceWavPool(entries, hp, DEV)
  pool = DeviceWavPool(entries, hp, DEV, resample_inputs=True)
  assert pool.is_int16 is False and pool.lengths == [resampled[name][1] for name, _, _ in FILES]
  seg = 2900                                                                           # longer than the first utterance
  picks = [(0, 0), (1, 100), (2, 546), (2, 0)]
  status = torch.zeros(1, dtype=torch.int32, device=DEV)
  rows = pool.gather(torch.tensor(picks, dtype=torch.int32).to(DEV), seg, status)
  assert int(status[0]) == 0
  for (u, s), row in zip(picks, rows):
    y, n = resampled[FILES[u][0]]
    want = torch.zeros(seg, device=DEV)
    want[:min(seg, n - s)] = y[0, s:s + seg]
    assert torch.equal(row, want), (u, s)


@pytest.fixture(scope="module")
def ckpt(tmp_path_factory):
  """(checkpoint path, hparams) of the 64-channel synthetic model the infer_batch_pcm tests of test_gpu_ragged_post use"""
  from waveglow_amd.checkpoint import CheckpointWaveglow
  hp = HParams(n_channels=64, n_layers=4, n_flows=4, n_early_every=2)
  m = WaveGlow(hp)
  m.load_state_dict(synthetic.to_weightnorm_form(synthetic.make_state_dict(hp, seed=8)))
  path = tmp_path_factory.mktemp("resample_ckpt") / "3.pt"
  CheckpointWaveglow.from_instances(m, None, hp, 3).save(path)
  return path, hp


def test_output_side_infer_batch_pcm(ckpt):
  from waveglow_amd.checkpoint import CheckpointWaveglow
  from waveglow_amd.synthesizer import Synthesizer
  synth = Synthesizer(CheckpointWaveglow.load(ckpt[0], torch.device(DEV)), device=torch.device(DEV))
  frames = (9, 17)
  mels = [synthetic.make_mel(1, T, seed=20 + T) for T in frames]
  kw = dict(sigma=0.9, denoiser_strength=0.01, seed=11)
  ref = synth.infer_batch(mels, **kw)
  plain = synth.infer_batch_pcm(mels, **kw)
  got = synth.infer_batch_pcm(mels, output_sampling_rate=16000, **kw)
  assert len(got) == 2
  for T, r, p, g in zip(frames, ref, plain, got):
    y, lens = rs.resample(torch.from_numpy(r.wav_denoised[None]).to(DEV), None, SR, 16000)
    y = y.cpu().numpy()[0]
    assert lens == [rs.out_len(256 * T, 320, 441)] and g.pcm.dtype == np.int16 and g.pcm.shape == (lens[0],)
    assert np.array_equal(g.pcm, convert_wav(normalize_wav(y), np.int16))
    assert g.sampling_rate == 16000 and g.peak == float(np.max(np.abs(y)))
    assert g.was_overamplified == p.was_overamplified == r.was_overamplified
    # without the argument: the bytes of infer_batch + the host functions, as before
    assert p.sampling_rate == SR and p.pcm.shape == (256 * T,)
    assert np.array_equal(p.pcm, convert_wav(normalize_wav(r.wav_denoised), np.int16))
    assert p.peak == float(np.max(np.abs(r.wav_denoised)))
  with pytest.raises(_lib.WgError):
    synth.infer_batch_pcm(mels, output_sampling_rate=192000, **kw)


def test_cli_synthesize_wav_resamples_in_and_out(ckpt, wav_folder, resampled, tmp_path):
  from scipy.io import wavfile
  from waveglow_amd import cli
  folder, _ = wav_folder
  out = tmp_path / "out"
  args = ["synthesize-wav", str(ckpt[0]), str(folder), "--custom-seed", "5", "--batch-size", "2", "-out", str(out),
          "--output-sampling-rate", "16000"]
  assert cli.main(args + ["--resample-inputs"]) == 0
  for name, _, _ in FILES:
    rate, data = wavfile.read(out / f"{name}.wav")
    n = resampled[name][1]
    assert rate == 16000 and data.dtype == np.int16
    assert data.shape == (rs.out_len(256 * (n // 256 + 1), 320, 441),), name
    assert np.abs(data.astype(np.int32)).max() == 32767                                # normalised after the resampling
  with pytest.raises(ValueError, match="48000Hz"):
    cli.main(args[:8] + [str(tmp_path / "out_refused")] + args[9:])
