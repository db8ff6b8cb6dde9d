"""What follows the flow in a batched synthesis, and what precedes it in ``synthesize-wav``, on ragged batches: the
denoiser (``wg_stft_denoise`` with ``lens``), the mel front-end (``wg_stft_mel`` with ``lens``) and the int16 finishing
(``wg_wav_finish``).  Every utterance of a batch must come out BIT FOR BIT as its single call / the host functions give
it: no tolerance anywhere in this file."""
import numpy as np
import pytest
import torch

from waveglow_amd import _lib, pcm, synthetic
from waveglow_amd.audio import convert_wav, float_to_wav, is_overamp, normalize_wav
from waveglow_amd.hparams import HParams
from waveglow_amd.model import WaveGlow

pytestmark = pytest.mark.gpu

DEV = "cuda:0"


@pytest.fixture(scope="module")
def ckpt(tmp_path_factory):
  """(checkpoint path, hparams) of the 64-channel synthetic model of test_synthesizer_batch_equals_one_by_one."""
  from waveglow_amd.checkpoint import CheckpointWaveglow
  hp = HParams(n_channels=64, n_layers=4, n_flows=4, n_early_every=2)
  m = WaveGlow(hp)
  m.load_state_dict(synthetic.to_weightnorm_form(synthetic.make_state_dict(hp, seed=8)))
  path = tmp_path_factory.mktemp("ragged_post") / "3.pt"
  CheckpointWaveglow.from_instances(m, None, hp, 3).save(path)
  return path, hp


@pytest.fixture(scope="module")
def synth(ckpt):
  from waveglow_amd.checkpoint import CheckpointWaveglow
  from waveglow_amd.synthesizer import Synthesizer
  return Synthesizer(CheckpointWaveglow.load(ckpt[0], torch.device(DEV)), device=torch.device(DEV))


DENOISE_FRAMES = (9, 40, 4, 31, 32)   # x 256 samples: 4 = the minimum (reflected ends meet), 31 -> F = 32 = one tile,
                                      # 32 -> F = 33 starts a second tile, the longest is not the first


@pytest.mark.parametrize("strength", [0.01, 0.5])
def test_denoiser_ragged_equals_single(synth, strength):
  den = synth.denoiser
  lens = [256 * t for t in DENOISE_FRAMES]
  N = max(lens)
  audio = (torch.rand((len(lens), N), generator=torch.Generator().manual_seed(3)) * 1.6 - 0.8).to(DEV)
  lens_dev = torch.tensor(lens, dtype=torch.int32).to(DEV)
  outs = []
  for _ in range(2):
    out = torch.full_like(audio, float("nan"))
    den.run_ragged(audio, lens, lens_dev, strength, out)
    outs.append(out)
  torch.cuda.synchronize()
  assert torch.equal(outs[0], outs[1])                                   # no NaN left, and the same bits twice
  for b, n in enumerate(lens):
    single = den(audio[b:b + 1, :n].contiguous(), strength)
    assert single.shape == (1, 1, n)
    assert torch.equal(outs[0][b, :n], single[0, 0]), f"utterance {b} ({n} samples)"
    assert not outs[0][b, n:].any(), f"utterance {b}: not zero behind its end"
    assert float(single.abs().max()) > 0
  via_forward = den(audio, strength, lengths=torch.tensor(lens))
  assert via_forward.shape == (len(lens), 1, N) and torch.equal(via_forward[:, 0], outs[0])
  assert torch.equal(den(audio, strength, lengths=lens)[:, 0], outs[0])


def test_denoiser_refusals_leave_the_device_usable(synth):
  den = synth.denoiser
  N = 256 * 12
  audio = (torch.rand((2, N), generator=torch.Generator().manual_seed(4)) - 0.5).to(DEV)
  for bad in ([768, N], [1024 + 100, N], [N, N + 256], [N], [N, N, N]):
    with pytest.raises(_lib.WgError):
      den(audio, 0.01, lengths=bad)
  good = den(audio, 0.01, lengths=[1024, N])
  assert torch.equal(good[1, 0], den(audio[1:2], 0.01)[0, 0])
  assert torch.equal(good[0, 0, :1024], den(audio[0:1, :1024].contiguous(), 0.01)[0, 0]) and not good[0, 0, 1024:].any()


def test_mel_ragged_equals_single(ckpt):
  from waveglow_amd.taco_stft import TacotronSTFT
  taco = TacotronSTFT(ckpt[1], torch.device(DEV))
  lens = [513, 8191, 8192, 8193, 10000]
  g = torch.Generator().manual_seed(5)
  wavs = [torch.rand(n, generator=g) * 2 - 1 for n in lens]
  mel, frames = taco.mel_spectrogram_ragged(wavs)
  assert frames == [n // 256 + 1 for n in lens]
  assert mel.shape == (len(lens), taco.n_mel_channels, max(frames))
  for b, w in enumerate(wavs):
    single = taco.mel_spectrogram(w[None])[0]
    assert single.shape[1] == frames[b]
    assert torch.equal(mel[b, :, :frames[b]], single), f"utterance {b} ({lens[b]} samples)"
    assert not mel[b, :, frames[b]:].any()
  # more than one 64-frame block and more than one 32-frame tile behind a short utterance
  long = torch.rand(20000, generator=g) * 2 - 1
  mel2, frames2 = taco.mel_spectrogram_ragged([wavs[0], long])
  assert frames2 == [3, 79] and not mel2[0, :, 3:].any()
  assert torch.equal(mel2[0, :, :3], mel[0, :, :3]) and torch.equal(mel2[1], taco.mel_spectrogram(long[None])[0])
  with pytest.raises(_lib.WgError):
    taco.mel_spectrogram_ragged([wavs[1], wavs[0][:512]])
  with pytest.raises(AssertionError):
    taco.mel_spectrogram_ragged([wavs[1], wavs[2] * 1.5])


def _finish_rows():
  k = np.arange(-32767, 32767, dtype=np.float32)
  tie = np.concatenate([(k + np.float32(0.5)) / np.float32(32767), np.ones(1, np.float32)]).astype(np.float32)
  rng = np.random.default_rng(6)
  loud = rng.uniform(-1, 1, 5000).astype(np.float32)
  loud[1234] = np.float32(-3.7)
  faint = (rng.uniform(-1, 1, 3001) * 1e-30).astype(np.float32)
  faint[7] = np.float32(1e-30)
  return [tie, np.zeros(2048, np.float32), loud, faint, rng.uniform(-0.9, 0.9, 4097).astype(np.float32)]


def _finish_prefilled(raw, den, lens):
  """wg_wav_finish through the C ABI into an int16 buffer that starts as 0x7fff: (pcm, stats) as numpy arrays."""
  import ctypes as C
  lib = _lib.load()
  B, N = den.shape
  r, d = torch.from_numpy(raw).to(DEV), torch.from_numpy(den).to(DEV)
  out = torch.full((B, N), 0x7fff, dtype=torch.int16, device=DEV)
  stats = torch.full((B, 8), float("nan"), dtype=torch.float32, device=DEV)
  ws = torch.empty(lib.wg_wav_finish_workspace_bytes(B), dtype=torch.uint8, device=DEV)
  ld = torch.tensor(lens, dtype=torch.int32).to(DEV)
  _lib.check(lib.wg_wav_finish(r.data_ptr(), d.data_ptr(), ld.data_ptr(), out.data_ptr(), stats.data_ptr(), B, N,
                               ws.data_ptr(), ws.numel(), C.c_void_p(torch.cuda.current_stream().cuda_stream)))
  return out.cpu().numpy(), stats.cpu().numpy()


def test_finish_equals_numpy():
  rows = _finish_rows()
  # on the host, before any device call: the first row really exercises the rounding mode
  t = rows[0] * np.float32(32767)
  assert t.dtype == np.float32 and np.max(np.abs(rows[0])) == 1.0
  assert int(np.sum(t - np.floor(t) == 0.5)) >= 60000
  expect = [convert_wav(normalize_wav(x), np.int16) for x in rows]
  assert np.any(expect[0] != np.floor(t + np.float32(0.5)).astype(np.int16))   # rounding half up would differ
  lens = [len(x) for x in rows]
  N = (max(lens) + 7) // 8 * 8
  den = np.zeros((len(rows), N), np.float32)
  for b, x in enumerate(rows):
    den[b, :lens[b]] = x
    den[b, lens[b]:] = 9.0                                 # behind an utterance: must not reach the statistics
  raw = (den * np.float32(0.5)).astype(np.float32)         # another signal, so that raw and denoised cannot be confused
  samples, stats = _finish_prefilled(raw, den, lens)
  for b, x in enumerate(rows):
    assert np.array_equal(samples[b, :lens[b]], expect[b]), f"row {b}"
    assert not samples[b, lens[b]:].any()
    r = raw[b, :lens[b]]
    assert stats[b, pcm.DEN_PEAK] == np.max(np.abs(x)) and stats[b, pcm.RAW_PEAK] == np.max(np.abs(r))
    assert stats[b, pcm.DEN_MIN] == x.min() and stats[b, pcm.DEN_MAX] == x.max()
    assert stats[b, pcm.RAW_MIN] == r.min() and stats[b, pcm.RAW_MAX] == r.max()
    assert bool(stats[b, pcm.RAW_MIN] < -1 or stats[b, pcm.RAW_MAX] > 1) == is_overamp(r)
    assert stats[b, pcm.NON_FINITE] == 0
  assert is_overamp(raw[2, :lens[2]]) and not is_overamp(raw[0, :lens[0]])
  # the Python layer returns the same arrays
  again, stats2 = pcm.finish(torch.from_numpy(raw).to(DEV), torch.from_numpy(den).to(DEV), lens)
  assert again.dtype == np.int16 and np.array_equal(again, samples) and np.array_equal(stats2, stats)


def test_finish_reports_non_finite_samples():
  rows = _finish_rows()[3:]
  lens = [len(x) for x in rows]
  N = (max(lens) + 7) // 8 * 8
  den = np.zeros((len(rows), N), np.float32)
  for b, x in enumerate(rows):
    den[b, :lens[b]] = x
  for bad in (np.nan, np.inf):
    den[1, 100] = bad
    d = torch.from_numpy(den).to(DEV)
    with pytest.raises(_lib.WgError, match="utterance 1"):
      pcm.finish(d, d, lens)
  den[1, 100] = 0.25
  den[0, lens[0] + 1] = np.nan                             # behind the utterance's end: not its sample
  d = torch.from_numpy(den).to(DEV)
  samples, _ = pcm.finish(d, d, lens)
  assert np.array_equal(samples[1, :lens[1]], convert_wav(normalize_wav(den[1, :lens[1]]), np.int16))


@pytest.mark.parametrize("strength", [0.01, 0.0])
def test_infer_batch_pcm_equals_infer_batch_plus_host_finishing(synth, strength):
  mels = [synthetic.make_mel(1, T, seed=20 + T) for T in (9, 30, 17)]
  ref = synth.infer_batch(mels, sigma=0.9, denoiser_strength=strength, seed=11)
  got = synth.infer_batch_pcm(mels, sigma=0.9, denoiser_strength=strength, seed=11)
  assert len(got) == 3
  for T, r, p in zip((9, 30, 17), ref, got):
    assert p.pcm.dtype == np.int16 and p.pcm.shape == (256 * T,)
    assert np.array_equal(p.pcm, convert_wav(normalize_wav(r.wav_denoised), np.int16))
    assert p.was_overamplified == r.was_overamplified and p.sampling_rate == r.sampling_rate
    assert p.peak == float(np.max(np.abs(r.wav_denoised)))
    if strength == 0:
      assert np.array_equal(r.wav, r.wav_denoised)


def test_cli_synthesize_wav_batch_equals_one_by_one(ckpt, tmp_path):
  from waveglow_amd import cli
  path, hp = ckpt
  src = tmp_path / "wavs"
  src.mkdir()
  rng = np.random.default_rng(7)
  for i, n in enumerate((3000, 5121, 4096)):
    float_to_wav(rng.uniform(-0.5, 0.5, n).astype(np.float32), src / f"u{i}.wav", sample_rate=hp.sampling_rate)
  outs = []
  for bs in ("1", "2"):
    out = tmp_path / f"out{bs}"
    assert cli.main(["synthesize-wav", str(path), str(src), "--custom-seed", "5", "--batch-size", bs, "-out", str(out)]) == 0
    outs.append([(out / f"u{i}.wav").read_bytes() for i in range(3)])
  from scipy.io import wavfile
  for i, (x, y) in enumerate(zip(*outs)):
    rate, data = wavfile.read(tmp_path / "out2" / f"u{i}.wav")
    assert rate == hp.sampling_rate and data.dtype == np.int16 and data.shape == (256 * ((3000, 5121, 4096)[i] // 256 + 1),)
    assert x == y, f"u{i}.wav differs between --batch-size 1 and 2"
