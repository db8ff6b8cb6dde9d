"""GPU: every public entry point that takes per-utterance counts takes the same forms of them (``waveglow_amd._args``).

For each entry point, at the smallest shape at which its ragged kernel can still go wrong (B = 2, one utterance shorter
than the row and crossing a frame or tile edge): a list, a tuple and an int64 CPU tensor -- and, where the entry point
takes device counts, an int32 tensor on the device -- give ``torch.equal`` results and input gradients; a bool entry, a
float entry, a count past either end of the range and a list of the wrong length raise WgError."""
import pytest
import torch

from _cases import Case
from waveglow_amd import (HParams, MultiResolutionSTFTLoss, MultiScaleMelLoss, SoftDTWLoss, STOILoss, WaveGlow, metrics,
                          resample, softdtw)
from waveglow_amd._lib import WgError
from waveglow_amd.denoiser import Denoiser
from waveglow_amd.taco_stft import TacotronSTFT, TSTFTHParams

pytestmark = pytest.mark.gpu

DEV = "cuda:0"


def _rand(*shape, seed=0, scale=0.3):
  g = torch.Generator().manual_seed(seed)
  return ((torch.rand(*shape, generator=g) * 2 - 1) * scale).to(DEV)


def _with_grad(x0, fn):
  """[result, d sum(result) / d x] of ``fn(x)`` on a fresh leaf; NaN results (an utterance without a score) add nothing."""
  x = x0.clone().requires_grad_(True)
  out = fn(x)
  torch.nan_to_num(out.double(), nan=0.0).sum().backward()
  return [out.detach(), x.grad]


def _vocoder(**over):
  c = Case("tiny")
  hp = HParams(**{**{k: getattr(c.hp, k) for k in ("n_mel_channels", "n_flows", "n_group", "n_early_every", "n_early_size",
                                                  "n_layers", "n_channels", "kernel_size")}, **over})
  from waveglow_amd import synthetic
  m = WaveGlow.remove_weightnorm(WaveGlow(hp))
  m.load_state_dict(synthetic.make_state_dict(hp, seed=7))
  return m.to(DEV).eval().requires_grad_(False)


@pytest.fixture(scope="module")
def entries():
  """name -> (run(counts) -> list of tensors, good counts, lo, hi, takes device counts)."""
  out = {}
  x256, y256 = _rand(2, 256, seed=1), _rand(2, 256, seed=2)
  stft = MultiResolutionSTFTLoss(fft_sizes=(64,), hop_sizes=(16,), win_lengths=(64,), device=DEV)
  out["stft_loss"] = (lambda l: _with_grad(x256, lambda x: stft(x, y256, l)), [200, 256], 33, 256, False)
  mel = MultiScaleMelLoss(n_ffts=(64,), hop_sizes=(16,), win_lengths=(64,), n_mels=(5,), device=DEV)
  out["mel_loss"] = (lambda l: _with_grad(x256, lambda x: mel(x, y256, l)), [200, 256], 33, 256, False)

  # 4 224 samples at 10 kHz are the fewest with a segment (tests/_stoi_loss_cases.py: j1); the shorter row has none: NaN
  N = 4224
  xs, ys = _rand(2, N, seed=3), _rand(2, N, seed=4)
  stoi = STOILoss(sampling_rate=10000, device=DEV)
  out["stoi_scores"] = (lambda l: _with_grad(xs, lambda x: stoi.scores(x, ys, l)), [4000, N], 0, N, False)

  x960 = _rand(2, 960, seed=5)
  out["resample"] = (lambda l: [resample.resample(x960, l, 48000, 22050)[0]], [500, 960], 0, 960, False)
  out["resample_differentiable"] = (
    lambda l: _with_grad(x960, lambda x: resample.resample_differentiable(x, l, 48000, 22050)[0]), [500, 960], 0, 960, False)

  tiny = _vocoder()
  den = Denoiser(tiny, TSTFTHParams(), "zeros", DEV)
  x2048 = _rand(2, 2048, seed=6)
  out["denoiser_forward"] = (lambda l: [den(x2048, 0.1, l)], [1024, 2048], 1024, 2048, True)
  out["denoiser_forward_differentiable"] = (
    lambda l: _with_grad(x2048, lambda x: den.forward_differentiable(x, 0.1, l)), [1024, 2048], 1024, 2048, True)

  taco = TacotronSTFT(TSTFTHParams(), DEV)
  x1536 = _rand(2, 1536, seed=7)
  out["mel_spectrogram_differentiable"] = (
    lambda l: _with_grad(x1536, lambda x: taco.mel_spectrogram_differentiable(x, l)), [1000, 1536], 513, 1536, False)

  def ragged_device(l):
    m, frames, frames_dev = taco.mel_spectrogram_ragged_device(x1536, l)
    assert frames == frames_dev.tolist()
    return [m, frames_dev]
  out["mel_spectrogram_ragged_device"] = (ragged_device, [1000, 1536], 513, 1536, False)

  fa, fb = _rand(2, 20, 12, seed=8, scale=2.0), _rand(2, 20, 12, seed=9, scale=2.0)
  out["mfcc"] = (lambda f: [metrics.mfcc(fa, f, 8)], [7, 12], 1, 12, True)
  out["dtw_distance"] = (lambda f: list(metrics.dtw_distance(fa, f, fb, [12, 7])), [7, 12], 1, 12, True)
  out["mel_metrics_enqueue"] = (lambda f: [metrics.mel_metrics_enqueue(fa, f, fb, [12, 7], 8)], [7, 12], 1, 12, True)
  out["soft_dtw"] = (lambda f: _with_grad(fa, lambda a: softdtw.soft_dtw(a, f, fb, [12, 7])), [7, 12], 1, 12, True)
  crit = SoftDTWLoss(features="mel", device=DEV)
  out["SoftDTWLoss"] = (lambda f: _with_grad(fa, lambda a: crit(a, f, fb, [12, 7])), [7, 12], 1, 12, True)

  # 1 648 samples are the fewest with two frames at the default parameters (1024 + 368 + 256)
  x1648 = _rand(2, 1648, seed=10)
  out["yin_f0"] = (lambda l: list(metrics.yin_f0(x1648, l)), [1392, 1648], 0, 1648, True)

  mel4, wav4 = _rand(2, 80, 4, seed=11, scale=1.0), _rand(2, 1024, seed=12)
  out["log_likelihood_enqueue"] = (lambda f: [tiny.log_likelihood_enqueue(mel4, wav4, frames=f)], [3, 4], 1, 4, True)

  wide = _vocoder(n_channels=64)                         # the gradient path takes the instantiated widths only
  zi = _rand(2, wide.n_remaining_channels, 128, seed=13, scale=1.0)
  ze = [_rand(2, wide.n_early_size, 128, seed=14 + i, scale=1.0) for i in range(wide.n_early_flows())]

  def infer(f):
    audio, g = _with_grad(mel4, lambda m: wide.infer_differentiable(m, 0.8, z_init=zi, z_early=ze, frames=f))
    return [audio[0, :256 * 3], audio[1], g]               # frames [3, 4]: nothing is promised of the audio behind row 0
  out["infer_differentiable"] = (infer, [3, 4], 1, 4, True)
  return out


NAMES = ["stft_loss", "mel_loss", "stoi_scores", "resample", "resample_differentiable", "denoiser_forward",
         "denoiser_forward_differentiable", "mel_spectrogram_differentiable", "mel_spectrogram_ragged_device", "mfcc",
         "dtw_distance", "mel_metrics_enqueue", "yin_f0", "soft_dtw", "SoftDTWLoss", "log_likelihood_enqueue",
         "infer_differentiable"]


def _same(a, b):
  return a.dtype == b.dtype and a.shape == b.shape and torch.equal(torch.nan_to_num(a, nan=-12345.0),
                                                                 torch.nan_to_num(b, nan=-12345.0))


@pytest.mark.parametrize("name", NAMES)
def test_every_accepted_form_gives_the_same_bits(entries, name):
  run, good, lo, hi, device_ok = entries[name]
  want = run(list(good))
  forms = {"tuple": tuple(good), "int64 CPU tensor": torch.tensor(good, dtype=torch.int64)}
  if device_ok:
    forms["int32 device tensor"] = torch.tensor(good, dtype=torch.int32).to(DEV)
  for form, counts in forms.items():
    got = run(counts)
    assert len(got) == len(want)
    for i, (g, w) in enumerate(zip(got, want)):
      assert _same(g, w), f"{name}: {form}: result {i} differs from the list form"
  if not device_ok:
    with pytest.raises(WgError):
      run(torch.tensor(good, dtype=torch.int32).to(DEV))


@pytest.mark.parametrize("bad", ["bool", "float", "hi + 1", "lo - 1", "one count"])
@pytest.mark.parametrize("name", NAMES)
def test_every_entry_point_refuses_the_same_counts(entries, name, bad):
  run, good, lo, hi, _ = entries[name]
  n = good[1]
  counts = {"bool": [True, n], "float": [float(n), n], "hi + 1": [n, hi + 1], "lo - 1": [lo - 1, n], "one count": [n]}[bad]
  with pytest.raises(WgError):
    run(counts)
