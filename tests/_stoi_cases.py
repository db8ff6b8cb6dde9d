"""The shared inputs of the intelligibility tests, with the oracle's results computed once per case and shared.

The speech-like signal: harmonics 1 .. 29 of an F0 wandering around 110 Hz, times a squared, clipped 1.3 Hz envelope so that
real pauses exist, peak 0.5, plus noise of 1e-4.  It is made at 22 050 Hz and brought to 10 kHz with
``scipy.signal.resample_poly(x, 200, 441)``, rounded to fp32.  The processed side is the clean side itself, or the clean
side plus white noise at 20 dB or at -5 dB."""
import functools

import numpy as np

import _stoi_oracle as oracle

SR = 22050
LENGTHS = (44100, 66927, 22050)                  # at 22 050 Hz
LENGTHS_10K = (20000, 30353, 10000)              # ceil(n 200 / 441)
SNRS = (None, 20.0, -5.0)                        # None: y is x
CASES = [(n, snr) for n in LENGTHS for snr in SNRS]

# the columns validate's table gains with intelligibility_metrics, before "Wav path"
STOI_COLUMNS = ["STOI", "ESTOI", "# STOI frames", "# STOI frames kept"]


@functools.lru_cache(maxsize=None)
def speech_22k(n=max(LENGTHS), seed=11):
  """fp32 [n] at 22 050 Hz."""
  rng = np.random.default_rng(seed)
  t = np.arange(n) / SR
  f0 = 110.0 + 12.0 * np.sin(2 * np.pi * 0.37 * t) + 5.0 * np.sin(2 * np.pi * 2.3 * t)
  phi = np.cumsum(2 * np.pi * f0 / SR)
  tone = sum(np.sin(k * phi) / k for k in range(1, 30))
  env = np.clip(np.sin(2 * np.pi * 1.3 * t), 0.0, 1.0) ** 2
  x = tone * env
  x = 0.5 * x / np.max(np.abs(x)) + 1e-4 * rng.standard_normal(n)
  return x.astype(np.float32)


@functools.lru_cache(maxsize=None)
def clean(n):
  """The first n samples of the speech-like signal at 22 050 Hz as fp32 at 10 kHz."""
  from scipy.signal import resample_poly
  return resample_poly(speech_22k()[:n].astype(np.float64), 200, 441).astype(np.float32)


def add_noise(x, snr_db, seed=5):
  """x plus white noise at snr_db, fp32."""
  rng = np.random.default_rng(seed)
  noise = rng.standard_normal(len(x))
  x64 = x.astype(np.float64)
  gain = np.sqrt(np.mean(x64 ** 2) / (np.mean(noise ** 2) * 10.0 ** (snr_db / 10.0)))
  return (x64 + gain * noise).astype(np.float32)


@functools.lru_cache(maxsize=None)
def pair(n, snr):
  """(x, y) fp32 at 10 kHz of a case."""
  x = clean(n)
  return x, (x if snr is None else add_noise(x, snr))


@functools.lru_cache(maxsize=None)
def reference(n, snr):
  """The oracle's result of a case."""
  return oracle.stoi(*pair(n, snr))


@functools.lru_cache(maxsize=None)
def stationary(frames, seed=2):
  """fp32 white noise of 256 + 128 frames samples: F0 = frames and every frame is kept."""
  return (0.1 * np.random.default_rng(seed).standard_normal(oracle.W + oracle.H * frames)).astype(np.float32)


@functools.lru_cache(maxsize=None)
def click(kept):
  """fp32 [20000]: silence with one click that `kept` (1 or 2) frames hold.  Sample 5 lies in frame 0 alone; sample 192 is
  sample 192 of frame 0 and sample 64 of frame 1, where the symmetric window has the same value but for rounding."""
  x = np.zeros(20000, np.float32)
  x[5 if kept == 1 else 192] = 0.5
  return x
