"""The signal pair and the parameter sets of the pitch tests, with the oracle's tracks computed once per set and shared."""
import functools

import numpy as np

import _pitch_oracle as oracle

SR = 22050
N = 6000
# name -> (parameters, sample count used)
CASES = {
  "defaults": (dict(), N),
  "tau255": (dict(frame_length=64, fmax=2000.0, fmin=86.5), N),          # tau_max = 255
  "tau256": (dict(frame_length=64, fmax=2000.0, fmin=86.2), N),          # tau_max = 256: a second pass of 256 lags
  "limits": (dict(frame_length=2048, fmin=21.54), N),                    # tau_max = 1024, W = 2048: both upper limits
  "hop1": (dict(hop_length=1), 1500),
}
RAGGED = (1391, 1392, 1648, 6000)                                        # 0, 1, 2 and 19 frames with the defaults

# the columns of validate's table as they are without the flag, and the seven the flag adds before "Wav path"
TODAY = ["Name", "Subpath", "Timepoint", "Iteration", "Seed", "Sigma", "Denoiser strength", "Inference duration (s)",
         "Denoising duration (s)", "Overamplified?", "Inferred wav duration (s)", "# Difference frames", "Sampling rate (Hz)",
         "# MFCC Coefficients", "MFCC DTW MCD", "MFCC DTW PEN", "# MFCC DTW frames", "MCD", "PEN", "# Frames",
         "Cosine Similarity (Padded)", "Wav path"]
PITCH = ["F0 RMSE (cents)", "F0 RMSE (Hz)", "Gross pitch error", "V/UV error", "# Pitch frames", "# Voiced frames original",
         "# Voiced frames inferred"]


def _harmonics(f):
  phi = np.cumsum(2 * np.pi * f / SR)
  return 0.2 * sum(np.sin(k * phi) / k for k in range(1, 6))


@functools.lru_cache(maxsize=None)
def signals():
  """(a, b) fp32 [6000]: five harmonics of a slowly modulated 150 Hz on side a; on side b a jump to 190 Hz at sample
  1500 and a noise floor; on both a stretch of noise (3000-4199) and silence from 5400 on."""
  n = np.arange(N)
  wobble = 10 * np.sin(2 * np.pi * n / SR)
  rng = np.random.default_rng(3)
  a = _harmonics(150 + wobble)
  a[3000:4200] = 0.05 * rng.standard_normal(1200)
  b = _harmonics(np.where(n < 1500, 150.0, 190.0) + wobble)
  b[3000:4200] = 0.05 * rng.standard_normal(1200)
  b += 0.003 * rng.standard_normal(N)                                   # the floor lies on the noise stretch too
  a[5400:] = 0
  b[5400:] = 0
  return a.astype(np.float32), b.astype(np.float32)


@functools.lru_cache(maxsize=None)
def tracks(case, side, n=None):
  """The oracle's tracks of side 0 / 1 cropped to n samples (default: the case's own count) under a case's parameters."""
  params, count = CASES[case]
  return oracle.yin(signals()[side][:count if n is None else n], **params)


@functools.lru_cache(maxsize=None)
def row(case, n=None):
  return oracle.compare(tracks(case, 0, n)["f0"], tracks(case, 1, n)["f0"])
