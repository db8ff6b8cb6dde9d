"""numpy fp64 restatement of the per-utterance likelihood (include/waveglow_amd.h: wg_nll): the
yardstick of tests/test_likelihood_cpu.py and tests/test_gpu_likelihood.py.  WaveGlowLoss (src/waveglow/train.py:31-45) of
every utterance alone, from z, the log_s of every flow, the per-column log|det W_k| and the frame counts."""
import math

import numpy as np

FRAME_COLS = 32          # columns (group-timesteps of 8 samples) per mel frame
ROW = ("nll", "bits_per_sample", "sum_z2", "sum_log_s", "log_det", "samples", "z_mean", "z_var")


def columns(frames, B, L):
  """Columns scored per utterance: 32 * frames[b], L without counts."""
  if frames is None:
    return [L] * B
  return [FRAME_COLS * int(f) if 1 <= int(f) <= L // FRAME_COLS else 0 for f in frames]


def likelihood_rows(z, log_s, logdets, frames=None, sigma=1.0):
  """z [B, 8, L], log_s: list of [B, h_k, L], logdets: log|det W_k| per column and flow.  Returns
  (rows fp64 [B, 8] in the order of ROW, track fp64 [B, ceil(L / 32)], yard fp64 [B]): ``yard`` is the magnitude
  (sum z^2 / (2 sigma^2) + sum |log_s| + |log_det|) / n_b that a summation-order bound scales with."""
  z = np.asarray(z, dtype=np.float64)
  log_s = [np.asarray(t, dtype=np.float64) for t in log_s]
  B, G, L = z.shape
  sigma = float(sigma)
  ld = float(np.sum(np.asarray(logdets, dtype=np.float64)))
  NF = (L + FRAME_COLS - 1) // FRAME_COLS
  rows = np.full((B, 8), np.nan)
  track = np.full((B, NF), np.nan)
  yard = np.zeros(B)
  for b, Lb in enumerate(columns(frames, B, L)):
    n = float(G * Lb)
    zb = z[b, :, :Lb]
    z2 = float(np.sum(zb * zb))
    ls = float(sum(np.sum(t[b, :, :Lb]) for t in log_s))
    log_det = Lb * ld
    rows[b, 2:6] = (z2, ls, log_det, n)
    if Lb == 0:
      continue
    nll = (z2 / (2 * sigma * sigma) - ls - log_det) / n
    mean = float(np.sum(zb)) / n
    rows[b, 0] = nll
    rows[b, 1] = (nll + 0.5 * math.log(2 * math.pi * sigma * sigma)) / math.log(2.0)
    rows[b, 6] = mean
    rows[b, 7] = z2 / n - mean * mean
    yard[b] = (z2 / (2 * sigma * sigma) + float(sum(np.sum(np.abs(t[b, :, :Lb])) for t in log_s)) + abs(log_det)) / n
    for q in range((Lb + FRAME_COLS - 1) // FRAME_COLS):
      c0, c1 = FRAME_COLS * q, min(FRAME_COLS * (q + 1), Lb)
      fz2 = float(np.sum(z[b, :, c0:c1] ** 2))
      fls = float(sum(np.sum(t[b, :, c0:c1]) for t in log_s))
      track[b, q] = (fz2 / (2 * sigma * sigma) - fls - (c1 - c0) * ld) / 256.0
  return rows, track, yard


def batch_mean(rows):
  """sum n_b nll_b / sum n_b: the batch loss of a dense batch."""
  rows = np.asarray(rows, dtype=np.float64)
  return float(np.sum(rows[:, 5] * rows[:, 0]) / np.sum(rows[:, 5]))
