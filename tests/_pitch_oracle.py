"""numpy fp64 restatement of the pitch metrics (include/waveglow_amd.h: wg_pitch_*): the YIN tracker,
steps 1-5 of de Cheveigne & Kawahara (2002), and the pair row.  It is the yardstick of tests/test_gpu_pitch.py; besides the
values it reports how stable its own decisions are, so that a test can refuse to pin a decision that hangs on a rounding:

  margin   the smallest |d'(tau) - threshold| over the lags the threshold search visited and the smallest
           |d'(tau+1) - d'(tau)| over the comparisons of the walk (inf where there was none)
  den      the smallest denominator a - 2b + c over the interpolated frames (inf where there was none)
"""
import math

import numpy as np

DEFAULTS = dict(sampling_rate=22050, frame_length=1024, hop_length=256, fmin=60.0, fmax=600.0, threshold=0.1)
ROW = ("f0_rmse_cents", "f0_rmse_hz", "gpe", "vuv_error", "frames", "voiced_a", "voiced_b", "voiced_both")


def lags(sampling_rate=22050, fmin=60.0, fmax=600.0):
  """(tau_min, tau_max)"""
  return max(2, math.floor(sampling_rate / fmax)), math.ceil(sampling_rate / fmin)


def frame_count(n, W, H, tau_max):
  return (n - W - tau_max) // H + 1 if n >= W + tau_max else 0


def difference(frame, W, tau_max):
  """d(tau), tau = 0 .. tau_max, of the W + tau_max samples of a frame; j ascending, as written."""
  x = np.asarray(frame, np.float64)
  d = np.zeros(tau_max + 1)
  for tau in range(1, tau_max + 1):
    e = x[:W] - x[tau:tau + W]
    acc = 0.0
    for v in e * e:                       # ascending, one rounding per product and per sum
      acc += v
    d[tau] = acc
  return d


def _difference_fast(frame, W, tau_max):
  """The same sums by np.cumsum (sequential in numpy: the ascending order of ``difference``)."""
  x = np.asarray(frame, np.float64)
  idx = np.arange(W)[None, :] + np.arange(tau_max + 1)[:, None]
  e = x[None, :W] - x[idx]
  return np.cumsum(e * e, axis=1)[:, -1]


def cmnd(d):
  """d'(tau): 1 at lag 0 and where the running sum of d is 0."""
  tau_max = len(d) - 1
  out = np.ones(tau_max + 1)
  run = 0.0
  for tau in range(1, tau_max + 1):
    run += d[tau]
    out[tau] = d[tau] * tau / run if run != 0.0 else 1.0
  return out


def pick(dp, sr, tau_min, tau_max, threshold):
  """(f0, aperiodicity, tau or 0, margin, den) of one frame's d'."""
  margin, den_out = np.inf, np.inf
  tau = 0
  for k in range(tau_min, tau_max + 1):
    margin = min(margin, abs(dp[k] - threshold))
    if dp[k] < threshold:
      tau = k
      break
  if tau == 0:
    return 0.0, float(np.min(dp[tau_min:tau_max + 1])), 0, margin, den_out
  while tau + 1 <= tau_max:
    margin = min(margin, abs(dp[tau + 1] - dp[tau]))
    if not dp[tau + 1] < dp[tau]:
      break
    tau += 1
  shift = 0.0
  if tau - 1 >= 1 and tau + 1 <= tau_max:
    a, b, c = dp[tau - 1], dp[tau], dp[tau + 1]
    den = a - 2.0 * b + c
    den_out = den
    if den > 0:
      sh = (a - c) / (2.0 * den)
      if abs(sh) <= 1:
        shift = sh
  return sr / (tau + shift), float(dp[tau]), tau, margin, den_out


def yin(x, sampling_rate=22050, frame_length=1024, hop_length=256, fmin=60.0, fmax=600.0, threshold=0.1, slow=False):
  """Tracks of one utterance (1-D fp32 / fp64 samples): dict f0, aperiodicity (fp64 [F]), tau (int [F], 0 = unvoiced),
  frames, margin, den."""
  x = np.asarray(x)
  tau_min, tau_max = lags(sampling_rate, fmin, fmax)
  W, H = frame_length, hop_length
  F = frame_count(len(x), W, H, tau_max)
  f0, ap, taus = np.zeros(F), np.zeros(F), np.zeros(F, np.int64)
  margin, den = np.inf, np.inf
  for t in range(F):
    frame = x[t * H:t * H + W + tau_max]
    assert len(frame) == W + tau_max
    d = difference(frame, W, tau_max) if slow else _difference_fast(frame, W, tau_max)
    f0[t], ap[t], taus[t], m, dn = pick(cmnd(d), float(sampling_rate), tau_min, tau_max, threshold)
    margin, den = min(margin, m), min(den, dn)
  return dict(f0=f0, aperiodicity=ap, tau=taus, frames=F, margin=margin, den=den)


def compare(f0_a, f0_b):
  """The pair row as a dict (keys ROW) plus gpe_margin, the smallest ||f0_b / f0_a - 1| - 0.2| (inf without a both-voiced
  frame).  a is the original, b the synthesis; the first min(Fa, Fb) frames count."""
  F = min(len(f0_a), len(f0_b))
  a, b = np.asarray(f0_a, np.float64)[:F], np.asarray(f0_b, np.float64)[:F]
  va, vb = a > 0, b > 0
  both = va & vb
  n = int(both.sum())
  nan = float("nan")
  row = dict(frames=F, voiced_a=int(va.sum()), voiced_b=int(vb.sum()), voiced_both=n,
             vuv_error=float((va != vb).sum()) / F if F else nan, f0_rmse_cents=nan, f0_rmse_hz=nan, gpe=nan,
             gpe_margin=np.inf)
  if n:
    ratio = b[both] / a[both]
    cents = 1200.0 * np.log2(ratio)
    row["f0_rmse_cents"] = math.sqrt(float(np.sum(cents * cents)) / n)
    row["f0_rmse_hz"] = math.sqrt(float(np.sum((b[both] - a[both]) ** 2)) / n)
    dev = np.abs(ratio - 1.0)
    row["gpe"] = float((dev > 0.2).sum()) / n
    row["gpe_margin"] = float(np.min(np.abs(dev - 0.2)))
  return row


def pitch_metrics(x_a, x_b, **params):
  """(row, tracks_a, tracks_b) of one pair of utterances."""
  ta, tb = yin(x_a, **params), yin(x_b, **params)
  return compare(ta["f0"], tb["f0"]), ta, tb
