"""The numpy restatement of the intelligibility metrics (include/waveglow_amd.h: wg_stoi): STOI and
ESTOI of a clean signal ``x`` and a processed signal ``y`` at 10 kHz, as ``pystoi.stoi(x, y, 10000, extended)`` computes
them, without the noise that package adds before its normalisations and with NaN where it has no segment.  fp64 on the
samples as given.  ``stoi_longdouble`` restates the same definition in ``np.longdouble`` with a direct DFT over bins 7 .. 218
and serves as a rounding yardstick only."""
import numpy as np

FS = 10000
W, H, NFFT = 256, 128, 512
BANDS, MIN_FREQ = 15, 150
N = 30
BETA, DYN_RANGE = -15.0, 40.0
EPS = 2.0 ** -52
BIN_LO, BIN_HI = 7, 219                          # the bins the bands reach at 10 kHz


def window():
  """fp64 w[i] = 0.5 - 0.5 cos(2 pi (i + 1) / 257), i = 0 .. 255: np.hanning(258)[1:-1]."""
  return np.hanning(W + 2)[1:-1].copy()


def _pi(dtype):
  return dtype(4) * np.arctan(dtype(1))


def band_table():
  """int [15, 2]: (lo, hi) of every band; band b sums bins lo .. hi - 1."""
  f = np.linspace(0, FS, NFFT + 1)[:NFFT // 2 + 1]
  k = np.arange(BANDS, dtype=np.float64)
  fl = MIN_FREQ * 2.0 ** ((2 * k - 1) / 6)
  fh = MIN_FREQ * 2.0 ** ((2 * k + 1) / 6)
  lo = [int(np.argmin((f - v) ** 2)) for v in fl]
  hi = [int(np.argmin((f - v) ** 2)) for v in fh]
  return np.array(list(zip(lo, hi)), dtype=np.int64)


def frame_count(n):
  """F0(n): the starts are range(0, n - W, H)."""
  return len(range(0, n - W, H))


def _frames(x, w):
  return np.array([w * x[i:i + W] for i in range(0, len(x) - W, H)]).reshape(-1, W)


def _overlap_add(frames, dtype):
  out = np.zeros((len(frames) - 1) * H + W, dtype=dtype)
  for i, f in enumerate(frames):
    out[i * H:i * H + W] += f
  return out


def _silence_free(x, y, w, dtype):
  """(x_s, y_s, F0, K, margin): step 3.  Without a frame the signals are empty and the margin is inf."""
  xf, yf = _frames(x, w), _frames(y, w)
  if len(xf) == 0:
    return np.zeros(0, dtype), np.zeros(0, dtype), 0, 0, float("inf")
  e = 20 * np.log10(np.sqrt(np.sum(xf * xf, axis=1)) + dtype(EPS))
  gap = (np.max(e) - dtype(DYN_RANGE)) - e
  mask = gap < 0
  return _overlap_add(xf[mask], dtype), _overlap_add(yf[mask], dtype), len(xf), int(mask.sum()), float(np.min(np.abs(gap)))


def _normalise(a, axis, eps):
  a = a - np.mean(a, axis=axis, keepdims=True)
  return a / (np.sqrt(np.sum(a * a, axis=axis, keepdims=True)) + eps)


def _correlate(X, Y, dtype):
  """(stoi, estoi, J) of the band spectra X, Y [15, F]: step 5."""
  F = X.shape[1]
  J = max(F - (N - 1), 0)
  if J == 0:
    return float("nan"), float("nan"), 0
  eps = dtype(EPS)
  xs = np.array([X[:, m - N:m] for m in range(N, F + 1)])                       # [J, 15, 30]
  ys = np.array([Y[:, m - N:m] for m in range(N, F + 1)])
  norm = lambda a: np.sqrt(np.sum(a * a, axis=2, keepdims=True))
  alpha = norm(xs) / (norm(ys) + eps)
  clip = dtype(1) + dtype(10) ** (dtype(-BETA) / dtype(20))
  yp = np.minimum(alpha * ys, xs * clip)
  d = np.sum(_normalise(xs, 2, eps) * _normalise(yp, 2, eps)) / dtype(BANDS * J)
  xn = _normalise(_normalise(xs, 2, eps), 1, eps)
  yn = _normalise(_normalise(ys, 2, eps), 1, eps)
  e = np.sum(np.sum(xn * yn / dtype(N), axis=(1, 2))) / dtype(J)
  return d, e, J


def _result(d, e, F0, K, J, margin):
  return {"stoi": float(d), "estoi": float(e), "frames": F0, "frames_kept": K, "segments": J, "margin": margin}


def stoi(x, y):
  """{"stoi", "estoi", "frames" (F0), "frames_kept" (K), "segments" (J), "margin"} of the pair; margin = min over the frames
  of |max(e) - 40 - e[t]| in dB, the distance of the closest frame to the energy gate (inf without a frame)."""
  n = min(len(x), len(y))
  x, y = np.asarray(x[:n], np.float64), np.asarray(y[:n], np.float64)
  w = window()
  xs, ys, F0, K, margin = _silence_free(x, y, w, np.float64)
  table = band_table()

  def spectra(s):
    f = _frames(s, w)
    if len(f) == 0:
      return np.zeros((BANDS, 0))
    p = np.abs(np.fft.rfft(f, n=NFFT, axis=1)) ** 2                             # [F, 257]
    return np.sqrt(np.array([p[:, lo:hi].sum(axis=1) for lo, hi in table]))

  d, e, J = _correlate(spectra(xs), spectra(ys), np.float64)
  return _result(d, e, F0, K, J, margin)


def stoi_longdouble(x, y):
  """The same definition with every operation in np.longdouble and a direct DFT over bins 7 .. 218; the window's values
  are the fp64 ones (the definition makes the window in fp64)."""
  L = np.longdouble
  n = min(len(x), len(y))
  x, y = np.asarray(x[:n], np.float64).astype(L), np.asarray(y[:n], np.float64).astype(L)
  w = window().astype(L)
  xs, ys, F0, K, margin = _silence_free(x, y, w, L)
  table = band_table()
  k = np.arange(BIN_LO, BIN_HI, dtype=L)[:, None]
  j = np.arange(W, dtype=L)[None, :]
  ang = L(2) * _pi(L) * np.fmod(k * j, L(NFFT)) / L(NFFT)
  cos, sin = np.cos(ang), np.sin(ang)                                           # [212, 256]

  def spectra(s):
    f = _frames(s, w)
    if len(f) == 0:
      return np.zeros((BANDS, 0), L)
    re, im = f @ cos.T, f @ sin.T                                               # [F, 212]
    p = re * re + im * im
    return np.sqrt(np.array([p[:, lo - BIN_LO:hi - BIN_LO].sum(axis=1) for lo, hi in table]))

  d, e, J = _correlate(spectra(xs), spectra(ys), L)
  return _result(d, e, F0, K, J, margin)
