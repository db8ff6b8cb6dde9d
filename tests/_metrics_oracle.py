"""numpy fp64 restatement of the validation metrics (include/waveglow_amd.h: wg_metrics_*), written
from the formulas alone: the same sum order over the feature axis and the same tie order as the kernels.  A helper, not
a test module."""
import itertools

import numpy as np

UP, LEFT, DIAG = 0, 1, 2
ORDER = (UP, LEFT, DIAG)                     # (i-1, j), (i, j-1), (i-1, j-1): the first minimal predecessor wins
OTHER_ORDERS = [p for p in itertools.permutations(ORDER) if p != ORDER]


def dct_basis(n_mel, n_mfcc):
  """[n_mfcc, n_mel]: row k-1 = sqrt(2/N) cos(pi k (2n+1) / (2N)), k = 1..n_mfcc."""
  k = np.arange(1, n_mfcc + 1, dtype=np.float64)[:, None]
  n = np.arange(n_mel, dtype=np.float64)[None, :]
  return np.sqrt(2.0 / n_mel) * np.cos(np.pi * k * (2 * n + 1) / (2 * n_mel))


def mfcc(mel, n_mfcc=16):
  """mel [n_mel, T] -> fp64 [n_mfcc, T]: products and the sum over n ascending in fp64, not rounded to fp32."""
  mel = np.asarray(mel, dtype=np.float64)
  basis = dct_basis(mel.shape[0], n_mfcc)
  acc = np.zeros((n_mfcc, mel.shape[1]))
  for n in range(mel.shape[0]):
    acc = acc + basis[:, n:n + 1] * mel[n:n + 1, :]
  return acc


def frame_distances(a, b):
  """D[i, j] = sqrt(sum_k (a[k, i] - b[k, j])^2), k outermost and ascending."""
  a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
  s = np.zeros((a.shape[1], b.shape[1]))
  for k in range(a.shape[0]):
    d = a[k][:, None] - b[k][None, :]
    s = s + d * d
  return np.sqrt(s)


def dtw(a, b, order=ORDER):
  """Exact DTW of the columns of a [K, Ta] and b [K, Tb], one anti-diagonal per step.
  Returns (cost, frames, decision margin): the margin is the smallest (second - best) / second over all cells with at
  least two finite predecessors (infinity when there is no such cell)."""
  D = frame_distances(a, b)
  Ta, Tb = D.shape
  C = np.full((Ta + 1, Tb + 1), np.inf)            # C[i + 1, j + 1] = cost of cell (i, j); row / column 0 = no cell
  L = np.zeros((Ta + 1, Tb + 1), dtype=np.int64)
  C[1, 1], L[1, 1] = D[0, 0], 1
  margin = np.inf
  for d in range(1, Ta + Tb - 1):
    i = np.arange(max(0, d - Tb + 1), min(Ta - 1, d) + 1)
    j = d - i
    pc = np.stack([C[i, j + 1], C[i + 1, j], C[i, j]])          # up, left, diagonal
    pl = np.stack([L[i, j + 1], L[i + 1, j], L[i, j]])
    best, bl = pc[order[0]], pl[order[0]]
    for p in order[1:]:
      take = pc[p] < best
      best, bl = np.where(take, pc[p], best), np.where(take, pl[p], bl)
    C[i + 1, j + 1] = D[i, j] + best
    L[i + 1, j + 1] = bl + 1
    srt = np.sort(pc, axis=0)
    two = np.isfinite(srt[1])
    if two.any():
      second, first = srt[1][two], srt[0][two]
      gap = np.where(second > 0, (second - first) / np.where(second > 0, second, 1.0), 0.0)
      margin = min(margin, float(gap.min()))
  return float(C[Ta, Tb]), int(L[Ta, Tb]), margin


def padded_mcd(fa, fb):
  """(mcd, penalty, frames) of MFCCs fa [K, Ta], fb [K, Tb], the shorter zero behind its end."""
  fa, fb = np.asarray(fa, dtype=np.float64), np.asarray(fb, dtype=np.float64)
  Ta, Tb = fa.shape[1], fb.shape[1]
  F = max(Ta, Tb)
  pa, pb = np.zeros((fa.shape[0], F)), np.zeros((fb.shape[0], F))
  pa[:, :Ta], pb[:, :Tb] = fa, fb
  s = np.zeros(F)
  for k in range(fa.shape[0]):
    d = pa[k] - pb[k]
    s = s + d * d
  return float(np.sum(np.sqrt(s)) / F), 2.0 - (Ta + Tb) / F, F


def cosine(mel_a, mel_b):
  """1 - mean_c (1 - u.v / (|u| |v|)), the shorter mel zero-padded in time, score 1 where |u| |v| = 0."""
  a, b = np.asarray(mel_a, dtype=np.float64), np.asarray(mel_b, dtype=np.float64)
  F = max(a.shape[1], b.shape[1])
  pa, pb = np.zeros((a.shape[0], F)), np.zeros((b.shape[0], F))
  pa[:, :a.shape[1]], pb[:, :b.shape[1]] = a, b
  scores = []
  for u, v in zip(pa, pb):
    den = np.sqrt(np.dot(u, u)) * np.sqrt(np.dot(v, v))
    scores.append(1.0 if den == 0 else 1.0 - np.dot(u, v) / den)
  return 1.0 - float(np.mean(scores))


def mel_metrics(mel_a, mel_b, n_mfcc=16):
  """The seven values of one pair of fp32 mels [n_mel, Ta], [n_mel, Tb] (the MFCCs rounded to fp32 as the device's), and
  the DTW's decision margin."""
  fa = mfcc(mel_a, n_mfcc).astype(np.float32)
  fb = mfcc(mel_b, n_mfcc).astype(np.float32)
  mcd, pen, F = padded_mcd(fa, fb)
  cost, L, margin = dtw(fa, fb)
  Ta, Tb = fa.shape[1], fb.shape[1]
  return dict(mcd=mcd, penalty=pen, frames=F, mcd_dtw=cost / L, penalty_dtw=2.0 - (Ta + Tb) / L, frames_dtw=L,
              cosine=cosine(mel_a, mel_b), margin=margin)
