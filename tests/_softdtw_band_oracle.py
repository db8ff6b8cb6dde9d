"""The soft-DTW of include/waveglow_amd.h inside a Sakoe-Chiba band (wg_softdtw_banded_*) and the
soft-DTW divergence, restated from the formulas alone, as tests/_softdtw_oracle.py restates the dense recursion.
(a) ``autograd``: torch fp64, ``logsumexp`` over the in-band predecessors, everything else by autograd.  (b) ``explicit``:
numpy, the masked R and E recursions and the gradient formulas written out, in fp64 or ``longdouble``.  (c) ``diagonal``:
the same recursions one anti-diagonal per step over the interval lo(d) .. hi(d), for shapes where cell-by-cell Python takes
too long (value and E only).  ``dtw`` is the exact warping cost inside the band, ``divergence`` the combination
v_ab - (v_aa + v_bb) / 2 with its gradients.  (a) and (b) take the band from the predicate, (c) from the interval formulas.
A helper, not a test module."""
import numpy as np
import torch

import _softdtw_oracle as O

COSTS = O.COSTS


# ---------------------------------------------------------------------------------------------------------- geometry
def in_band(i, j, Ta, Tb, w):
  """|i m - j n| <= w max(n, m) with n = Ta - 1, m = Tb - 1, in Python integers."""
  n, m = Ta - 1, Tb - 1
  return abs(i * m - j * n) <= w * max(n, m)


def mask(Ta, Tb, w):
  """bool [Ta, Tb] by the predicate, cell by cell.  ``w`` None: the whole matrix."""
  if w is None:
    return np.ones((Ta, Tb), dtype=bool)
  return np.array([[in_band(i, j, Ta, Tb, w) for j in range(Tb)] for i in range(Ta)], dtype=bool)


def interval(d, Ta, Tb, w):
  """(lo, hi) of anti-diagonal d by the closed formulas (floor division of Python integers)."""
  n, m = Ta - 1, Tb - 1
  if n + m == 0:
    return 0, 0
  W = w * max(n, m)
  return max(0, d - m, -((W - d * n) // (n + m))), min(n, d, (d * n + W) // (n + m))


# ----------------------------------------------------------------------------------------------- (a) torch autograd
def value_torch(D, gamma, M):
  """R(Ta-1, Tb-1) of a distance matrix under the mask M, cell by cell: softmin over the in-band predecessors."""
  Ta, Tb = D.shape
  R = [[None] * Tb for _ in range(Ta)]
  for i in range(Ta):
    for j in range(Tb):
      if not M[i, j]:
        continue
      prev = [R[p][q] for p, q in ((i - 1, j), (i, j - 1), (i - 1, j - 1)) if p >= 0 and q >= 0 and M[p, q]]
      R[i][j] = D[i, j] if not prev else D[i, j] - gamma * torch.logsumexp(-torch.stack(prev) / gamma, dim=0)
  return R[Ta - 1][Tb - 1]


def autograd(a, b, gamma, cost="l2", w=None):
  """a [K, Ta], b [K, Tb] -> dict(value, E [Ta, Tb], g_a, g_b) as fp64 numpy, for an upstream gradient of 1."""
  ta = torch.tensor(np.asarray(a, dtype=np.float64), requires_grad=True)
  tb = torch.tensor(np.asarray(b, dtype=np.float64), requires_grad=True)
  D = O.distances_torch(ta, tb, cost)
  D.retain_grad()
  v = value_torch(D, float(gamma), mask(ta.shape[1], tb.shape[1], w))
  v.backward()
  return dict(value=float(v.detach()), E=D.grad.numpy().copy(), g_a=ta.grad.numpy().copy(), g_b=tb.grad.numpy().copy())


# ---------------------------------------------------------------------------------------------- (b) numpy, explicit
def explicit(a, b, gamma, cost="l2", w=None, dtype=np.float64):
  """dict(value, R, E, g_a, g_b, D) in ``dtype``, for an upstream gradient of 1; R is +infinity and E 0 outside the band."""
  a, b = np.asarray(a, dtype=dtype), np.asarray(b, dtype=dtype)
  g = dtype(gamma)
  D, _ = O.distances(a, b, cost, dtype)
  Ta, Tb = D.shape
  M = mask(Ta, Tb, w)
  inf = dtype(np.inf)
  R = np.full((Ta, Tb), inf, dtype=dtype)
  for i in range(Ta):
    for j in range(Tb):
      if not M[i, j]:
        continue
      if i == 0 and j == 0:
        R[0, 0] = D[0, 0]
        continue
      x = np.array([R[i - 1, j] if i > 0 else inf, R[i, j - 1] if j > 0 else inf,
                    R[i - 1, j - 1] if i > 0 and j > 0 else inf], dtype=dtype)
      m = x.min()
      t = np.zeros(3, dtype=dtype)
      fin = np.isfinite(x)
      t[fin] = np.exp(-(x[fin] - m) / g)
      R[i, j] = D[i, j] + (m - g * np.log((t[0] + t[1]) + t[2]))
  E = np.zeros((Ta, Tb), dtype=dtype)
  for i in range(Ta - 1, -1, -1):
    for j in range(Tb - 1, -1, -1):
      if not M[i, j]:
        continue
      if i == Ta - 1 and j == Tb - 1:
        E[i, j] = 1
        continue
      e = dtype(0)
      for p, q in ((i + 1, j), (i, j + 1), (i + 1, j + 1)):
        if p < Ta and q < Tb and M[p, q]:
          e = e + E[p, q] * np.exp((R[p, q] - R[i, j] - D[p, q]) / g)
      E[i, j] = e
  if cost == "sq":
    Wt = 2 * E
  else:
    pos = D > 0
    Wt = np.where(pos, E / np.where(pos, D, 1), 0).astype(dtype)
  g_a, g_b = np.zeros_like(a), np.zeros_like(b)
  for k in range(a.shape[0]):
    wd = Wt * (a[k][:, None] - b[k][None, :])
    for j in range(Tb):
      g_a[k] = g_a[k] + wd[:, j]
    for i in range(Ta):
      g_b[k] = g_b[k] - wd[i, :]
  return dict(value=R[Ta - 1, Tb - 1], R=R, E=E, g_a=g_a, g_b=g_b, D=D)


# ------------------------------------------------------------------------------------------ (c) one diagonal per step
def diagonal(a, b, gamma, cost="l2", w=1, dtype=np.float64, want_e=True):
  """dict(value, E [Ta, Tb] or None, rmax): the masked recursions with the rows lo(d) .. hi(d) of a diagonal at once."""
  a, b = np.asarray(a, dtype=dtype), np.asarray(b, dtype=dtype)
  g = dtype(gamma)
  K, Ta = a.shape
  Tb = b.shape[1]
  nd = Ta + Tb - 1
  inf = dtype(np.inf)

  def dist(i, j):
    s = np.zeros(i.shape, dtype=dtype)
    for k in range(K):
      df = a[k, i] - b[k, j]
      s = s + df * df
    return s if cost == "sq" else np.sqrt(s)

  rows, Rd, Dd = [], [], []                         # per diagonal: the row indices, R and d of the interval
  p1 = np.full(Ta + 1, inf, dtype=dtype)            # p[i + 1] = R(i, .) of the diagonal before; p[0] stands for row -1
  p2 = p1.copy()
  for d in range(nd):
    lo, hi = interval(d, Ta, Tb, w)
    i = np.arange(lo, hi + 1)
    dd = dist(i, d - i)
    if d == 0:
      r = dd.copy()
    else:
      x = np.stack([p1[i], p1[i + 1], p2[i]])        # (i-1, j), (i, j-1), (i-1, j-1)
      m = x.min(axis=0)
      with np.errstate(invalid="ignore"):
        t = np.where(np.isfinite(x), np.exp(-(x - m) / g), 0)
      r = dd + (m - g * np.log((t[0] + t[1]) + t[2]))
    cur = np.full(Ta + 1, inf, dtype=dtype)
    cur[i + 1] = r
    p2, p1 = p1, cur
    rows.append(i), Rd.append(r), Dd.append(dd)
  value = Rd[-1][-1]
  rmax = max(float(np.abs(r).max()) for r in Rd)
  if not want_e:
    return dict(value=value, E=None, rmax=rmax)
  E = np.zeros((Ta, Tb), dtype=dtype)
  # e[i] = E(i, .), q[i] = R - d of a later diagonal, zeros outside its interval; index Ta stands for row Ta
  e1, q1, in1 = np.zeros(Ta + 1, dtype=dtype), np.zeros(Ta + 1, dtype=dtype), np.zeros(Ta + 1, dtype=bool)
  e2, q2, in2 = e1.copy(), q1.copy(), in1.copy()
  for d in range(nd - 1, -1, -1):
    i, r = rows[d], Rd[d]
    if d == nd - 1:
      e = np.ones(1, dtype=dtype)
    else:
      e = np.zeros(i.shape, dtype=dtype)
      for ee, qq, inn, s in ((e1, q1, in1, i + 1), (e1, q1, in1, i), (e2, q2, in2, i + 1)):
        arg = np.where(inn[s], (qq[s] - r) / g, 0)
        e = e + np.where(inn[s], ee[s] * np.exp(arg), 0)
    E[i, d - i] = e
    ce, cq, cin = np.zeros(Ta + 1, dtype=dtype), np.zeros(Ta + 1, dtype=dtype), np.zeros(Ta + 1, dtype=bool)
    ce[i], cq[i], cin[i] = e, r - Dd[d], True
    e2, q2, in2, e1, q1, in1 = e1, q1, in1, ce, cq, cin
  return dict(value=value, E=E, rmax=rmax)


# ------------------------------------------------------------------------------------------------- exact DTW, banded
def dtw(a, b, cost="l2", w=None):
  """The cost of the best warping path inside the band: a plain min over the in-band predecessors, fp64."""
  D, _ = O.distances(a, b, cost)
  Ta, Tb = D.shape
  M = mask(Ta, Tb, w)
  C = np.full((Ta, Tb), np.inf)
  for i in range(Ta):
    for j in range(Tb):
      if not M[i, j]:
        continue
      prev = [C[p, q] for p, q in ((i - 1, j), (i, j - 1), (i - 1, j - 1)) if p >= 0 and q >= 0]
      C[i, j] = D[i, j] + (min(prev) if prev else 0.0)
  return float(C[Ta - 1, Tb - 1])


# --------------------------------------------------------------------------------------------------------- divergence
def divergence(a, b, gamma, cost="l2", w=None, dtype=np.float64, fn=None):
  """dict(value, g_a, g_b, v_ab, v_aa, v_bb, parts): D = v_ab - (v_aa + v_bb) / 2 and its gradients from three runs of
  ``fn`` (``explicit`` in ``dtype`` by default, or ``autograd``); a self-term's gradient is the sum of both of its sides."""
  if fn is None:
    def fn(x, y):
      return explicit(x, y, gamma, cost, w, dtype)
  ab, aa, bb = fn(a, b), fn(a, a), fn(b, b)
  half = dtype(0.5)
  return dict(value=ab["value"] - half * (aa["value"] + bb["value"]),
              g_a=ab["g_a"] - half * (aa["g_a"] + aa["g_b"]), g_b=ab["g_b"] - half * (bb["g_a"] + bb["g_b"]),
              v_ab=ab["value"], v_aa=aa["value"], v_bb=bb["value"], parts=(ab, aa, bb))
