"""Two independent restatements of the soft-DTW of include/waveglow_amd.h (wg_softdtw_*), written from
the formulas alone.  (a) ``autograd``: torch fp64, the R recursion with ``logsumexp``, everything else by autograd.
(b) ``explicit``: numpy, the R and E recursions (Cuturi and Blondel 2017, Algorithm 2) and the gradient formulas written
out, in fp64 or ``longdouble``.  A helper, not a test module."""
import numpy as np
import torch

COSTS = ("l2", "sq")


# ----------------------------------------------------------------------------------------------- (a) torch autograd
def _safe_sqrt(s):
  """sqrt with gradient 0 at 0 (the library's convention for a root at 0)."""
  pos = s > 0
  return torch.where(pos, torch.sqrt(torch.where(pos, s, torch.ones_like(s))), torch.zeros_like(s))


def distances_torch(a, b, cost):
  """D[i, j] of a [K, Ta], b [K, Tb] (fp64 tensors), k outermost and ascending."""
  s = torch.zeros((a.shape[1], b.shape[1]), dtype=torch.float64)
  for k in range(a.shape[0]):
    d = a[k][:, None] - b[k][None, :]
    s = s + d * d
  return s if cost == "sq" else _safe_sqrt(s)


def value_torch(D, gamma):
  """R(Ta-1, Tb-1) of a distance matrix, cell by cell: softmin over the predecessors inside the matrix."""
  Ta, Tb = D.shape
  R = [[None] * Tb for _ in range(Ta)]
  for i in range(Ta):
    for j in range(Tb):
      prev = []
      if i > 0:
        prev.append(R[i - 1][j])
      if j > 0:
        prev.append(R[i][j - 1])
      if i > 0 and j > 0:
        prev.append(R[i - 1][j - 1])
      R[i][j] = D[i, j] if not prev else D[i, j] - gamma * torch.logsumexp(-torch.stack(prev) / gamma, dim=0)
  return R[Ta - 1][Tb - 1]


def autograd(a, b, gamma, cost="l2"):
  """a [K, Ta], b [K, Tb] (any float arrays) -> dict(value, E [Ta, Tb], g_a [K, Ta], g_b [K, Tb]) as fp64 numpy, for an
  upstream gradient of 1."""
  ta = torch.tensor(np.asarray(a, dtype=np.float64), requires_grad=True)
  tb = torch.tensor(np.asarray(b, dtype=np.float64), requires_grad=True)
  D = distances_torch(ta, tb, cost)
  D.retain_grad()
  v = value_torch(D, float(gamma))
  v.backward()
  return dict(value=float(v.detach()), E=D.grad.numpy().copy(), g_a=ta.grad.numpy().copy(), g_b=tb.grad.numpy().copy())


# ---------------------------------------------------------------------------------------------- (b) numpy, explicit
def distances(a, b, cost, dtype=np.float64):
  """(D, S): S[i, j] = sum_k ascending (a[k, i] - b[k, j])^2, D = S or its root."""
  a, b = np.asarray(a, dtype=dtype), np.asarray(b, dtype=dtype)
  s = np.zeros((a.shape[1], b.shape[1]), dtype=dtype)
  for k in range(a.shape[0]):
    d = a[k][:, None] - b[k][None, :]
    s = s + d * d
  return (s if cost == "sq" else np.sqrt(s)), s


def explicit(a, b, gamma, cost="l2", dtype=np.float64):
  """dict(value, R, E, g_a, g_b, D) in ``dtype``, for an upstream gradient of 1."""
  a, b = np.asarray(a, dtype=dtype), np.asarray(b, dtype=dtype)
  g = dtype(gamma)
  D, _ = distances(a, b, cost, dtype)
  Ta, Tb = D.shape
  inf = dtype(np.inf)
  R = np.full((Ta, Tb), inf, dtype=dtype)
  for i in range(Ta):
    for j in range(Tb):
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
      if i == Ta - 1 and j == Tb - 1:
        E[i, j] = 1
        continue
      e = dtype(0)
      if i + 1 < Ta:
        e = e + E[i + 1, j] * np.exp((R[i + 1, j] - R[i, j] - D[i + 1, j]) / g)
      if j + 1 < Tb:
        e = e + E[i, j + 1] * np.exp((R[i, j + 1] - R[i, j] - D[i, j + 1]) / g)
      if i + 1 < Ta and j + 1 < Tb:
        e = e + E[i + 1, j + 1] * np.exp((R[i + 1, j + 1] - R[i, j] - D[i + 1, j + 1]) / g)
      E[i, j] = e
  if cost == "sq":
    W = 2 * E
  else:
    pos = D > 0
    W = np.where(pos, E / np.where(pos, D, 1), 0).astype(dtype)
  g_a, g_b = np.zeros_like(a), np.zeros_like(b)
  for k in range(a.shape[0]):
    diff = a[k][:, None] - b[k][None, :]
    wd = W * diff
    for j in range(Tb):
      g_a[k] = g_a[k] + wd[:, j]
    for i in range(Ta):
      g_b[k] = g_b[k] - wd[i, :]
  return dict(value=R[Ta - 1, Tb - 1], R=R, E=E, g_a=g_a, g_b=g_b, D=D)


def distance(x, y):
  """The largest distance of two results over the value (relative to max(1, |value|)), E (absolute) and both gradients
  (relative to max |g| over both): how the accuracy bar of tests/test_gpu_softdtw.py measures."""
  gmax = max(float(np.abs(np.asarray(y["g_a"], dtype=np.float64)).max()),
             float(np.abs(np.asarray(y["g_b"], dtype=np.float64)).max()))
  gmax = gmax if gmax > 0 else 1.0
  dv = abs(float(x["value"]) - float(y["value"])) / max(1.0, abs(float(y["value"])))
  de = float(np.abs(np.asarray(x["E"], dtype=np.longdouble) - y["E"]).max())
  dg = max(float(np.abs(np.asarray(x["g_a"], dtype=np.longdouble) - y["g_a"]).max()),
           float(np.abs(np.asarray(x["g_b"], dtype=np.longdouble) - y["g_b"]).max())) / gmax
  return dict(value=dv, E=de, grad=dg, worst=max(dv, de, dg), gmax=gmax)
