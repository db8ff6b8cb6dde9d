"""The cases (K, Ta, Tb, gamma) of the soft-DTW tests, their inputs and their references, computed once per process and
shared by tests/test_softdtw_cpu.py and tests/test_gpu_softdtw.py.  A helper, not a test module.

The wavefront kernels take rows-per-thread variants 1..4 by the row count, (tmax_a + 1023) // 1024, as the exact DTW does:
the last four cases are the smallest shapes that reach the variants 2, 3 and 4, with a mirror of the first."""
import functools

import numpy as np

import _softdtw_oracle as O

CASES = (
  (16, 1, 1, 1.0),
  (16, 1, 7, 0.5),
  (16, 9, 1, 0.5),
  (3, 5, 6, 1.0),
  (16, 37, 41, 1.0),
  (80, 33, 30, 0.1),
  (16, 70, 45, 0.01),        # crosses a wave at 64 rows
  (4, 1025, 3, 1.0),         # two rows per thread
  (4, 3, 1025, 1.0),         # its mirror: one thread row, 1025 columns
  (4, 2049, 2, 1.0),         # three rows per thread
  (4, 4096, 1, 1.0),         # four rows per thread, the largest row count
)
COSTS = O.COSTS
IDS = [f"K{K}-{Ta}x{Tb}-g{g:g}" for K, Ta, Tb, g in CASES]


def inputs(case, seed=0):
  """(a [K, Ta], b [K, Tb]) fp32: a smooth random walk per feature row plus noise, so that neighbouring frames are close
  (as speech features are) and the alignment is not degenerate; b is a rescaled, shifted relative of a's process."""
  K, Ta, Tb, _ = case
  rng = np.random.default_rng(1000 * seed + 7 * K + 131 * Ta + 17 * Tb)
  def walk(T):
    return np.cumsum(rng.standard_normal((K, T)) * 0.4, axis=1) + rng.standard_normal((K, 1))
  a = walk(Ta) + 0.1 * rng.standard_normal((K, Ta))
  b = walk(Tb) + 0.1 * rng.standard_normal((K, Tb))
  return a.astype(np.float32), b.astype(np.float32)


@functools.lru_cache(maxsize=None)
def reference(index, cost):
  """dict for case ``index`` and ``cost``: a, b, gamma, the three oracle results ``auto`` (a), ``f64`` and ``ld`` (b, fp64 and
  longdouble), Y (their largest distance: (a) against (b) in fp64) and rmax (the largest finite |R|).  Treat as read-only."""
  case = CASES[index]
  a, b = inputs(case)
  gamma = case[3]
  auto = O.autograd(a, b, gamma, cost)
  f64 = O.explicit(a, b, gamma, cost, np.float64)
  ld = O.explicit(a, b, gamma, cost, np.longdouble)
  y = O.distance(auto, f64)
  return dict(case=case, a=a, b=b, gamma=gamma, auto=auto, f64=f64, ld=ld, Y=y["worst"], Y_parts=y,
              rmax=float(np.abs(ld["R"]).max()))


def bar(ref):
  """The accuracy bar of a device result for this case: 100 max(Y, 2^-52 (Ta + Tb) max(1, max|R| / gamma)).  Y is the
  disagreement of the two oracle formulations, the second term the rounding of the exponent arguments (2^-53 |R| / gamma
  each, along at most Ta + Tb cells, doubled); the factor 100 is for fused multiply-adds and the device exp / log."""
  _, Ta, Tb, gamma = ref["case"]
  return 100.0 * max(ref["Y"], 2.0 ** -52 * (Ta + Tb) * max(1.0, ref["rmax"] / gamma))
