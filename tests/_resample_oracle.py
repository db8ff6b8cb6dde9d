"""The resampler's definition in numpy fp64 loops (include/waveglow_amd.h: wg_resample), written
independently of waveglow_amd/resample.py: the closed form of ``scipy.signal.resample_poly(x, up, down)`` with its defaults.

    M = max(up, down), half = 10 M, h = up * firwin(2 half + 1, 1 / M, window=('kaiser', 5.0))
    out_len(len) = ceil(len up / down)
    y[n] = sum over m ascending, 0 <= m < len with 0 <= half + n down - m up <= 2 half, of x[m] h[half + n down - m up]

``resample`` keeps fp64; ``resample_device`` emulates the device's last step (one rounding to fp32, then the optional
clip).  The sum starts at +0.0 and adds the products one by one in ascending m, each product rounded on its own -- which
is what the kernel does, so the emulation is expected to give the kernel's bits."""
import math

import numpy as np

RATIOS = ((320, 147), (147, 320), (1, 2), (2, 1), (441, 320), (320, 441), (147, 640))     # (up, down)


def taps(up: int, down: int):
  """(half, h) of the reduced ratio up / down."""
  from scipy.signal import firwin
  assert math.gcd(up, down) == 1 and up != down
  M = max(up, down)
  half = 10 * M
  return half, up * firwin(2 * half + 1, 1.0 / M, window=("kaiser", 5.0))


def out_len(n: int, up: int, down: int) -> int:
  return -((-n * up) // down)


def resample(x, up: int, down: int) -> np.ndarray:
  """fp64 result of the closed form for one utterance ``x`` (any float dtype; widened to fp64 exactly)."""
  x = np.asarray(x).astype(np.float64)
  half, h = taps(up, down)
  n_in = x.shape[0]
  y = np.zeros(out_len(n_in, up, down), dtype=np.float64)
  for n in range(y.shape[0]):
    c = half + n * down
    m_lo = max(0, -((2 * half - c) // up))           # ceil((c - 2 half) / up)
    m_hi = min(n_in - 1, c // up)
    acc = np.float64(0.0)
    for m in range(m_lo, m_hi + 1):
      acc = acc + x[m] * h[c - m * up]
    y[n] = acc
  return y


def resample_device(x, up: int, down: int, clip: bool = False) -> np.ndarray:
  """The device's result for fp32 ``x``: the fp64 sum rounded to fp32 once, then clamped to [-1, 1] with ``clip``."""
  assert np.asarray(x).dtype == np.float32
  y = resample(x, up, down).astype(np.float32)
  return np.clip(y, np.float32(-1), np.float32(1)) if clip else y


def branch_l1(up: int, down: int) -> float:
  """L of the tolerance: the largest polyphase branch's L1 norm, max over p of sum_k |h[p + k up]|."""
  _, h = taps(up, down)
  return max(float(np.abs(h[p::up]).sum()) for p in range(up))
