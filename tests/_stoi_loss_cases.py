"""The shared inputs of the STOI-loss tests, built at 10 kHz with seeded generators, and the oracle's gradients computed once
per case and shared (tests/_stoi_loss_oracle.py).  Every case keeps the oracle's margin to the energy gate at 1e-3 dB or
more (tests/test_stoi_loss_cpu.py), so the device and the oracle cannot disagree on the kept frames.

  j1      4 224 samples, ungated: F0 = K = 31, F = 30, J = 1, the smallest case with a segment
  j5      J = 5: more segments than one workgroup of the forward's segment kernel holds (4)
  f33     F = 33: across the 8-frame tile of the band kernels
  gated   five silent frames in the middle, a gated first and a gated last frame: the kept list is not contiguous
  loud    a 1 kHz burst in y far above a quiet stretch of x inside the one segment: the clip branch wins there
  silent  y = 0: the values are exactly 0.0 and the gradient exactly zero
  short   F0 = 20: no segment (J = 0)
"""
import functools

import numpy as np

import _stoi_loss_oracle as lo
import _stoi_oracle as oracle

# Rounding yardstick of the gradient: Y = max |g_rfft - g_direct| / max |g| between the oracle's two DFT forms, the largest
# over NAMES with (g_stoi, g_estoi) = WEIGHTS, computed on the CPU by tests/test_stoi_loss_cpu.py (which asserts that the
# value stated here is not below what it measures): 1.81e-15 when this was written, rounded up.  The device bar is
# 100 Y max |g|, the factor 100 for fused multiply-adds and the kernels' longer serial chains.  The device's measured
# distance max |g_device - g_rfft| / max |g| over the same cases, measured on MI355X: 2.0e-15 (tests/test_gpu_stoi_loss.py prints it per case), a hundredth of the bar.
Y = 2e-15
WEIGHTS = (1.0, 0.5)
NAMES = ("j1", "j5", "f33", "gated", "loud", "silent")
MIN_MARGIN = 1e-3

SR = 22050
N_22K = 10000                                    # 4 536 samples at 10 kHz: F0 = 34, J = 4
LENGTHS_22K = (10000, 9600, 5000)                # 34, 33 and 16 frames at 10 kHz: the last one has no segment


def _noise(frames, seed, scale=0.1):
  return scale * np.random.default_rng(seed).standard_normal(oracle.W + oracle.H * frames)


@functools.lru_cache(maxsize=None)
def pair(name):
  """(x, y) fp32 at 10 kHz."""
  H = oracle.H
  if name in ("j1", "j5", "f33", "short", "silent", "loud"):
    frames = {"j1": 31, "j5": 35, "f33": 34, "short": 20, "silent": 31, "loud": 31}[name]
    x = _noise(frames, 21 + frames)
    if name == "loud":
      x[10 * H:16 * H] *= 0.1                                                  # quiet, not gated, where y will be loud
    y = x + _noise(frames, 77 + frames, 0.05)
    if name == "silent":
      y = np.zeros_like(x)
    if name == "loud":
      t = np.arange(len(x)) / oracle.FS
      burst = 2.0 * np.sin(2 * np.pi * 1000.0 * t)
      burst[:10 * H] = 0.0
      burst[16 * H:] = 0.0
      y = y + burst
  elif name == "gated":
    frames = 50
    x = _noise(frames, 5)
    x[:2 * H] *= 1e-4                                                          # frame 0 is gated, frame 1 is not
    x[(frames - 1) * H:] *= 1e-4                                               # the last frame and the tail behind it
    x[20 * H:26 * H] = 0.0                                                     # frames 20 .. 24
    y = x + _noise(frames, 6, 0.05)
  else:
    raise KeyError(name)
  return x.astype(np.float32), y.astype(np.float32)


@functools.lru_cache(maxsize=None)
def reference(name, dft="rfft"):
  """(d_y fp64 [n], stoi, estoi, info) of the case with the weights WEIGHTS."""
  x, y = pair(name)
  return lo.gradient(x, y, WEIGHTS[0], WEIGHTS[1], dft)


def bar(g):
  """The device bar of a gradient whose oracle is g."""
  return 100.0 * Y * float(np.max(np.abs(g))) if len(g) else 0.0


@functools.lru_cache(maxsize=None)
def pair_22k():
  """(x, y) fp32 [3, N_22K] at 22 050 Hz: smoothed noise so that most of the energy lies below 5 kHz."""
  rng = np.random.default_rng(9)
  k = np.hanning(9)
  k /= k.sum()
  x = np.stack([np.convolve(rng.standard_normal(N_22K + 8), k, "valid") for _ in LENGTHS_22K]) * 0.3
  y = x + 0.05 * rng.standard_normal(x.shape)
  return x.astype(np.float32), y.astype(np.float32)
