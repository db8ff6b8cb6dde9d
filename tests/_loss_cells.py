"""Per-cell and per-sample error bounds for the STFT loss and the mel loss at the seams of the conv-STFT core
(tests/test_loss_cells_cpu.py, tests/test_gpu_loss_cells.py).

Every other comparison of the two waveform losses with their oracle is a scalar (a mean over all cells of all scales) or
one relative L2 norm per utterance, in which a kernel that is wrong in a few cells -- one frame at a tile seam, the last
frame's reflection, one M tile of one workgroup -- is diluted by all the cells that are right (the argument of
tests/_seams.py for the flow path).  Here a plane with a frame axis (the rows of the transform, the linear mels) is
compared cell by cell,

  e[b, r, f] = |got - ref| / rms over the valid cells (f < F_b) of the plane of ref ,

and a gradient sample by sample,

  e[b, s] = |got - ref| / rms over the samples of utterance b where ref != 0 ,

``ref`` restatement (a) of tests/_mel_loss_oracle.py (``torch.stft`` in fp64) on the inputs the kernel received, cropped
per utterance for a ragged batch.  The error is normalised by the plane's RMS and not by the cell's own value, so a quiet
cell needs no floor and no cell is left out.  The statistic is the maximum of e; its position is reported as utterance, row
(with its M tile ``row // 32`` and, when the GEMM has more than one workgroup along M, the workgroup that owns the tile) or
bin, frame or sample, the distance to the nearest utterance end and the distance in frames to the nearest multiple of 64.

Two bounds.  The yardstick Y of a quantity is the same maximum for restatement (b) in fp32 on the CPU (pad + unfold +
matmul with the library's fp32 basis) against (a), the largest over the input draws ``YARD_SEEDS``, computed when a test
asks for it and cached; the device is held to ``BOUND_FACTOR`` (4, the factor every loss test applies to the fp32
restatement) times Y.  The derived cap holds for every cell of the transform on its own, whatever was measured:

  |got - ref| <= (win + 2) 2^-24 sum_k |x_k| |basis_k| ,

the forward bound of an fp32 dot product of ``win`` terms in any summation order plus the rounding of the basis to fp32,
the sum formed in fp64 from the padded frame and the library's fp32 basis.  A correct kernel cannot exceed it whatever its
schedule; it is coarse (the floor of sensitivity), the yardstick is the sharp bound.

Restatement (c), ``rows_c32``, accumulates the transform in fp32 in the kernel's order (pairs of taps ascending from
``lpad``, one chain per cell): the yardstick of the cases in ``ROWS_FROM_C`` (and, for the mels formed from that transform,
``MELS_FROM_C``) is taken from it, because there the length of the chain alone, which the CPU GEMM of (b) blocks, puts a
correct kernel above 4 Y of (b); tests/test_gpu_loss_cells.py has both measured values.

The geometry arithmetic below is restated from the comments of csrc/wg_stftconv.h; tests/test_loss_cells_cpu.py holds the
case table to it.
"""
import functools
import math

import torch

import _mel_loss_oracle as O
from _ragged_ref import ragged_grad64, ragged_unfold
from test_stft_loss_cpu import fragile_bins

BOUND_FACTOR = 4                # the factor of every loss test here on the fp32 restatement
L2_FLOOR = 1e-6                 # the floor of the per-utterance L2 bound of tests/test_gpu_mel_loss.py: max(4 g32, 1e-6)
YARD_SEEDS = (0, 1, 2, 3)       # input draws of a yardstick (draw 0 is the device's): the seeds of the plane inputs
STFT_EPS = 1e-2                 # the clamp of the STFT loss at which its log-magnitude gradient is compared
K_BN, K_TW = 64, 4              # frames per workgroup; M tiles per wave at most

# ---------------------------------------------------------------- geometry (csrc/wg_stftconv.h, restated)
def ceil_div(a, b):
  return (a + b - 1) // b


def up64(n):
  return ceil_div(n, 64) * 64


def frames_of(n, hop):
  """F_b of an utterance of n samples."""
  return n // hop + 1


def gemm_nby(MT):
  """Workgroups along the MT tiles of a GEMM: at most 4 K_TW tiles each."""
  return ceil_div(MT, 4 * K_TW)


def tiles_per_wave(MT, nby):
  """Tiles per wave of the fullest workgroup: the kernel instance TW."""
  return ceil_div(ceil_div(MT, nby), 4)


def m_ranges(MT, nby):
  """[m0, m1) of every workgroup along M: y MT / nby rounded down."""
  return [(y * MT // nby, (y + 1) * MT // nby) for y in range(nby)]


def geometry(scale):
  """lpad, and per GEMM (forward: tiles of 32 basis rows; backward: tiles of 32 window taps) MT, nby, TW and the ranges."""
  n_fft, hop, win, _ = scale
  out = {"lpad": (n_fft - win) // 2}
  for leg, MT in (("f", n_fft // 32), ("b", ceil_div(win, 32))):
    nby = gemm_nby(MT)
    out["MT" + leg], out["nby" + leg], out["TW" + leg], out["m" + leg] = MT, nby, tiles_per_wave(MT, nby), m_ranges(MT, nby)
  return out


def owner(row, MT, nby):
  """The workgroup along M that owns the tile of ``row``."""
  return next(y for y, (m0, m1) in enumerate(m_ranges(MT, nby)) if m0 <= row // 32 < m1)


# ---------------------------------------------------------------- cases
# id: (n_fft, hop, win, n_mels), the smallest geometries that reach each seam of the core.  Forward GEMM: MTf = n_fft / 32
# tiles of basis rows; backward GEMM: MTb = ceil(win / 32) tiles of window taps (Wp = 32 MTb); nby = ceil(MT / 16)
# workgroups along M, TW = ceil(ceil(MT / nby) / 4) tiles per wave; a workgroup deals its tiles to 4 waves as m0 + wave + 4 t.
#   g32    MTf 1, TW 1: waves 1 .. 3 have no tile and only stage.                        MTb 1.   lpad 0
#   g64    MTf 2, TW 1: waves 2, 3 only stage.                                            MTb 2.   lpad 0
#   g160   MTf 5, TW 2: wave 0 holds tiles 0 and 4, waves 1 .. 3 repeat tile 4 (never stored).
#          MTb 5 (win 150 = 4 x 32 + 22: 10 padded taps in the last tile must be zero), TW 2.      lpad 5
#   g288   MTf 9, TW 3: wave 0 holds three tiles, waves 1 .. 3 two and a repeat.          MTb 9.   lpad 0
#   g544   MTf 17, nby 2, ranges 0 .. 8 | 8 .. 17 (8 and 9 tiles), TW 3: in the first workgroup every wave repeats a tile,
#          in the second waves 1 .. 3 do.  MTb 17 (win 530 = 16 x 32 + 18), the same split.         lpad 7
#   g1024  MTf 32, nby 2, 16 | 16, TW 4: every wave full.                                 MTb 32.  lpad 0
#   g2048  MTf 64, nby 4, 16 each, TW 4.                                                  MTb 64.  lpad 0
SCALES = {
  "g32": (32, 8, 32, 5), "g64": (64, 16, 64, 10), "g160": (160, 40, 150, 20), "g288": (288, 72, 288, 32),
  "g544": (544, 136, 530, 40), "g1024": (1024, 256, 1024, 80), "g2048": (2048, 512, 2048, 320),
  "e256": O.EMPTY_ROWS, "d256": O.DENSE_SCALE,              # the two other banks of the mel comparison (BANK_CASES)
}
# what the comment above states, held to ``geometry`` by tests/test_loss_cells_cpu.py: (MTf, nbyf, TWf, MTb, nbyb, TWb, lpad)
EXPECT = {
  "g32": (1, 1, 1, 1, 1, 1, 0), "g64": (2, 1, 1, 2, 1, 1, 0), "g160": (5, 1, 2, 5, 1, 2, 5), "g288": (9, 1, 3, 9, 1, 3, 0),
  "g544": (17, 2, 3, 17, 2, 3, 7), "g1024": (32, 2, 4, 32, 2, 4, 0), "g2048": (64, 4, 4, 64, 4, 4, 0),
}
G544_RANGES = [(0, 8), (8, 17)]

# id: (scale ids, B, N, lens or None).  F = N // hop + 1, Fp = F rounded up to 64 (the frame tiles of K_BN = 64):
#   g32     F 130: seams at 64 and 128, the last tile holds two frames
#   g64     F 129: seams at 64 and 128, the last tile holds ONE frame
#   g160    F 65, g288 F 71, g544 F 67, g1024 F 65, g2048 F 66: one seam, a last tile of 1, 7, 3, 1 and 2 frames
#   full64  F 64 = Fp: no spare column, one tile
#   g64r    lens 33 (the shortest legal one, n_fft / 2 + 1), 1023, 2051: F_b 3, 64, 129.  Utterance 0 leaves two frame tiles
#           without work, utterance 1 fills its first tile to the last column and leaves two
#   g544r   lens 273 (the shortest), 8704 + 5, 8981: F_b 3, 65, 67
#   multi   three scales in one module: the blocks of spectra and mels "scale after scale, each rounded up to 64 floats",
#           and the gather accumulating (i > 0).  F 562, 225, 67
CASES = {
  "g32": (("g32",), 2, 1035, None),
  "g64": (("g64",), 2, 2051, None),
  "g160": (("g160",), 2, 2567, None),
  "g288": (("g288",), 1, 5041, None),
  "g544": (("g544",), 2, 8981, None),
  "g1024": (("g1024",), 1, 16385, None),
  "g2048": (("g2048",), 1, 33283, None),
  "full64": (("g64",), 2, 1023, None),
  "g64r": (("g64",), 3, 2051, (33, 1023, 2051)),
  "g544r": (("g544",), 3, 8981, (273, 8704 + 5, 8981)),
  "multi": (("g64", "g160", "g544"), 2, 8981, None),
  # mel cells under the two other banks, F 65: 80 Slaney filters over 129 bins (rows of zeros, which the span tables hold as
  # empty), and the dense bank of tests/test_gpu_mel_loss.py (negative entries, zeros inside spans)
  "empty256": (("e256",), 2, 4111, None),
  "dense256": (("d256",), 2, 4111, None),
}
BANK_CASES = ["empty256", "dense256"]
EXPECT_F = {"g32": [130], "g64": [129], "g160": [65], "g288": [71], "g544": [67], "g1024": [65], "g2048": [66], "full64": [64],
            "g64r": [129], "g544r": [67], "multi": [562, 225, 67]}
EXPECT_FB = {"g64r": [3, 64, 129], "g544r": [3, 65, 67]}
SINGLE = [c for c in CASES if c != "multi" and c not in BANK_CASES]
RAGGED = [c for c in CASES if CASES[c][3] is not None]

# The seeds of the gradient comparisons, one per draw: per case "whole" (``O.inputs(B, N, seed, silent=False)``) and every
# local difference the case runs (``Case.local_inputs``), found by trying 0, 1, ... on the CPU (``search_seeds``).  At each
# of them ``qualifies`` holds; tests/test_loss_cells_cpu.py asserts it for draw 0, the input of the GPU tests.
SEEDS = {
  "g32": {"whole": (0, 1, 2, 3), "first": (0, 1, 2, 3), "last": (0, 1, 2, 3), "seam64": (0, 1, 2, 3), "seam128": (0, 1, 2, 3)},
  "g64": {"whole": (0, 1, 2, 3), "first": (0, 1, 2, 3), "last": (0, 2, 3, 4), "seam64": (0, 1, 2, 3), "seam128": (0, 1, 2, 3)},
  "g160": {"whole": (0, 1, 2, 3), "first": (0, 4, 12, 13), "last": (4, 7, 27, 28), "seam64": (0, 1, 4, 5)},
  "g288": {"whole": (0, 1, 2, 3), "first": (0, 3, 4, 5), "last": (0, 1, 2, 3), "seam64": (0, 1, 2, 3)},
  "g544": {"whole": (0, 1, 2, 3), "first": (11, 15, 17, 23), "last": (0, 3, 4, 11), "seam64": (1, 4, 9, 11)},
  "g1024": {"whole": (0, 1, 2, 3), "first": (4, 9, 13, 14), "last": (0, 1, 3, 5), "seam64": (1, 2, 4, 6)},
  "g2048": {"whole": (0, 1, 2, 3), "first": (348, 438, 611, 729), "last": (3, 7, 9, 13), "seam64": (0, 12, 13, 14)},
  "full64": {"whole": (0, 1, 2, 3), "first": (0, 1, 2, 3), "last": (0, 1, 2, 3)},
  "g64r": {"whole": (0, 1, 2, 3), "first": (0, 3, 4, 6), "last": (0, 1, 2, 3), "seam64": (0, 1, 2, 3), "seam128": (0, 1, 2, 3)},
  "g544r": {"whole": (0, 1, 2, 3), "first": (1, 5, 13, 20), "last": (0, 1, 7, 8), "seam64": (5, 9, 10, 14)},
  "multi": {"whole": (0, 1, 2, 3)},
}

# cases whose transform yardstick comes from restatement (c) (module docstring); the test's docstring has both values
ROWS_FROM_C = ("g2048",)
MELS_FROM_C = ("g2048",)        # the same for the linear mels, whose yardstick is then formed from (c)'s transform


class Case:
  def __init__(self, name):
    ids, self.B, self.N, lens = CASES[name]
    self.name = name
    self.ids = ids
    self.scales = tuple(SCALES[i] for i in ids)
    self.res = tuple(s[:3] for s in self.scales)
    self.lengths = None if lens is None else list(lens)
    self.lens = [self.N] * self.B if lens is None else list(lens)

  def banks(self):
    return [O.dense_bank() if s == O.DENSE_SCALE else O.bank(s) for s in self.scales]

  def F(self, i):
    return frames_of(self.N, self.scales[i][1])

  def Fp(self, i):
    return up64(self.F(i))

  def Fb(self, i):
    return [frames_of(n, self.scales[i][1]) for n in self.lens]

  def min_len(self):
    return max(s[0] for s in self.scales) // 2 + 1

  def plane_inputs(self, draw=0):
    """(prediction, target) of the transform and mel comparisons, which ask nothing of their inputs: seed YARD_SEEDS[draw]."""
    return O.inputs(self.B, self.N, YARD_SEEDS[draw], silent=False)

  def seed(self, draw, where):
    return SEEDS[self.name]["whole" if where is None else where][draw]

  def inputs(self, draw=0, seed=None):
    """(prediction, target) of the whole-signal gradient comparisons."""
    return O.inputs(self.B, self.N, self.seed(draw, None) if seed is None else seed, silent=False)

  # ---- local differences
  def intervals(self):
    """The local differences of a single-scale case: name -> per utterance (a, b) or None.  The first and the last
    max(hop / 2, 2) samples of every utterance (its own end for a ragged one), and hop samples centred on sample 64 hop
    (frames 63 | 64) and, where the utterance reaches it, on sample 128 hop, cut at the utterance's end."""
    hop = self.scales[0][1]
    w = max(hop // 2, 2)
    out = {"first": [(0, w) for n in self.lens], "last": [(n - w, n) for n in self.lens]}
    for name, c in (("seam64", 64 * hop), ("seam128", 128 * hop)):
      iv = [(c - hop // 2, min(c - hop // 2 + hop, n)) if n >= c else None for n in self.lens]
      if any(v is not None for v in iv):
        out[name] = iv
    return out

  def local_inputs(self, where, draw=0, seed=None):
    """The target equals the prediction everywhere except on the interval, where y = 0.5 x + 0.1 noise."""
    s = self.seed(draw, where) if seed is None else seed
    x = O.noise(self.B, self.N, s)
    y = x.clone()
    other = 0.5 * x + 0.1 * O.noise(self.B, self.N, s + 50)
    for b, iv in enumerate(self.intervals()[where]):
      if iv is not None:
        y[b, iv[0]:iv[1]] = other[b, iv[0]:iv[1]]
    return x, y

  def touching(self, where, i=0):
    """Per utterance the frames of scale i whose window holds a sample of the interval (index tensor, maybe empty)."""
    return [touching_frames(self.scales[i], n, iv) for n, iv in zip(self.lens, self.intervals()[where])]

  def support(self, where, i=0):
    """[B, N] bool: the samples under the frames of ``touching``."""
    m = torch.zeros(self.B, self.N, dtype=torch.bool)
    for b, (n, fr) in enumerate(zip(self.lens, self.touching(where, i))):
      m[b, :n] = support_of(self.scales[i], n, fr)
    return m


@functools.lru_cache(maxsize=None)
def case(name):
  return Case(name)


def _sample_index(scale, n):
  """[F, n_fft] the sample under every position of every reflect-padded frame of an utterance of n samples, and [n_fft]
  bool the positions that the window weighs (the periodic Hann window is 0 at its first tap)."""
  n_fft, hop, win, _ = scale
  p = torch.arange(frames_of(n, hop))[:, None] * hop + torch.arange(n_fft)[None, :] - n_fft // 2
  p = p.abs()
  p = torch.where(p >= n, 2 * (n - 1) - p, p)
  lpad = (n_fft - win) // 2
  weighs = torch.zeros(n_fft, dtype=torch.bool)
  weighs[lpad:lpad + win] = torch.hann_window(win, dtype=torch.float64) != 0
  return p, weighs


def touching_frames(scale, n, interval):
  if interval is None:
    return torch.zeros(0, dtype=torch.long)
  p, weighs = _sample_index(scale, n)
  hit = (p >= interval[0]) & (p < interval[1]) & weighs[None, :]
  return torch.nonzero(hit.any(1)).flatten()


def support_of(scale, n, frames):
  p, weighs = _sample_index(scale, n)
  m = torch.zeros(n, dtype=torch.bool)
  m[p[frames][:, weighs].reshape(-1)] = True
  return m


def local_margin(c):
  """Per scale the distance two mels of a local difference must keep: the device's mel cells are held to
  BOUND_FACTOR Y of their plane's RMS (``yard_mels``), so mel(x) and mel(y) are each off by at most that, and their order --
  the sign both terms of the loss take -- is theirs when they differ by more than the sum.  The RMS is that of noise at
  the inputs' level, (a) on draw 0 of the plane inputs."""
  out = []
  for i, s in enumerate(c.scales):
    W = O.bank(s)
    rms = [math.sqrt(sum(float(m.pow(2).sum()) for m in p) / sum(m.numel() for m in p))
           for p in (mels_of(O.mag_stft, s, W, sig, c.lens, torch.float64) for sig in c.plane_inputs())]
    out.append(BOUND_FACTOR * yard_mels(c.name, i, "b") * (rms[0] + rms[1]))
  return out


def qualifies(c, seed, where=None):
  """From (a) alone.  Whole signal: no fragile mel cell (tau = 1e-4) and no fragile bin of the STFT loss at eps = STFT_EPS.
  A local difference: no mel cell on the frames that touch it within ``local_margin`` (every other cell is equal by
  construction; the STFT loss takes its spectral-convergence term there, which has no sign to flip)."""
  if where is None:
    x, y = c.inputs(seed=seed)
    if O.fragile_cells(x, y, c.scales, lengths=c.lengths) != 0:
      return False
    return all(fragile_bins(x[b:b + 1, :n], y[b:b + 1, :n], c.res, eps=STFT_EPS)[0] == 0 for b, n in enumerate(c.lens))
  x, y = c.local_inputs(where, seed=seed)
  fr = [c.touching(where, i) for i in range(len(c.scales))]
  return O.fragile_cells(x, y, c.scales, lengths=c.lengths, frames=fr, margin=local_margin(c)) == 0


def search_seeds(name, where=None, n=len(YARD_SEEDS), limit=1000):
  """The first n qualifying seeds of a case (how SEEDS was made)."""
  c, out = case(name), []
  for seed in range(limit):
    if qualifies(c, seed, where):
      out.append(seed)
      if len(out) == n:
        return tuple(out)
  raise AssertionError(f"{name} {where}: only {out} qualify below {limit}")


# ---------------------------------------------------------------- the documented layouts (include/waveglow_amd.h)
def interleave(re, im):
  """(re, im) [.., K, F] -> rows [.., n_fft, F]: row 0 = re of bin 0, row 1 = re of bin n_fft / 2, rows 2p and 2p + 1 =
  (re, im) of bin p, 1 <= p < n_fft / 2."""
  half = re.shape[-2] - 1
  rows = re.new_zeros(re.shape[:-2] + (2 * half, re.shape[-1]))
  rows[..., 0, :] = re[..., 0, :]
  rows[..., 1, :] = re[..., half, :]
  rows[..., 2::2, :] = re[..., 1:half, :]
  rows[..., 3::2, :] = im[..., 1:half, :]
  return rows


def deinterleave(rows):
  """rows [.., n_fft, F] -> (re, im) [.., n_fft / 2 + 1, F], the imaginary parts of bins 0 and n_fft / 2 zero; written from
  the header's text, bin by bin."""
  n_fft = rows.shape[-2]
  half = n_fft // 2
  re = rows.new_zeros(rows.shape[:-2] + (half + 1, rows.shape[-1]))
  im = torch.zeros_like(re)
  re[..., 0, :] = rows[..., 0, :]
  re[..., half, :] = rows[..., 1, :]
  for p in range(1, half):
    re[..., p, :] = rows[..., 2 * p, :]
    im[..., p, :] = rows[..., 2 * p + 1, :]
  return re, im


def row_of(part, k, n_fft):
  """The row that holds the real (part 0) or imaginary (part 1) part of bin k."""
  if k == 0 or k == n_fft // 2:
    assert part == 0
    return 0 if k == 0 else 1
  return 2 * k + part


def layout(scales, B, N):
  """Float offsets of the blocks of the two saved buffers: spectra [(offset, shape)], mels [(offset x, offset y, shape)],
  the offset of the cell counts, and the two totals."""
  spec, mel, at, am = [], [], 0, 0
  for n_fft, hop, win, n_mels in scales:
    Fp = up64(frames_of(N, hop))
    spec.append((at, (B, n_fft, Fp)))
    at += up64(B * n_fft * Fp)
    blk = up64(B * n_mels * Fp)
    mel.append((am, am + blk, (B, n_mels, Fp)))
    am += 2 * blk
  return spec, mel, am, at, am + 64


def block(buf, offset, shape):
  return buf[offset:offset + math.prod(shape)].reshape(shape)


def written_mask(scales, B, N, lens):
  """(spectra, mels) bool masks over the floats of the two buffers: the cells f < F_b of every block, and the cell counts."""
  spec, mel, tail, ns, nm = layout(scales, B, N)
  ms, mm = torch.zeros(ns, dtype=torch.bool), torch.zeros(nm, dtype=torch.bool)
  for (n_fft, hop, win, n_mels), (at, shape), (ax, ay, mshape) in zip(scales, spec, mel):
    for b, n in enumerate(lens):
      Fb = frames_of(n, hop)
      block(ms, at, shape)[b, :, :Fb] = True
      block(mm, ax, mshape)[b, :, :Fb] = True
      block(mm, ay, mshape)[b, :, :Fb] = True
  mm[tail:tail + 16] = True                                 # fp64 [8]
  return ms, mm


# ---------------------------------------------------------------- restatements of the planes, per utterance
def rows_of(spec_fn, scale, x, lens, dtype):
  """The interleaved rows of every crop: a list of [n_fft, F_b]."""
  n_fft, hop, win, _ = scale
  return [interleave(*spec_fn(x[b:b + 1, :n], n_fft, hop, win, dtype))[0] for b, n in enumerate(lens)]


def rows_a(scale, x, lens):
  return rows_of(O.spec_stft, scale, x, lens, torch.float64)


def rows_b(scale, x, lens, dtype=torch.float32):
  return rows_of(O.spec_unfold, scale, x, lens, dtype)


def rows_c32(scale, x, lens):
  """(c): fp32, one chain per cell in the kernel's order -- pairs of taps ascending from lpad, the two products of a pair
  added to the accumulator one after the other."""
  n_fft, hop, win, _ = scale
  lpad = (n_fft - win) // 2
  fb = O._basis(n_fft, win)                                 # [2K, n_fft] fp32
  K = n_fft // 2 + 1
  bt = interleave(fb[:K], fb[K:]).t().contiguous()          # [tap, row]: the basis with its rows interleaved
  out = []
  for b, n in enumerate(lens):
    fr = O.frames_unfold(x[b:b + 1, :n], n_fft, hop, torch.float32)[0]      # [F, n_fft]
    acc = torch.zeros(fr.shape[0], n_fft)
    for k in range(lpad, lpad + win):                       # the taps behind the window meet a zero basis
      acc = acc + fr[:, k, None] * bt[k][None, :]
    out.append(acc.t())
  return out


def rows_cap(scale, x, lens):
  """The derived cap of every cell: (win + 2) 2^-24 sum_k |x_k| |basis_k| in fp64, as interleaved rows per crop."""
  n_fft, hop, win, _ = scale
  ab = O._basis(n_fft, win).double().abs()
  K = n_fft // 2 + 1
  out = []
  for b, n in enumerate(lens):
    S = O.frames_unfold(x[b:b + 1, :n], n_fft, hop, torch.float64)[0].abs() @ ab.t()      # [F, 2K]
    out.append((win + 2) * 2.0 ** -24 * interleave(S[:, :K].t(), S[:, K:].t()))
  return out


def mels_of(mag_fn, scale, W, x, lens, dtype):
  """The linear mels of every crop: a list of [n_mels, F_b]."""
  return [O.mels(mag_fn, x[b:b + 1, :n], scale, W, None, dtype) for b, n in enumerate(lens)]


def crop_planes(t, Fb):
  """A device block [B, R, Fp] -> the list of [R, F_b] in fp64 on the CPU."""
  t = t.detach().double().cpu()
  return [t[b, :, :f] for b, f in enumerate(Fb)]


# ---------------------------------------------------------------- statistics
def cell_errors(got, ref):
  """e of the module docstring for lists of planes [R, F_b]; NaN counts as infinite."""
  den = math.sqrt(sum(float(r.double().pow(2).sum()) for r in ref) / sum(r.numel() for r in ref))
  return [torch.nan_to_num((g.double() - r.double()).abs() / max(den, 1e-300), nan=float("inf")) for g, r in zip(got, ref)]


def worst_cell(errs):
  """(max e, (utterance, row, frame, frames to the nearest utterance end, frames to the nearest multiple of 64))."""
  b = max(range(len(errs)), key=lambda i: float(errs[i].max()))
  e = errs[b]
  r, f = divmod(int(e.argmax()), e.shape[1])
  return float(e[r, f]), (b, r, f, min(f, e.shape[1] - 1 - f), min(f % 64, 64 - f % 64))


def describe_cell(pos, MT=None):
  b, r, f, end, seam = pos
  s = f"utterance {b} row {r} frame {f} ({end} frames from the utterance's end, {seam} from a multiple of 64)"
  if MT is not None:
    nby = gemm_nby(MT)
    s += f", M tile {r // 32}" + (f" of workgroup {owner(r, MT, nby)} along M" if nby > 1 else "")
  return s


def cell_stat(got, ref):
  return worst_cell(cell_errors(got, ref))


def sample_errors(got, ref, lens):
  """e [B, N] of the module docstring (fp64); an utterance whose reference is all zeros asks for exact zeros (inf else)."""
  got, ref = got.detach().double().cpu(), ref.detach().double().cpu()
  e = torch.zeros_like(ref)
  for b, n in enumerate(lens):
    r = ref[b, :n]
    nz = r != 0
    d = torch.nan_to_num((got[b, :n] - r).abs(), nan=float("inf"))
    if nz.any():
      e[b, :n] = d / float(r[nz].pow(2).mean().sqrt())
    else:
      e[b, :n] = torch.where(d == 0, 0.0, float("inf"))
  return e


def worst_sample(e, lens, hop):
  """(max e, (utterance, sample, samples to the nearest utterance end, frames to the nearest multiple of 64))."""
  b, s = divmod(int(e.argmax()), e.shape[1])
  fr = s / hop
  return float(e[b, s]), (b, s, min(s, lens[b] - 1 - s), round(min(fr % 64, 64 - fr % 64), 2))


def describe_sample(pos):
  return (f"utterance {pos[0]} sample {pos[1]} ({pos[2]} samples from the utterance's end, {pos[3]} frames from a multiple "
          f"of 64)")


def sample_stat(got, ref, lens, hop):
  return worst_sample(sample_errors(got, ref, lens), lens, hop)


def l2_per_utterance(got, ref, lens):
  """Relative L2 per utterance over its samples; None where the reference is all zeros."""
  out = []
  for b, n in enumerate(lens):
    den = float(ref[b, :n].double().norm())
    out.append(float((got[b, :n].double().cpu() - ref[b, :n].double()).norm()) / den if den > 0 else None)
  return out


# ---------------------------------------------------------------- gradients of the restatements
MEL_TERMS = {"log": (1.0, 0.0), "lin": (0.0, 1.0), "both": (1.0, 1.0)}
STFT_TERMS = {"sc": (1.0, 0.0, 1e-7), "mag": (0.0, 1.0, STFT_EPS)}      # factor_sc, factor_mag, eps
# the terms a local difference runs under: the mel loss at unit factors, the STFT loss's spectral convergence (``qualifies``)
LOCAL_TERMS = (("mel", "both"), ("stft", "sc"))


def grad_a(c, loss, term, x, y, banks=None):
  """(a)'s gradient [B, N] in fp64."""
  if loss == "mel":
    fl, fn = MEL_TERMS[term]
    return O.grad_of(O.loss_stft, x, y, c.scales, banks=banks, factor_log=fl, factor_lin=fn, lengths=c.lengths)
  fs, fm, eps = STFT_TERMS[term]
  return ragged_grad64(x, y, c.lens, c.res, eps, fs, fm)


def grad_b32(c, loss, term, x, y, banks=None):
  """(b)'s gradient in fp32 under autograd."""
  if loss == "mel":
    fl, fn = MEL_TERMS[term]
    return O.grad_of(O.loss_unfold, x, y, c.scales, banks=banks, factor_log=fl, factor_lin=fn, lengths=c.lengths,
                     dtype=torch.float32)
  fs, fm, eps = STFT_TERMS[term]
  return ragged_grad64(x, y, c.lens, c.res, eps, fs, fm, fn=functools.partial(ragged_unfold, dtype=torch.float32))


# ---------------------------------------------------------------- references of draw 0 and yardsticks, cached
@functools.lru_cache(maxsize=None)
def ref_rows(name, i=0, swap=False):
  """(a)'s rows of scale i on the case's own batch (the target's with ``swap``): computed once, shared, never modified."""
  c = case(name)
  return rows_a(c.scales[i], c.plane_inputs()[1 if swap else 0], c.lens)


@functools.lru_cache(maxsize=None)
def ref_spec(name, i=0, swap=False):
  """(a)'s (re, im), each [K, F_b], per utterance."""
  c = case(name)
  n_fft, hop, win, _ = c.scales[i]
  sig = c.plane_inputs()[1 if swap else 0]
  return [tuple(t[0] for t in O.spec_stft(sig[b:b + 1, :n], n_fft, hop, win, torch.float64)) for b, n in enumerate(c.lens)]


@functools.lru_cache(maxsize=None)
def ref_mels(name, i=0, swap=False):
  c = case(name)
  return mels_of(O.mag_stft, c.scales[i], c.banks()[i], c.plane_inputs()[1 if swap else 0], c.lens, torch.float64)


@functools.lru_cache(maxsize=None)
def ref_cap(name, i=0, swap=False):
  c = case(name)
  return rows_cap(c.scales[i], c.plane_inputs()[1 if swap else 0], c.lens)


@functools.lru_cache(maxsize=None)
def ref_grad(name, loss, term, where=None):
  c = case(name)
  x, y = c.inputs() if where is None else c.local_inputs(where)
  return grad_a(c, loss, term, x, y)


@functools.lru_cache(maxsize=None)
def l2_b32(name, loss, term, where=None):
  """g32 of the existing tests: the per-utterance relative L2 error of (b) in fp32 on the case's own batch."""
  c = case(name)
  x, y = c.inputs() if where is None else c.local_inputs(where)
  return l2_per_utterance(grad_b32(c, loss, term, x, y), ref_grad(name, loss, term, where), c.lens)


@functools.lru_cache(maxsize=None)
def yard_rows(name, i=0, restatement=None):
  """Y of the transform rows of scale i: the worst cell of (b) in fp32 -- of (c) for the cases of ROWS_FROM_C -- over the
  draws, prediction and target."""
  c = case(name)
  restatement = ("c" if name in ROWS_FROM_C else "b") if restatement is None else restatement
  fn = rows_c32 if restatement == "c" else rows_b
  y = 0.0
  for d in range(len(YARD_SEEDS)):
    for sig in c.plane_inputs(d):
      y = max(y, cell_stat(fn(c.scales[i], sig, c.lens), rows_a(c.scales[i], sig, c.lens))[0])
  return y


def mag_c32(x, n_fft, hop, win, dtype):
  """The magnitudes of (c), in the form of ``O.mag_unfold``: [1, K, F] of one crop."""
  re, im = deinterleave(rows_c32((n_fft, hop, win, 0), x, [x.shape[1]])[0])
  return O._root(re ** 2 + im ** 2)[None]


@functools.lru_cache(maxsize=None)
def yard_mels(name, i=0, restatement=None):
  """Y of the linear mels of scale i under the case's bank, from (b) in fp32 or, for the cases of MELS_FROM_C, from (c)'s
  transform."""
  c = case(name)
  restatement = ("c" if name in MELS_FROM_C else "b") if restatement is None else restatement
  s, W = c.scales[i], c.banks()[i]
  fn = mag_c32 if restatement == "c" else O.mag_unfold
  return max(cell_stat(mels_of(fn, s, W, sig, c.lens, torch.float32), mels_of(O.mag_stft, s, W, sig, c.lens, torch.float64))[0]
             for d in range(len(YARD_SEEDS)) for sig in c.plane_inputs(d))


@functools.lru_cache(maxsize=None)
def yard_grad(name, loss, term, where=None):
  """Y of a gradient: the worst sample of (b) in fp32 over the draws."""
  c = case(name)
  hop = c.scales[0][1]
  y = 0.0
  for d in range(len(YARD_SEEDS)):
    xs, ys = c.inputs(d) if where is None else c.local_inputs(where, d)
    ref = ref_grad(name, loss, term, where) if d == 0 else grad_a(c, loss, term, xs, ys)
    y = max(y, sample_stat(grad_b32(c, loss, term, xs, ys), ref, c.lens, hop)[0])
  return y
