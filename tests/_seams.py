"""Per-column error bounds at utterance edges and tile seams (tests/test_seams_cpu.py, tests/test_gpu_seams.py).

Every other comparison of the flow path with its oracle is one norm over a whole tensor, in which a kernel that is wrong in
a few columns -- the first or last column of an utterance, the frames on either side of a tile seam, a dilated tap that
reads a guard row -- is diluted by all the columns that are right.  Here a quantity with a time axis is compared column by
column,

  e[b, j] = || got[b, :, j] - ref[b, :, j] ||_2 / rms over (b, j) of || ref[b, :, j] ||_2 ,

``ref`` the fp64 oracle (``_hot.exact``) on the inputs the kernel received.  The error is normalised by the tensor's RMS
column norm and not by the column's own, so a quiet column needs no floor and no column is left out.  The statistic is
the maximum over (b, j); its position is reported as (utterance, column, distance to the nearest utterance end, rows of
the polyphase plane to the nearest tile seam).  The yardstick of a quantity is the same maximum for ``_hot.emulated`` against
``_hot.exact``: the largest over the input draws ``YARD_SEEDS`` and, per draw, three dithered realisations of the fp16
roundings; the device is held to ``BOUND_FACTOR`` (3) times that.  Parameter gradients have no time
axis: they keep the whole-tensor statistic of ``_hot.check`` and are made sensitive to the edges by a cotangent that is
non-zero at the utterance ends, around column 128, around the columns whose deep taps land on the utterance's first and
last column, or on the frames at a tile seam only.

Every position is a row of the case's own geometry: the guard frames of a case are ``_envelope.guard_frames(n_layers)``
(4 up to 8 layers, 8 and 16 at 9 and 10), which tests/test_envelope_cpu.py pins to the library.

The weights are the ordinary synthetic ones; the yardsticks are computed when a test asks for them and cached.
"""
import functools

import torch

import _hot as H
import _corners as K
from _cases import oracle_cfg_from_hp
from _envelope import guard_frames
from waveglow_amd import synthetic
from waveglow_amd.hparams import HParams

YARD_SEEDS = H.YARD_SEEDS
BOUND_FACTOR = H.BOUND_FACTOR
REALISATIONS = 3                # dithered realisations of the roundings per input draw
COL128 = 128                    # the column whose two sides the "col128" cotangent covers
REACH_MIN = 64                  # the "reach" cotangent covers the taps of every dilation from here up
GUARD8 = guard_frames(8)        # guard frames on each side of an utterance up to 8 layers; a case has its own (Seam.guard)

# The planes are polyphase: flow column t of utterance b lies in phase block t % 32 at row
# b (F + 2 Gf) + Gf + t // 32, F = T frames, Gf = _envelope.guard_frames(n_layers) guard frames (4 up to 8 layers, 8 / 16 at
# 9 / 10: wg_host.h make_geom), and a tile of the WN layer kernel (64 or 128 wide) or of the plane GEMM
# (32 ct wide) is that many consecutive ROWS of one phase block.  A tile seam therefore lies between two frames, at a row
# that is a multiple of 64 or 128, and not at a flow column that is one.
# id: (HParams overrides, B, T, weight seed).
#   seam_c64, seam_c256: 288 columns, 34 / 17 rows per phase block: ONE tile.  They pin the utterance ends and the dilated
#     taps (up to 128, inside the utterance on both sides) that reach guard rows; no tile seam.  seam_c64 splits an early
#     output off at flow 1, so that the synthesis direction has a z_early.
#   tile64_*: B 4 x T 10, 18 rows per utterance: row 64 is frame 6 of utterance 3 (the seam of the 64-wide tiles lies
#     between its frames 5 and 6; one 128-wide tile).
#   tile128_*: B 8 x T 9, 17 rows per utterance: row 128 is frame 5 of utterance 7 (a seam of both tile widths); row 64
#     is the first guard row behind utterance 3, whose last frame is the last row of a 64-wide tile.
CASES = {
  "seam_c64": (dict(n_channels=64, n_layers=8, n_flows=2, n_early_every=1), 2, 9, 51),
  "seam_c256": (dict(n_channels=256, n_layers=8, n_flows=1, n_early_every=4), 1, 9, 52),
  "tile64_c64": (dict(n_channels=64, n_layers=8, n_flows=2, n_early_every=1), 4, 10, 53),
  "tile128_c64": (dict(n_channels=64, n_layers=8, n_flows=2, n_early_every=1), 8, 9, 54),
  "tile64_c256": (dict(n_channels=256, n_layers=8, n_flows=1, n_early_every=4), 4, 10, 55),
  "tile128_c256": (dict(n_channels=256, n_layers=8, n_flows=1, n_early_every=4), 8, 9, 56),
  # 9 and 10 layers: dilations 256 and 512, 8 and 16 guard frames.  A tap of dilation 512 lands 16 rows away, the whole of
  # the slack in front of and behind a plane (kRowPad).
  #   seam_l10_*, seam_l9_c128: B 1 x T 18, 576 columns, 50 / 34 rows: ONE tile; the taps of dilation 256 and 512 have real
  #     columns on both sides (column 512 reads column 0, column 63 reads column 575) and reach guard rows everywhere else.
  #   seam_c128, seam_c512: the other two channel counts of the kernels at the 8-layer edge shape (288 columns).
  #   tile_l10_*: B 2 x T 52, Fp = 84: row 64 is frame 48 of utterance 0 (rows 16 .. 67), row 128 frame 28 of utterance 1
  #     (rows 100 .. 151).  The 16-row taps of the frames at both seams read frames of the same utterance.
  #   first64_*: 8 layers, B 4 x T 12, Fp = 20: row 64 is frame 0 of utterance 3; rows 60 .. 63, the last of the 64-wide tile
  #     in front of it, are that utterance's leading guard rows, and row 55 is the last frame of utterance 2.
  "seam_l10_c64": (dict(n_channels=64, n_layers=10, n_flows=2, n_early_every=1), 1, 18, 61),
  "seam_l10_c256": (dict(n_channels=256, n_layers=10, n_flows=1, n_early_every=4), 1, 18, 62),
  "seam_l9_c128": (dict(n_channels=128, n_layers=9, n_flows=2, n_early_every=1, n_early_size=2), 1, 18, 63),
  "seam_c128": (dict(n_channels=128, n_layers=8, n_flows=2, n_early_every=1), 2, 9, 64),
  "seam_c512": (dict(n_channels=512, n_layers=8, n_flows=1, n_early_every=4), 1, 9, 65),
  "tile_l10_c64": (dict(n_channels=64, n_layers=10, n_flows=2, n_early_every=1), 2, 52, 66),
  "tile_l10_c256": (dict(n_channels=256, n_layers=10, n_flows=1, n_early_every=4), 2, 52, 67),
  "first64_c64": (dict(n_channels=64, n_layers=8, n_flows=2, n_early_every=1), 4, 12, 68),
  "first64_c256": (dict(n_channels=256, n_layers=8, n_flows=1, n_early_every=4), 4, 12, 69),
}
IDS = ["seam_c64", "seam_c256"]                       # the edge cases up to dilation 128: "edge" and "col128" cotangents
DEEP_IDS = ["seam_l10_c64", "seam_l10_c256", "seam_l9_c128"]      # edge cases with dilations 256 / 512: "edge" and "reach"
WIDE_IDS = ["seam_c128", "seam_c512"]                 # the other channel counts at the 8-layer edge shape: "edge" and "reach"
EDGE_IDS = IDS + DEEP_IDS + WIDE_IDS
# the cases with a tile seam inside an utterance, and the seam on an utterance's first frame ("first" cotangent)
TILE_IDS = [n for n in CASES if n.startswith("tile")]
FIRST_IDS = ["first64_c64", "first64_c256"]
# (row, utterance, frame) of every seam of a case that has frames of one utterance on both sides
TILE_SEAM = {"tile64_c64": [(64, 3, 6)], "tile64_c256": [(64, 3, 6)], "tile128_c64": [(128, 7, 5)], "tile128_c256": [(128, 7, 5)],
             "tile_l10_c64": [(64, 0, 48), (128, 1, 28)], "tile_l10_c256": [(64, 0, 48), (128, 1, 28)]}
FIRST_SEAM = {"first64_c64": (64, 3), "first64_c256": (64, 3)}      # (row, utterance whose frame 0 it is)


def tile_widths(n_channels):
  """The values of WG_FORCE_BN that select a tile width of their own at that channel count (kernels.hip: WnCfg<C>::BN is 64
  from 512 channels up, so there 128 is ignored and one run covers the case)."""
  return ["64"] if n_channels >= 512 else ["128", "64"]


def cotangents(name):
  """The local cotangents a case runs under."""
  if name in IDS:
    return ["edge", "col128"]
  if name in DEEP_IDS or name in WIDE_IDS:
    return ["edge", "reach"]
  return ["first"] if name in FIRST_IDS else ["seam"]


def plane_row(b, col, n_frames, guard=GUARD8):
  """The row of flow column ``col`` of utterance ``b`` in its phase block, ``guard`` guard frames on each side of an utterance."""
  return b * (n_frames + 2 * guard) + guard + col // 32


# ---------------------------------------------------------------- columns
def columns(q, t, n_group=8):
  """The tensor of quantity ``q`` as [B, J, n] (fp64, CPU): J columns of n entries, or None when ``q`` has no time axis.
  audio, d audio: the 8 samples of squeezed column j (samples behind the last whole column, which the unfold drops, are
  not part of any column); d mel: the channels of frame j; everything else with three axes: the channel axis."""
  t = t.detach().double().cpu()
  if q in ("audio", "d audio"):
    J = t.size(1) // n_group
    return t[:, :J * n_group].reshape(t.size(0), J, n_group)
  if q == "d mel" or q == "z" or q.startswith(("log_s.", "d z_")):
    return t.permute(0, 2, 1)
  return None


def stride(q):
  """Flow columns per column of ``q``: a mel frame spans 32 of them."""
  return 32 if q == "d mel" else 1


def col_error(q, got, ref):
  """e [B, J] of the module docstring."""
  g, r = columns(q, got), columns(q, ref)
  assert g.shape == r.shape, f"{q}: shape {tuple(g.shape)} vs {tuple(r.shape)}"
  den = float(r.norm(dim=2).pow(2).mean().sqrt())
  return (g - r).norm(dim=2) / max(den, 1e-300)


def worst(q, got, ref, guard=GUARD8):
  """(max e, (utterance, column, distance to the nearest utterance end, rows to the nearest tile seam)); column and the
  first distance in flow columns (a mel frame counts from its first column); the second is 0 for the two rows of a phase
  block on either side of a multiple of 64 (plane_row), 1 for their neighbours, up to 31."""
  e = col_error(q, got, ref)
  e = torch.nan_to_num(e, nan=float("inf"))
  b, j = divmod(int(e.argmax()), e.size(1))
  s = stride(q)
  col, last = j * s, (e.size(1) - 1) * s
  row = plane_row(b, col, (e.size(1) * s + 31) // 32, guard)
  return float(e[b, j]), (b, col, min(col, last - col), min(row % 64, 63 - row % 64))


# ---------------------------------------------------------------- cases, inputs, cotangents
class Seam:
  """A case and direction at the ordinary synthetic weights: hp, cfg, sd (dense), sdn (weight-norm form), inputs."""

  def __init__(self, name, direction, shape=None):
    over, self.B, self.T, self.wseed = CASES[name] if shape is None else shape
    self.name, self.direction = name, direction
    self.hp = HParams(**over)
    self.guard = guard_frames(self.hp.n_layers)      # tests/test_envelope_cpu.py pins it to the library
    self.cfg = oracle_cfg_from_hp(self.hp)
    self.sd = synthetic.make_state_dict(self.hp, seed=self.wseed)
    self.sdn = synthetic.to_weightnorm_form(self.sd)
    self.L = 32 * self.T
    self.sigma = H.SIGMA
    self.inputs = self.draw(0)
    self.mel = self.inputs[0]
    if direction == "fwd":
      self.wav = self.inputs[1]
    else:
      self.z_init, self.z_early = self.inputs[1], self.inputs[2]

  def draw(self, d):
    return H.make_inputs_at(self.hp, self.B, self.T, self.direction, d, crop=0)

  def cotangent(self, where):
    """None ("loss" / "values"), or a cotangent that is non-zero only at the "edge" (the first and the last 32 columns of
    every utterance), on the 32 columns on each side of column 128 ("col128": interior columns, no tile seam) or, for a
    tile case, on the two frames on either side of its tile seam ("seam": 64 columns of one utterance, and at 10 layers the
    frames ``seam_frames`` adds), on the 32 columns on each side of every column of ``reach_columns`` ("reach": the deep
    taps that land on the utterance's first and last column, which "edge" leaves without a cotangent), or on frames 0 and 1
    of the utterance whose first frame is row 64 and the last frame of the one in front of it ("first"): on z [B, 8, L] for
    "fwd", on the audio [B, 8 L] for "inv".  Scaled as the mean loss scales its own (1 / number of samples), so that the
    automatic loss scale of the gradient planes fits."""
    if where in (None, "loss", "values"):
      return None
    keep = torch.zeros(self.B, self.L)
    if where == "edge":
      keep[:, :32] = 1.0
      keep[:, -32:] = 1.0
    elif where == "col128":
      keep[:, COL128 - 32:COL128 + 32] = 1.0
    elif where == "reach":
      for c in self.reach_columns():
        keep[:, max(c - 32, 0):c + 32] = 1.0
    elif where == "first":
      row, b = self.first_seam()
      keep[b, :64] = 1.0
      keep[b - 1, -32:] = 1.0
    else:
      assert where == "seam"
      for f in self.seam_frames():
        keep[f[0], 32 * f[1]:32 * (f[1] + 1)] = 1.0
    g = torch.Generator().manual_seed(11)
    n = self.B * 8 * self.L
    if self.direction == "fwd":
      return torch.randn(self.B, 8, self.L, generator=g) * keep[:, None, :] / n
    return torch.randn(self.B, self.L, 8, generator=g).mul(keep[:, :, None]).reshape(self.B, 8 * self.L) / n

  def reach_columns(self):
    """Columns ``d`` and ``L - 1 - d`` for every dilation d >= REACH_MIN of the model: the columns whose outer taps land on
    the utterance's first and last column."""
    ds = [2 ** i for i in range(self.hp.n_layers) if REACH_MIN <= 2 ** i < self.L]
    return sorted({c for d in ds for c in (d, self.L - 1 - d)})

  def tile_seams(self):
    """[(row, utterance, frame)]: the rows of the phase blocks that are a multiple of 64 and hold a frame with a frame of
    the same utterance in front of them (a seam of the 64-wide tiles; of the 128-wide too when row % 128 == 0)."""
    seams = TILE_SEAM[self.name]
    for row, b, f in seams:
      assert plane_row(b, 32 * f, self.T, self.guard) == row and row % 64 == 0 and 1 <= f < self.T and b < self.B
    return seams

  def tile_seam(self):
    """The first of ``tile_seams``."""
    return self.tile_seams()[0]

  def seam_frames(self):
    """[(utterance, frame)] of the "seam" cotangent: the two frames on either side of every seam and, where the model has a
    tap of 16 rows (dilation 512), the frames of the same utterance that those taps read ACROSS the seam: frame f - 16 (the
    left tap of frame f, behind the seam) and frame f - 1 + 16 (the right tap of frame f - 1, in front of it)."""
    out = []
    for row, b, f in self.tile_seams():
      out += [(b, f - 1), (b, f)]
      if self.hp.n_layers == 10:
        out += [(b, g) for g in (f - 16, f - 1 + 16) if 0 <= g < self.T]
    return sorted(set(out))

  def first_seam(self):
    """(row, utterance): a multiple of 64 that is the row of frame 0 of an utterance with another one in front of it."""
    row, b = FIRST_SEAM[self.name]
    assert plane_row(b, 0, self.T, self.guard) == row and row % 64 == 0 and 1 <= b < self.B
    assert plane_row(b - 1, self.L - 1, self.T, self.guard) == row - 2 * self.guard - 1
    return row, b

  def grad_scale(self):
    """The loss scale of the fp16 gradient planes that ``_hot.emulated`` uses: the automatic one."""
    return H.grad_scale(self.B * 8 * self.L)


def round16(inputs):
  rnd = lambda t: t.half().float()     # noqa: E731
  return rnd(inputs[0]), rnd(inputs[1]), {k: rnd(v) for k, v in inputs[2].items()}


def run(c, normed, where, inputs=None, fault=None, emulate=False, dither=None):
  """The oracle (or the emulation) of a case: the training step ("fwd": loss backward, or the backward of sum(z u)) or
  synthesis ("inv": values only for ``where`` = "values", else the backward of sum(audio r))."""
  sd = c.sdn if normed else c.sd
  inputs = c.inputs if inputs is None else inputs
  cot = c.cotangent(where)
  kw = dict(u=cot) if c.direction == "fwd" else dict(r=cot)
  if emulate:
    return H.emulated(c.direction, sd, inputs, c.cfg, fault=fault, dither=dither, **kw)
  return H.exact(c.direction, sd, inputs, c.cfg, fault=fault, **kw)


# ---------------------------------------------------------------- yardstick and bound
@functools.lru_cache(maxsize=None)
def _case(name, direction):
  return Seam(name, direction)


@functools.lru_cache(maxsize=None)
def oracle(name, direction, normed, where, io16=False):
  """The fp64 oracle on the case's own batch (draw 0), computed once, shared, never modified."""
  c = _case(name, direction)
  return run(c, normed, where, round16(c.inputs) if io16 else None)


def measure(c, normed, where, seeds=YARD_SEEDS, realisations=REALISATIONS, dither_seed=0, oracle0=None):
  """{quantity: statistic} of the emulation against the fp64 oracle, the largest over ``seeds`` x ``realisations``
  (dithered; generator seeded with ``dither_seed``): the worst column for a quantity with a time axis, the relative L2
  error of the whole tensor for every other one (log_det and the loss, which no column fault moves alone, are left to
  their own tests)."""
  gen = torch.Generator().manual_seed(dither_seed)
  out = {}
  for d in seeds:
    inputs = c.inputs if d == 0 else c.draw(d)
    ref = oracle0 if (d == 0 and oracle0 is not None) else run(c, normed, where, inputs)
    for _ in range(realisations):
      got = run(c, normed, where, inputs, emulate=True, dither=gen)
      for q, v in statistics(got, ref).items():
        out[q] = max(out.get(q, 0.0), v)
  return out


def statistics(got, ref):
  out = {}
  for q, t in ref.items():
    if q in ("log_det", "loss"):
      continue
    if columns(q, t) is not None:
      out[q] = worst(q, got[q], t)[0]
    else:
      g = torch.nan_to_num(got[q].detach().double().cpu(), nan=float("inf"))
      out[q] = float((g - t.double()).norm()) / max(float(t.double().norm()), 1e-300)
  return out


@functools.lru_cache(maxsize=None)
def yardstick(name, direction, normed, where):
  c = _case(name, direction)
  return measure(c, normed, where, oracle0=oracle(name, direction, normed, where))


def check(got, ref, yard, what, factor=BOUND_FACTOR, quiet=False, only=None, case=None):
  """Every quantity of ``ref`` (but log_det and the loss) against ``got``: per column where it has a time axis, else
  whole-tensor (||got - ref|| <= factor * yardstick * ||ref||, with no absolute floor: under the 1 / n-scaled local
  cotangents a floor of 1e-7 would be most of the bound of the small tensors; a reference that is exactly zero asks for
  exactly zero).  Prints the device's figure, the yardstick
  and their ratio per quantity, for the column quantities with the position of the worst column; returns the misses as
  (ratio to the yardstick, quantity, position or None), worst first.  ``case``: the Seam whose guard frames place the rows
  (8-layer geometry without one) and whose structurally zero parameter gradients (tests/_corners.py) are left out, as that
  module leaves them out."""
  rows = []
  guard = GUARD8 if case is None else case.guard
  for q, t in ref.items():
    if q in ("log_det", "loss") or (only is not None and not only(q)):
      continue
    if case is not None and q.startswith("p/") and K.structurally_zero(case.hp, q[2:]):
      continue
    g = got[q]
    assert g is not None, f"{what}: {q}: missing"
    g = g.detach().double().cpu()
    assert g.shape == t.shape, f"{what}: {q}: shape {tuple(g.shape)} vs {tuple(t.shape)}"
    y = yard[q]
    if columns(q, t) is not None:
      e, pos = worst(q, g, t, guard)
      ok = e <= factor * y
      rows.append((e / max(y, 1e-300), q, e, y, pos, ok))
    else:
      g = torch.nan_to_num(g, nan=float("inf"))
      err, den = float((g - t.double()).norm()), float(t.double().norm())
      ok = err <= factor * y * den
      rel = err / max(den, 1e-30)
      rows.append((rel / max(y, 1e-30), q, rel, y, None, ok))
  rows.sort(key=lambda r: r[0], reverse=True)
  if not quiet:
    cols = [r for r in rows if r[4] is not None]
    rest = [r for r in rows if r[4] is None]
    for ratio, q, e, y, pos, ok in cols + rest[:6]:
      where = "" if pos is None else (f" at utterance {pos[0]} column {pos[1]} ({pos[2]} from the utterance's end, "
                                      f"{pos[3]} rows from a tile seam)")
      kind = "worst column" if pos is not None else "rel"
      print(f"{what}: {q}: {kind} {e:.3e} yardstick {y:.3e} ratio {ratio:.2f}{where}{'' if ok else '  <-- MISS'}")
    if rest:
      print(f"{what}: {len(rest)} whole-tensor quantities, worst ratio {rest[0][0]:.2f} ({rest[0][1]})")
  return [(ratio, q, pos) for ratio, q, e, y, pos, ok in rows if not ok]
