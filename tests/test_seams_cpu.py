"""CPU: the per-column bounds of tests/_seams.py -- the gap they close, on record.

Faults planted in the emulation (``_hot.Prec``): an in-layer input that loses the utterance's last column, a left tap that
is lost at column ``d``, a left tap that reads one column off at one column (a tile that stages its halo wrongly), and a
weight gradient that omits the last column's term.  For each:

(a) at a shape the existing GPU tests run, the emulation WITH the fault is inside every whole-tensor bound of the suite
    (``_inside_cold_bounds`` of test_hot_cpu.py: RMS_TOL, FWD_TOL, the loss bound, GRAD_TOL);
(b) at the seam cases of tests/test_gpu_seams.py at least one quantity is beyond 2 x the per-column bound (for the
    weight-gradient fault: one parameter gradient beyond 2 x its whole-tensor yardstick bound under the edge cotangent);
(c) three further dithered realisations of the fault-free emulation stay inside the per-column bound.

The planes are polyphase, so a tile seam of the kernels lies between two FRAMES (rows 63 | 64 or 127 | 128 of a phase
block), not at a flow column that is a multiple of 64: (b) and (c) are shown once more at a case that has such a seam
inside an utterance, with the fault on the first column behind it and the cotangent on the two frames around it.

9 and 10 layers (dilations 256 and 512, 8 and 16 guard frames): the geometry of every such case is asserted row by row,
and (b) and (c) are shown at seam_l10_c64 for the layers of dilation 256 and 512 under the training loss / the values and
under the "reach" cotangent -- under "edge" a lost tap of column 512 leaves every gradient exact, because that column
carries no cotangent (test_deep_taps_need_the_reach_cotangent).
"""
import pytest
import torch

import _hot as H
import _seams as S
from test_hot_cpu import _inside_cold_bounds

# (a): shapes of test_gpu_parity.test_infer_ragged_lengths_vs_oracle (synthesis) and
# test_gpu_train.test_train_step_every_tile_width (training), at their weight seeds.  The model, B, T and the weights are
# those tests'; the batch is not: the inputs are drawn as _hot.make_inputs draws them (another mel seed, replayed noise at
# sigma 0.7, a waveform with loud and quiet stretches and no crop where the GPU test crops 72 samples).
SYNTH = (dict(n_channels=64, n_layers=8, n_flows=4, n_early_every=2), 2, 33, 11)
TRAIN = (dict(n_channels=64, n_layers=3, n_flows=4, n_early_every=2), 6, 50, 11)
# fault: (direction, shape) at which it is inside every existing bound.  Where the other placements of the same fault sit:
# of eight placements of drop_col / drop_tap / seam in flows 0, 1 and 3, four are inside the synthesis bound on the audio
# (the others at 1.10 ... 1.13 of it) and five inside the training bounds at TRAIN (the others at 1.07 ... 1.39 x GRAD_TOL
# on d audio), measured with the emulation.
INVISIBLE = {
  ("drop_col", 3, 0): [("inv", SYNTH), ("fwd", TRAIN)],
  ("drop_tap", 0, 7): [("inv", SYNTH)],
  ("drop_tap", 3, 0): [("fwd", TRAIN)],
  ("seam", 0, 2, 64): [("inv", SYNTH)],
  ("seam", 3, 0, 128): [("fwd", TRAIN)],
  # through synthesis at SYNTH, under a full random cotangent, the fault is at 3.7 ... 4.3 x GRAD_TOL: (a) holds in the
  # training direction only
  ("wgrad_last", 3, 0): [("fwd", TRAIN)],
}
# (b): the same kinds of fault inside the seam cases (two flows / one flow)
VISIBLE = {
  "seam_c64": [("drop_col", 1, 0), ("drop_col", 0, 3), ("drop_tap", 1, 0), ("drop_tap", 0, 7), ("seam", 1, 0, 128),
               ("seam", 0, 2, 64), ("seam", 1, 7, 256), ("wgrad_last", 1, 0), ("wgrad_last", 0, 3)],
  "seam_c256": [("drop_col", 0, 0), ("drop_col", 0, 3), ("drop_tap", 0, 0), ("drop_tap", 0, 7), ("seam", 0, 0, 128),
                ("seam", 0, 2, 64), ("wgrad_last", 0, 0), ("wgrad_last", 0, 3)],
}


def test_columns_and_positions():
  """The column axis of every kind of quantity, and where the arg-max is reported."""
  ref = {"audio": torch.zeros(2, 8 * 288 + 5), "z": torch.zeros(2, 8, 288), "log_s.0": torch.zeros(2, 4, 288),
         "d mel": torch.zeros(2, 80, 9), "d z_early.0": torch.zeros(2, 2, 288), "d z_init": torch.zeros(2, 6, 288),
         "d audio": torch.zeros(2, 8 * 288), "p/x.weight": torch.zeros(4, 4, 3), "loss": torch.zeros(1)}
  shapes = {q: (None if S.columns(q, t) is None else tuple(S.columns(q, t).shape)) for q, t in ref.items()}
  assert shapes == {"audio": (2, 288, 8), "z": (2, 288, 8), "log_s.0": (2, 288, 4), "d mel": (2, 9, 80),
                    "d z_early.0": (2, 288, 2), "d z_init": (2, 288, 6), "d audio": (2, 288, 8), "p/x.weight": None,
                    "loss": None}
  r = torch.ones(2, 8, 288)
  g = r.clone()
  g[1, 3, 287] += 0.5                                 # the last column of utterance 1
  e, pos = S.worst("z", g, r)
  assert pos == (1, 287, 0, 29) and abs(e - 0.5 / 8 ** 0.5) < 1e-12      # row 17 + 4 + 8 = 29 of its phase block
  g = torch.ones(2, 8 * 288)
  g[0, 8 * 130 + 7] = 3.0                             # column 130: frame 4, row 8
  assert S.worst("audio", g, torch.ones(2, 8 * 288))[1] == (0, 130, 130, 8)
  g = torch.ones(2, 80, 9)
  g[0, 5, 4] = 2.0                                    # frame 4 = columns 128 ... 159
  assert S.worst("d mel", g, torch.ones(2, 80, 9))[1] == (0, 128, 128, 8)
  # B 4 x T 10: 18 rows per utterance; frames 5 | 6 of utterance 3 are rows 63 | 64, both "0 rows from a tile seam"
  assert [S.plane_row(3, 32 * f, 10) for f in (5, 6)] == [63, 64]
  for col, dist in ((32 * 5 + 31, 0), (32 * 6, 0), (32 * 7, 1), (32 * 4, 1)):
    g = torch.ones(4, 8, 320)
    g[3, 0, col] = 2.0
    assert S.worst("z", g, torch.ones(4, 8, 320))[1][3] == dist
  # a quiet column is not left out, and is measured against the tensor's rms column norm
  r = torch.ones(1, 8, 288)
  r[0, :, 100] = 0.0
  g = r.clone()
  g[0, 0, 100] = 0.1
  e, pos = S.worst("z", g, r)
  assert pos[1] == 100 and abs(e - 0.1 / (8 * 287 / 288) ** 0.5) < 1e-8        # 0.1 is an fp32 value here


def test_cotangents_are_edge_local():
  for name in S.IDS:
    for d in H.DIRECTIONS:
      c = S._case(name, d)
      for where, cols in (("edge", list(range(32)) + list(range(c.L - 32, c.L))), ("col128", list(range(96, 160)))):
        u = c.cotangent(where)
        per_col = S.columns("z" if d == "fwd" else "audio", u).abs().amax(dim=(0, 2))
        assert sorted(torch.nonzero(per_col).flatten().tolist()) == cols
    assert c.L == 288 and 2 ** (c.hp.n_layers - 1) < c.L
    assert c.guard == 4 and c.B * (c.T + 2 * c.guard) <= 64              # one tile: these cases have no tile seam
  for name in S.TILE_IDS:
    for d in H.DIRECTIONS:
      c = S.Seam(name, d)
      per = S.columns("z" if d == "fwd" else "audio", c.cotangent("seam")).abs().amax(dim=2)
      assert torch.nonzero(per).tolist() == [[b, j] for b, f in c.seam_frames() for j in range(32 * f, 32 * (f + 1))]
      if c.hp.n_layers <= 8:
        row, b, f = c.tile_seam()
        assert c.seam_frames() == [(b, f - 1), (b, f)] and row in (64, 128) and 128 >= 2 ** (c.hp.n_layers - 1)


@pytest.mark.parametrize("fault", list(INVISIBLE), ids=lambda f: "-".join(str(v) for v in f))
def test_planted_fault_is_inside_every_whole_tensor_bound(fault):
  for direction, shape in INVISIBLE[fault]:
    c = S.Seam("existing", direction, shape=shape)
    normed = direction == "fwd"                                        # the training tests take the weight-norm form
    ref = S.run(c, normed, "loss" if direction == "fwd" else "values")
    got = S.run(c, normed, "loss" if direction == "fwd" else "values", fault=fault, emulate=True)
    e = H.errors(got, ref)
    _inside_cold_bounds(e, ref)
    stats = S.statistics(got, ref)
    print(f"{fault} {direction} at B {c.B} x T {c.T}: inside every whole-tensor bound; worst relative error "
          f"{max(err / max(den, 1e-30) for err, den in e.values()):.2e}; worst columns "
          f"{ {q: f'{v:.1e}' for q, v in stats.items() if not q.startswith('p/')} }")


@pytest.mark.parametrize("name", S.IDS)
@pytest.mark.parametrize("direction", H.DIRECTIONS)
def test_planted_faults_exceed_the_per_column_bound(name, direction):
  """(b) and (c) under the edge cotangent, which carries every quantity of a direction: values, data gradients per column,
  parameter gradients whole-tensor."""
  c = S._case(name, direction)
  ref = S.oracle(name, direction, True, "edge")
  yard = S.yardstick(name, direction, True, "edge")
  print(f"{name}/{direction} yardsticks:", {q: f"{v:.2e}" for q, v in yard.items() if not q.startswith("p/")},
        "parameter gradients at most", f"{max(v for q, v in yard.items() if q.startswith('p/')):.2e}")
  assert all(v > 0 for q, v in yard.items() if S.columns(q, ref[q]) is not None)
  for fault in VISIBLE[name]:
    got = S.run(c, True, "edge", fault=fault, emulate=True)
    miss = S.check(got, ref, yard, f"{fault} {name}/{direction}", factor=2.0 * S.BOUND_FACTOR, quiet=True)
    cols = [(round(r, 1), q, pos) for r, q, pos in miss if pos is not None]
    par = [(round(r, 1), q) for r, q, pos in miss if pos is None]
    print(f"{fault} {name}/{direction}: beyond 2 x the bound: columns {cols}; {len(par)} parameter gradients, worst {par[:1]}")
    if fault[0] == "wgrad_last":
      assert not cols                                                  # values and data gradients stay exact
      key = f"p/WN.{fault[1]}.in_layers.{fault[2]}."
      assert par and all(q.startswith(key) for _, q in par), par
    else:
      assert cols, f"{fault}: no column of {name}/{direction} exceeds twice the per-column bound"
  gen = torch.Generator().manual_seed(1000)
  for rep in range(3):
    got = S.run(c, True, "edge", emulate=True, dither=gen)
    miss = S.check(got, ref, yard, f"{name}/{direction} realisation {rep}", quiet=True)
    print(f"{name}/{direction} fault-free realisation {rep}: worst ratio to the yardstick "
          f"{max(v / yard[q] for q, v in S.statistics(got, ref).items() if yard[q] > 0):.2f}")
    assert not miss, miss[:4]


def test_fault_position_is_reported():
  """drop_col: the worst column is one of the utterance's last; seam: the column of the seam itself."""
  c = S._case("seam_c64", "inv")
  ref = S.oracle("seam_c64", "inv", False, "values")
  got = S.run(c, False, "values", fault=("drop_col", 1, 0), emulate=True)
  e, pos = S.worst("audio", got["audio"], ref["audio"])
  assert pos[2] <= 1, pos
  got = S.run(c, False, "values", fault=("seam", 1, 0, 128), emulate=True)
  assert S.worst("audio", got["audio"], ref["audio"])[1][1:3] == (128, 128)


@pytest.mark.parametrize("direction", H.DIRECTIONS)
def test_fault_at_a_tile_seam_exceeds_the_bound(direction):
  """(b) and (c) where the kernels really have a seam: tile64_c64, rows 63 | 64 = frames 5 | 6 of utterance 3.  The left
  tap of the first column of frame 6 reads one column off (at dilation 1 and 32 it reaches over the seam into frame 5)."""
  name = "tile64_c64"
  c = S._case(name, direction)
  row, b, f = c.tile_seam()
  ref = S.oracle(name, direction, True, "seam")
  yard = S.yardstick(name, direction, True, "seam")
  for fault in (("seam", 1, 0, 32 * f), ("seam", 0, 5, 32 * f)):
    got = S.run(c, True, "seam", fault=fault, emulate=True)
    miss = S.check(got, ref, yard, f"{fault} {name}/{direction}", factor=2.0 * S.BOUND_FACTOR, quiet=True)
    cols = [(round(r, 1), q, pos) for r, q, pos in miss if pos is not None]
    print(f"{fault} {name}/{direction}: beyond 2 x the bound: columns {cols}; "
          f"{sum(pos is None for _, _, pos in miss)} parameter gradients")
    assert cols and any(pos[3] == 0 for _, _, pos in cols), cols
  gen = torch.Generator().manual_seed(1000)
  for rep in range(3):
    miss = S.check(S.run(c, True, "seam", emulate=True, dither=gen), ref, yard, f"{name}/{direction} realisation {rep}", quiet=True)
    assert not miss, miss[:4]


# ---------------------------------------------------------------- 9 and 10 layers, 128 and 512 channels, a seam on frame 0
# (b) at seam_l10_c64: every kind of fault in the layer of dilation 512 of flow 1 and of dilation 256 of flow 0.  Columns
# 540 and 300 are ordinary interior columns behind column d, so the shifted left tap reads real columns.
DEEP = "seam_l10_c64"
DEEP_FAULTS = [("drop_col", 1, 9), ("drop_col", 0, 8), ("drop_tap", 1, 9), ("drop_tap", 0, 8), ("seam", 1, 9, 540),
               ("seam", 0, 8, 300), ("wgrad_last", 1, 9), ("wgrad_last", 0, 8)]
WHOLE_TENSOR = "RMS_TOL 1e-3 (audio), FWD_TOL 2e-3 (z, log_s), GRAD_TOL 5e-3 (gradients)"


def _rows(c, b, frames):
  return [S.plane_row(b, 32 * f, c.T, c.guard) for f in frames]


def test_geometry_of_the_deep_wide_and_first_frame_cases():
  """Where every row of interest of the new cases falls, by plane_row at the guard of the case."""
  from _envelope import ROW_PAD, geom
  for name in S.DEEP_IDS:
    c = S._case(name, "fwd")
    d = 2 ** (c.hp.n_layers - 1)
    assert (c.B, c.L) == (1, 576) and c.guard == {9: 8, 10: 16}[c.hp.n_layers] and c.guard * 32 >= d
    assert geom(c.B, c.T, c.hp.n_layers).Fp == c.T + 2 * c.guard <= 64          # 34 / 50 rows: one tile, no tile seam
    # the deepest tap has real columns on both sides: column d reads column 0, column L - 1 - d reads column L - 1 ...
    assert 0 < c.L - 1 - d and d < c.L
    assert S.plane_row(0, d, c.T, c.guard) - S.plane_row(0, 0, c.T, c.guard) == d // 32
    assert S.plane_row(0, 0, c.T, c.guard) == c.guard and S.plane_row(0, c.L - 1, c.T, c.guard) == c.guard + c.T - 1
    # ... and everywhere else it reads the case's own guard rows: never a row in front of the plane's first
    assert S.plane_row(0, 0, c.T, c.guard) - d // 32 >= 0 and S.plane_row(0, c.L - 1, c.T, c.guard) + d // 32 < c.T + 2 * c.guard
    assert c.reach_columns() == sorted({x for dd in (64, 128, 256, 512) if dd <= d for x in (dd, c.L - 1 - dd)})
  assert 512 // 32 == ROW_PAD                       # a tap of dilation 512 lands exactly kRowPad rows away
  for name in S.WIDE_IDS:
    c = S._case(name, "fwd")
    assert c.hp.n_layers == 8 and c.guard == 4 and c.L == 288 and c.B * (c.T + 2 * c.guard) <= 64
    assert c.reach_columns() == [64, 128, 159, 223]
  for name in ("tile_l10_c64", "tile_l10_c256"):
    c = S._case(name, "fwd")
    assert c.guard == 16 and geom(c.B, c.T, 10).Fp == 84 and c.tile_seams() == [(64, 0, 48), (128, 1, 28)]
    assert _rows(c, 0, (0, 32, 47, 48, 51)) == [16, 48, 63, 64, 67]       # the left tap of row 64 reads frame 32
    assert _rows(c, 1, (0, 12, 27, 28, 43, 51)) == [100, 112, 127, 128, 143, 151]
    assert c.seam_frames() == [(0, 32), (0, 47), (0, 48), (1, 12), (1, 27), (1, 28), (1, 43)]
    for b, f in c.seam_frames():
      assert 0 <= f < c.T                            # every frame of the cotangent is a real one of the same utterance
  for name in S.FIRST_IDS:
    c = S._case(name, "fwd")
    row, b = c.first_seam()
    assert (row, b, c.guard) == (64, 3, 4) and geom(c.B, c.T, 8).Fp == 20
    assert _rows(c, 3, (0, 1)) == [64, 65] and _rows(c, 2, (11,)) == [55]   # rows 56 .. 63: guard rows of both utterances
    for d in H.DIRECTIONS:
      per = S.columns("z" if d == "fwd" else "audio", S._case(name, d).cotangent("first")).abs().amax(dim=2)
      assert torch.nonzero(per).tolist() == [[2, j] for j in range(352, 384)] + [[3, j] for j in range(64)]
  # positions are reported at the guard of the case: column 0 of a 10-layer utterance is row 16
  g = torch.ones(1, 8, 576)
  g[0, 0, 512] = 2.0
  assert S.worst("z", g, torch.ones(1, 8, 576), 16)[1] == (0, 512, 63, 31)
  assert S.worst("z", g, torch.ones(1, 8, 576), 8)[1] == (0, 512, 63, 24)


def test_reach_cotangent_is_local():
  for name in S.DEEP_IDS + S.WIDE_IDS:
    for d in H.DIRECTIONS:
      c = S._case(name, d)
      per_col = S.columns("z" if d == "fwd" else "audio", c.cotangent("reach")).abs().amax(dim=(0, 2))
      want = sorted({j for x in c.reach_columns() for j in range(max(x - 32, 0), min(x + 32, c.L))})
      assert sorted(torch.nonzero(per_col).flatten().tolist()) == want
      assert all(per_col[x] > 0 for x in c.reach_columns())


def _misses(c, ref, yard, where, fault):
  got = S.run(c, True, where, fault=fault, emulate=True)
  miss = S.check(got, ref, yard, f"{fault} {c.name}/{c.direction}", factor=2.0 * S.BOUND_FACTOR, quiet=True, case=c)
  e = H.errors(got, ref)
  rel = max((err / max(den, 1e-30), q) for q, (err, den) in e.items() if q not in ("loss", "log_det"))
  cols = [(round(r, 1), q, pos) for r, q, pos in miss if pos is not None]
  par = [(round(r, 1), q) for r, q, pos in miss if pos is None]
  print(f"{fault} {c.name}/{c.direction} {where}: beyond 2 x the bound: columns {cols}; {len(par)} parameter gradients, worst "
        f"{par[:1]}; worst whole-tensor relative error {rel[0]:.2e} ({rel[1]}) beside {WHOLE_TENSOR}")
  return cols, par


@pytest.mark.parametrize("direction", H.DIRECTIONS)
def test_deep_taps_need_the_reach_cotangent(direction):
  """Under "edge" a lost or misplaced left tap of the layers of dilation 256 and 512 moves no gradient beyond the bound
  (column d and the interior columns carry no cotangent); under "reach" it reaches a data gradient and the parameter
  gradients of its own layer."""
  c = S._case(DEEP, direction)
  for where in ("edge", "reach"):
    ref, yard = S.oracle(DEEP, direction, True, where), S.yardstick(DEEP, direction, True, where)
    for fault in (("drop_tap", 1, 9), ("drop_tap", 0, 8), ("seam", 1, 9, 540), ("seam", 0, 8, 300)):
      cols, par = _misses(c, ref, yard, where, fault)
      grads = [q for _, q, _ in cols if q.startswith("d ")]
      own = [q for _, q in par if q.startswith(f"p/WN.{fault[1]}.in_layers.{fault[2]}.")]
      if where == "reach":
        assert grads and own, (fault, cols, par[:4])
      elif fault[0] == "drop_tap":
        assert not grads and not par, (fault, cols, par[:4])


@pytest.mark.parametrize("direction", H.DIRECTIONS)
def test_deep_planted_faults_exceed_the_per_column_bound(direction):
  """(b) and (c) at seam_l10_c64 under the loss (training) or the values (synthesis) and under "reach".  wgrad_last omits
  the LAST column's term, which "reach" gives no cotangent and a values-only run no gradient: it is held under the loss
  in the training direction and under "edge" in the synthesis direction."""
  c = S._case(DEEP, direction)
  plain = "loss" if direction == "fwd" else "values"
  wgrad_where = "loss" if direction == "fwd" else "edge"
  for where in dict.fromkeys((plain, "reach", wgrad_where)):
    ref, yard = S.oracle(DEEP, direction, True, where), S.yardstick(DEEP, direction, True, where)
    print(f"{DEEP}/{direction} {where} yardsticks:", {q: f"{v:.2e}" for q, v in yard.items() if not q.startswith("p/")})
    for fault in DEEP_FAULTS:
      wgrad = fault[0] == "wgrad_last"
      if (wgrad and where != wgrad_where) or (not wgrad and where == "edge"):
        continue
      cols, par = _misses(c, ref, yard, where, fault)
      if wgrad:
        assert not cols                              # values and data gradients stay exact
        key = f"p/WN.{fault[1]}.in_layers.{fault[2]}."
        assert par and all(q.startswith(key) for _, q in par), par
      else:
        assert cols, f"{fault}: no column of {DEEP}/{direction} under {where} exceeds twice the per-column bound"
    if where == "edge":
      continue
    gen = torch.Generator().manual_seed(1000)
    for rep in range(3):
      got = S.run(c, True, where, emulate=True, dither=gen)
      miss = S.check(got, ref, yard, f"{DEEP}/{direction} {where} realisation {rep}", quiet=True, case=c)
      print(f"{DEEP}/{direction} {where} fault-free realisation {rep}: worst ratio to the yardstick "
            f"{max(v / yard[q] for q, v in S.statistics(got, ref).items() if yard[q] > 0):.2f}")
      assert not miss, miss[:4]


@pytest.mark.parametrize("direction", H.DIRECTIONS)
def test_fault_at_a_tile_seam_under_a_16_row_tap(direction):
  """(b) and (c) at tile_l10_c64: the left tap of dilation 512 of the first column behind row 64 (frame 48 of utterance 0)
  reads frame 32, 16 rows in front of the seam, one column off.  seam_l10_c64 has 18 frames and no such column, so the
  fault is planted in the case that has the seam."""
  name = "tile_l10_c64"
  c = S._case(name, direction)
  row, b, f = c.tile_seam()
  assert (row, b, f) == (64, 0, 48)
  ref = S.oracle(name, direction, True, "seam")
  yard = S.yardstick(name, direction, True, "seam")
  cols, par = _misses(c, ref, yard, "seam", ("seam", 1, 9, 32 * f))
  assert cols and any(pos[3] == 0 for _, _, pos in cols), cols
  gen = torch.Generator().manual_seed(1000)
  for rep in range(3):
    miss = S.check(S.run(c, True, "seam", emulate=True, dither=gen), ref, yard, f"{name}/{direction} realisation {rep}",
                   quiet=True, case=c)
    assert not miss, miss[:4]
