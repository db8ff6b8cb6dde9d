"""``wg_plan`` (the functions the launch code itself calls, waveglow_amd/csrc/wg_plan.h) against a Python restatement of
the dispatcher's rules (tests/_dispatch.py), the table of tile widths at 256 CUs, and the search for the kernel classes that
tests/test_gpu_dispatch_identity.py crosses.  No GPU."""
import pytest

import _batch_independence as BI
import _dispatch as D
from waveglow_amd import _lib, build

CHANNELS = (64, 128, 256, 512)
N_CU = (256, 304, 1)
ROWS = range(128, 8192 + 1, 128)


@pytest.fixture(autouse=True)
def _no_switches(monkeypatch):
  build.build_library()
  D.clean_environment(monkeypatch)


def _at(channels, direction, Rp, n_cu):
  """The plan of one utterance of Rp - 8 frames: Fp = Rp rows, no rounding."""
  return D.plan(D.config(channels), direction, 1, Rp - 8, n_cu)


@pytest.mark.parametrize("n_cu", N_CU)
@pytest.mark.parametrize("channels", CHANNELS)
def test_inference_and_forward_plans_follow_the_rules(channels, n_cu):
  seen = set()
  for Rp in ROWS:
    bn = D.rule_infer_bn(channels, Rp, n_cu)
    n_tiles = 32 * Rp // bn
    form, wgs, deep = D.rule_launch(channels, bn, n_tiles, n_cu)
    want = dict(block_n=bn, form=form, resident_wgs=wgs, deep=deep, frag16=int(channels == 256 and bn == 128), halves=1,
                rows_per_utterance=Rp, rows_per_phase=Rp, n_tiles=n_tiles)
    for direction in (D.INFER, D.FORWARD):
      assert D.fields(_at(channels, direction, Rp, n_cu)) == want, (channels, n_cu, Rp, direction)
    seen.add((bn, form, deep))
  if n_cu == 256:
    assert len(seen) >= len(D.CLASSES[channels])           # every class, and at 256 channels the 64-column pairs too


@pytest.mark.parametrize("n_cu", N_CU)
@pytest.mark.parametrize("channels", CHANNELS)
def test_training_plans_follow_the_rules(channels, n_cu):
  cfg = D.config(channels)
  halved = 0
  for B, T in [(1, Rp - 8) for Rp in ROWS] + [(B, T) for B in (2, 4, 6, 12, 16, 32) for T in (8, 24, 56, 63, 64, 80, 120, 248)]:
    bn, halves, Fp, Rp = D.rule_train(channels, B, T + 8, n_cu)
    p = D.plan(cfg, D.TRAIN, B, T, n_cu)
    want = dict(block_n=bn, form=D.SINGLE, resident_wgs=0, deep=0, frag16=0, halves=halves, rows_per_utterance=Fp,
                rows_per_phase=Rp, n_tiles=32 * (Rp // halves // bn))
    assert D.fields(p) == want, (channels, n_cu, B, T)
    halved += halves == 2
  assert halved or n_cu == 1                                # the half-batch chains are reached: 32 x 63 is config 4
  if n_cu == 256:
    assert D.plan(cfg, D.TRAIN, 32, 63, 256).halves == 2 and D.plan(cfg, D.TRAIN, 32, 63, 256).rows_per_utterance == 72


def test_tile_width_table_at_256_cus():
  """256 channels on 256 CUs, up to 8 layers: the table of DESIGN.md section 4e, as literals."""
  for Rp in ROWS:
    p = _at(256, D.INFER, Rp, 256)
    narrow = Rp <= 512 or 1152 <= Rp <= 1536
    assert p.block_n == (64 if narrow else 128), Rp
    assert p.deep == int(narrow) and p.frag16 == int(not narrow), Rp
  for Rp in (2048, 4096):
    p = _at(256, D.INFER, Rp, 256)
    assert (p.block_n, p.form, p.resident_wgs) == (128, D.RESIDENT, 256), Rp
  # the shapes of the README's promises: a 7 s utterance alone, a stream window of it, six 80-frame utterances, one of them
  cfg12 = D.config(256, n_flows=12, n_early_every=4)
  assert D.plan(cfg12, D.INFER, 1, 603, 256).rows_per_phase == 640 and D.plan(cfg12, D.INFER, 1, 603, 256).block_n == 128
  assert D.plan(cfg12, D.INFER, 1, 32 + 99 + 99, 256).rows_per_phase == 256 and D.plan(cfg12, D.INFER, 1, 230, 256).block_n == 64
  assert D.plan(cfg12, D.INFER, 6, 80, 256).rows_per_phase == 640 and D.plan(cfg12, D.INFER, 6, 80, 256).block_n == 128
  assert D.plan(cfg12, D.INFER, 1, 80, 256).rows_per_phase == 128 and D.plan(cfg12, D.INFER, 1, 80, 256).block_n == 64
  # 64 channels, 4096 rows: 1024 tiles, 4 rounds as single tiles or as pairs -> pairs
  p = _at(64, D.INFER, 4096, 256)
  assert (p.block_n, p.n_tiles, p.form) == (128, 1024, D.PAIR)


@pytest.mark.parametrize("channels", [64, 256, 512])
def test_classes_found_by_hand(channels):
  for cls, Rp in D.BY_HAND_256[channels].items():
    p = _at(channels, D.INFER, Rp, 256)
    assert D.class_of(channels, p) == cls, (channels, cls, Rp, D.describe(p))


@pytest.mark.parametrize("direction", [D.INFER, D.FORWARD])
@pytest.mark.parametrize("channels", CHANNELS)
def test_class_search_succeeds_at_256_cus(channels, direction):
  """Every class of tests/test_gpu_dispatch_identity.py is reached by a shape with B * Fp <= 8192, as a batch of utterances
  that run alone in the small class, and (256 channels) as a single utterance for the stream."""
  cfg = D.config(channels)
  for cls in D.CLASSES[channels]:
    if cls == "small":
      assert D.class_of(channels, D.plan(cfg, direction, 1, 16, 256)) == "small"
      continue
    found = D.find_batch(channels, cls, 256, direction)
    assert found is not None, (channels, cls)
    B, T = found
    lens = D.lengths(B, T)
    assert B * (T + 8) <= D.MAX_ROWS and max(lens) == lens[1] == T and min(lens) == lens[2] and len(set(lens)) > 2
    assert D.class_of(channels, D.plan(cfg, direction, B, T, 256)) == cls
    for t in lens:
      assert D.class_of(channels, D.plan(cfg, direction, 1, t, 256)) == "small"
    print(f"{channels} channels, {cls}: {B} x {T} frames -- {D.describe(D.plan(cfg, direction, B, T, 256))}")
  if channels == 256:
    mid, big = D.find_single(256, "middle", 256), D.find_single(256, "large", 256)
    assert (mid, big) == (508, 1916)                       # Rp 640 and 2048: the first rows of those classes
    assert D.find_single(256, "large", 256, step=8) + 8 <= D.MAX_ROWS


@pytest.mark.parametrize("name", ["c256_wide", "c64_wide"])
def test_wide_gradient_cases_cross_the_training_tile_widths(name):
  """tests/_batch_independence.py: the batch on 128-column tiles, an utterance alone on 64-column ones, one chain each."""
  over, B, T, _, _ = BI.CASES[name]
  cfg = D.config(over["n_channels"], over["n_layers"], over["n_flows"], over["n_early_every"])
  batch, one = D.plan(cfg, D.TRAIN, B, T, 256), D.plan(cfg, D.TRAIN, 1, T, 256)
  assert (batch.block_n, one.block_n) == (128, 64) and batch.halves == one.halves == 1


def test_switches_reach_the_plan(monkeypatch):
  cfg = D.config(256)
  monkeypatch.setenv("WG_FORCE_BN", "128")
  assert D.plan(cfg, D.INFER, 1, 16, 256).block_n == 128 and D.plan(cfg, D.TRAIN, 1, 16, 256).block_n == 128
  assert D.plan(D.config(512), D.INFER, 1, 16, 256).block_n == 64
  monkeypatch.setenv("WG_FORCE_BN", "64")
  assert D.plan(cfg, D.INFER, 1, 2040, 256).block_n == 64 and D.plan(cfg, D.TRAIN, 12, 80, 256).block_n == 64
  monkeypatch.delenv("WG_FORCE_BN")
  monkeypatch.setenv("WG_DISABLE_DEEP", "1")
  assert (D.plan(cfg, D.INFER, 1, 16, 256).block_n, D.plan(cfg, D.INFER, 1, 16, 256).deep) == (64, 0)
  monkeypatch.delenv("WG_DISABLE_DEEP")
  monkeypatch.setenv("WG_RESIDENT", "0")
  assert D.plan(cfg, D.INFER, 1, 4088, 256).form == D.PAIR           # 1024 tiles: resident without the switch
  monkeypatch.setenv("WG_RESIDENT", "20")
  p = D.plan(D.config(64), D.INFER, 1, 16, 256)
  assert (p.form, p.resident_wgs) == (D.RESIDENT, 24)
  monkeypatch.delenv("WG_RESIDENT")
  monkeypatch.setenv("WG_TRAIN_HALVES", "2")
  assert D.plan(cfg, D.TRAIN, 4, 13, 256).halves == 2 and D.plan(cfg, D.TRAIN, 3, 13, 256).halves == 1
  monkeypatch.setenv("WG_TRAIN_HALVES", "1")
  assert D.plan(cfg, D.TRAIN, 32, 63, 256).halves == 1


def test_refusals():
  import ctypes as C
  lib = _lib.load()
  out = _lib.WgPlanResult()
  cfg = D.config(256)
  for args in ((3, 1, 16, 256), (D.INFER, 0, 16, 256), (D.INFER, 1, 0, 256), (D.INFER, 1, 16, 0)):
    assert lib.wg_plan(C.byref(cfg), *args, C.byref(out)) == -1
  assert lib.wg_plan(C.byref(D.config(96)), D.INFER, 1, 16, 256, C.byref(out)) == -1
  assert lib.wg_plan(None, D.INFER, 1, 16, 256, C.byref(out)) == -1
  assert lib.wg_plan(C.byref(cfg), D.INFER, 1, 16, 256, None) == -1
  assert lib.wg_plan(C.byref(cfg), D.INFER, 4096, 4096, 256, C.byref(out)) == -1      # outside the size range of wg_infer
