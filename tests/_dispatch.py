"""Shared by tests/test_dispatch_cpu.py and tests/test_gpu_dispatch_identity.py: the kernel classes the library's own
dispatcher reaches (``wg_plan``, waveglow_amd/csrc/wg_plan.h) and the search for shapes that land in them.

A class is what makes two launches DIFFERENT KERNELS: the tile width, the launch form (single tiles, pairs, the resident
walk), the deep-prefetch kernel and the 16x16x32 MFMA loop.  The README's bit-identity promises compare calls of different
workload size, i.e. of different classes; the GPU test crosses every pair the table below names, at shapes found here for
the device's own CU count, and this module's CPU test checks that the search succeeds at 256 CUs.
"""
from waveglow_amd import _lib

INFER, FORWARD, TRAIN = _lib.WG_PLAN_INFER, _lib.WG_PLAN_FORWARD, _lib.WG_PLAN_TRAIN
SINGLE, PAIR, RESIDENT = _lib.WG_PLAN_SINGLE, _lib.WG_PLAN_PAIR, _lib.WG_PLAN_RESIDENT
FORMS = {SINGLE: "single tiles", PAIR: "pairs", RESIDENT: "resident walk"}
MAX_ROWS = 8192                      # B * Fp of every shape the tests use
SWITCHES = ("WG_FORCE_BN", "WG_RESIDENT", "WG_DISABLE_DEEP", "WG_NO_START_FOLD")

# channels: {class: the fields of wg_plan_result that define it}
CLASSES = {
  256: {"small": dict(block_n=64, form=SINGLE, deep=1, frag16=0),
        "middle": dict(block_n=128, form=SINGLE, deep=0, frag16=1),
        "large": dict(block_n=128, form=RESIDENT, deep=0, frag16=1)},
  128: {"small": dict(block_n=64, form=SINGLE, deep=0, frag16=0),
        "middle": dict(block_n=128, form=SINGLE, deep=0, frag16=0),
        "large": dict(block_n=128, form=PAIR, deep=0, frag16=0)},
  512: {"small": dict(block_n=64, form=SINGLE, deep=0, frag16=0),
        "large": dict(block_n=64, form=PAIR, deep=0, frag16=0)},
}
CLASSES[64] = CLASSES[128]
# Rp at which each class was found by hand from the rules at 256 CUs
BY_HAND_256 = {256: {"small": 128, "middle": 640, "large": 2048}, 64: {"small": 128, "middle": 640, "large": 4096},
               512: {"small": 128, "large": 2048}}


def clean_environment(monkeypatch):
  """Every switch that pins a kernel choice leaves the environment: the dispatcher decides."""
  import os
  for k in list(os.environ):
    if k in SWITCHES or k.startswith("WG_TRAIN_"):
      monkeypatch.delenv(k)


def config(channels, n_layers=8, n_flows=4, n_early_every=2, n_mel=80):
  return _lib.WgConfig(n_mel, n_flows, 8, n_early_every, 2, n_layers, channels, 3, 1024, 256)


def config_of(hp):
  return config(hp.n_channels, hp.n_layers, hp.n_flows, hp.n_early_every, (hp.n_mel_channels + 15) // 16 * 16)


def plan(cfg, direction, B, T, n_cu):
  return _lib.plan(cfg, direction, B, T, n_cu)


def fields(p):
  return {n: getattr(p, n) for n, _ in p._fields_}


def describe(p):
  """One line for the test log: the plan a side of a comparison ran."""
  s = f"Rp {p.rows_per_phase}: {p.n_tiles} tiles of {p.block_n} columns, {FORMS[p.form]}"
  if p.form == RESIDENT:
    s += f" ({p.resident_wgs} workgroups)"
  if p.deep:
    s += ", deep prefetch"
  if p.frag16:
    s += ", 16x16x32 MFMA"
  if p.halves == 2:
    s += ", two half-batch chains"
  return s


def class_of(channels, p):
  """Name of the class a plan is in, or None (e.g. 64-column pairs at 256 channels: no test crosses into those)."""
  f = fields(p)
  for name, want in CLASSES[channels].items():
    if all(f[k] == v for k, v in want.items()):
      return name
  return None


def same_kernel(p, q):
  return all(getattr(p, k) == getattr(q, k) for k in ("block_n", "form", "deep", "frag16"))


def find_batch(channels, cls, n_cu, direction=INFER, min_B=4, n_layers=8):
  """(B, T) of the cheapest batch with B >= min_B and B * Fp <= MAX_ROWS whose plan is in class ``cls`` while every
  utterance of up to T frames runs alone in the small class; None if there is none.  T >= 16: room for unequal lengths."""
  cfg, best = config(channels, n_layers), None
  for B in range(min_B, 65):
    for T in range(16, MAX_ROWS // B - 8 + 1, 4):
      if best is not None and B * (T + 8) >= best[0]:
        break
      if class_of(channels, plan(cfg, direction, B, T, n_cu)) != cls:
        continue
      if class_of(channels, plan(cfg, direction, 1, T, n_cu)) != "small":
        break                                   # longer utterances only leave the small class further behind
      best = (B * (T + 8), B, T)
  return None if best is None else best[1:]


def find_single(channels, cls, n_cu, direction=INFER, n_layers=8, step=4):
  """The shortest utterance (frames, a multiple of ``step``) whose own call is in class ``cls``; None if there is none."""
  cfg = config(channels, n_layers)
  for T in range(step, MAX_ROWS - 8 + 1, step):
    if class_of(channels, plan(cfg, direction, 1, T, n_cu)) == cls:
      return T
  return None


def lengths(B, T):
  """Unequal frame counts of a batch padded to T: the longest second, the shortest third, no two neighbours alike."""
  lens = [T - 1 - (5 * b) % (T // 2) for b in range(B)]
  lens[1] = T
  lens[2] = max(1, T // 8)
  return lens


# ---------------------------------------------------------------- the rules, restated from the comments of wg_plan.h
def _ceil(a, b):
  return -(-a // b)


def rule_widest(channels):
  return 64 if channels >= 512 else 128


def rule_infer_bn(channels, Rp, n_cu):
  """64-column tiles where they buy whole rounds: a narrow tile costs 0.6 of a wide one, below four wide tiles per CU."""
  if rule_widest(channels) == 64:
    return 64
  t128 = 32 * Rp // 128
  return 64 if t128 < 4 * n_cu and 6 * _ceil(2 * t128, n_cu) < 10 * _ceil(t128, n_cu) else 128      # 0.6 r64 < r128


def rule_launch(channels, bn, n_tiles, n_cu, n_mel=80):
  """(form, resident workgroups, deep)."""
  tail = n_tiles % n_cu
  if channels == 256 and bn == 128 and n_tiles >= 2 * n_cu and not 0 < tail < n_cu / 4:
    return RESIDENT, 8 * min(_ceil(_ceil(n_tiles, 8), 2), _ceil(n_cu, 8)), 0
  if n_tiles >= 4 * n_cu and 2 * _ceil(_ceil(n_tiles, 2), n_cu) <= _ceil(n_tiles, n_cu):
    return PAIR, 0, 0
  return SINGLE, 0, int(channels == 256 and bn == 64 and n_mel == 80)


def rule_train(channels, B, Fp, n_cu):
  """(tile width, halves, Fp, Rp) of the training forward."""
  Rp = _ceil(B * Fp, 128) * 128
  halves = 1
  if B % 2 == 0:
    fp = Fp
    while (B // 2 * fp) % 128:
      fp += 1
    tiles = 32 * Rp // 128
    idle = _ceil(tiles, n_cu) * n_cu - tiles
    if tiles > n_cu and 10 * idle >= tiles and B * fp <= Rp + Rp // 32:
      halves, Fp, Rp = 2, fp, B * fp
  bn = 64 if rule_widest(channels) == 128 and 32 * (Rp // 128) < n_cu else rule_widest(channels)
  return bn, halves, Fp, Rp
