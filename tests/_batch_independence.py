"""Shared by tests/test_gpu_batch_independence.py and tests/test_batch_independence_cpu.py: the gradient paths must not
depend on the batch an utterance is in.

One model, one fixed set of inputs and cotangents for a batch of B utterances; the same call on every utterance alone
(B = 1, its slice of the inputs and cotangents).  The losses are linear in the outputs and nothing is normalised by the
batch, so with the SAME loss scale in every call (2^round(log2 N) of the batch; the cotangents carry 1 / N of the batch)

* row b of every value (z, log_s_k, audio) and of every input gradient (d mel, d audio, d z_init, d z_early) of the batch
  call is the single call's -- on the GPU bit for bit: each is a per-column / per-frame quantity whose reduction runs over
  channels and taps in an order that does not depend on where the column sits in a tile, a slab or the batch;
* every parameter gradient is additive, g(batch) = sum_b g(utterance b) -- up to the fp32 accumulation order, since these
  reduce over positions.  How much the order alone moves them is measured on the reference (this module's oracle in
  float32, ``measure_f32``) and recorded in ``F32_RATIO``; the GPU bound is ``FACTOR`` x that figure per tensor plus the
  suite's absolute floor;
* log_det_W_k = B L logdet W_k is one fp32 rounding per call: the fp64 sum of the single calls and the batch's value agree
  to 2^-22 relative (tests/test_gpu_envelope.py).

The utterances of a batch differ (mel, audio / noise and cotangents per row), and row 1 is ``LOUD`` times its neighbours in
the audio, the noise and the cotangents, so that a leak out of it shows in a quiet row.
"""
import torch

import _corners as K
import _hot as H
from _cases import GRAD_TOL, oracle_cfg_from_hp
from waveglow_amd import synthetic
from waveglow_amd.hparams import HParams

SIGMA = 0.7
LOUD = 8.0                      # row LOUD_ROW against every other row
LOUD_ROW = 1
FLOOR = 1e-7                    # the absolute floor of _cases._check
FACTOR = 4.0                    # MFMA K-chunking and slab order differ from torch's blocking; the element count per sum does not
LOGDET_TOL = 2.0 ** -22
BOUND_LIMIT = GRAD_TOL / 50     # a bound above this would not be worth the name: change the case, not the factor
ROW_TOL_64 = 1e-11              # "equal to fp64 rounding" on the CPU: 2^-53 = 1.1e-16 with five decades for the depth
DIRECTIONS = ("fwd", "inv")     # training direction (forward + backward), synthesis direction (infer_differentiable)

# id: (HParams overrides, B, T, audio crop of the training direction, weight seed; None: the flow-corner fixture's)
CASES = {
  # L = 413 columns per utterance (a partial last frame); the widest dilation, 128, reaches well across an utterance
  "c64_l8": (dict(n_channels=64, n_layers=8, n_flows=4, n_early_every=2), 4, 13, 24, 6),
  # L = 160 is below the dilations 256 and 512: every outer tap of the last layers lands in padding or guard rows; B is
  # odd (the library splits even batches only: this one runs as one chain whatever WG_TRAIN_HALVES says).  The cases whose
  # taps of dilation 256 and 512 reach real samples, against the fp64 oracle, are seam_l10_*, seam_l9_c128 and tile_l10_*
  # of tests/_seams.py (576 and 1664 columns per utterance)
  "c64_l10": (dict(n_channels=64, n_layers=10, n_flows=4, n_early_every=2), 3, 5, 0, 7),
  "c256_l8": (dict(n_channels=256, n_layers=8, n_flows=4, n_early_every=2), 4, 13, 24, 6),
  # flow widths 8, 6, 4, 2 in one model (tests/_corners.py), training direction only
  "c2": (K.LAYOUTS["c2"], 3, 7, 24, None),
  # The batch and a single utterance on different kernels at the library's own choice (tests/test_gpu_dispatch_identity.py):
  # 12 x (80 + 8) = 1056 rows per phase are 288 tiles of 128 columns, at least one per CU of a 256-CU device, so the batch
  # runs the fused layer kernel on 128-column tiles and an utterance alone (88 rows) on 64-column ones (wg_plan says so, and
  # tests/test_dispatch_cpu.py asserts it); GPU only, unpinned
  "c256_wide": (dict(n_channels=256, n_layers=8, n_flows=4, n_early_every=2), 12, 80, 24, 6),
  "c64_wide": (dict(n_channels=64, n_layers=8, n_flows=4, n_early_every=2), 12, 80, 24, 6),
}

# Worst per-tensor ||g(batch) - sum_b g(utterance b)|| / ||g(batch)|| of the float32 oracle (``measure_f32``): the larger of
# a one-thread and a many-thread run.  tests/test_batch_independence_cpu.py measures them again.
F32_RATIO = {
  ("c64_l8", "fwd"): 1.15e-6, ("c64_l8", "inv"): 1.66e-6,
  ("c64_l10", "fwd"): 8.9e-7, ("c64_l10", "inv"): 1.17e-6,
  ("c256_l8", "fwd"): 1.36e-6, ("c256_l8", "inv"): 1.72e-6,
  ("c2", "fwd"): 9.1e-7,
  # 12 utterances of 2557 / 2560 columns: the bias gradients, sums over 30 720 positions, lead
  ("c64_wide", "fwd"): 5.1e-6, ("c64_wide", "inv"): 5.07e-6,
  ("c256_wide", "fwd"): 4.88e-6, ("c256_wide", "inv"): 4.88e-6,
}


def bound(name, direction):
  """Relative part of the GPU bound of every parameter gradient of a case (the floor comes on top)."""
  return FACTOR * F32_RATIO[(name, direction)]


class Case:
  """Model, inputs and cotangents of one case, on the CPU.  ``sd`` is in weight-norm form."""

  def __init__(self, name):
    over, self.B, self.T, self.crop, wseed = CASES[name]
    self.name = name
    self.hp = HParams(**over)
    self.cfg = oracle_cfg_from_hp(self.hp)
    if wseed is None:
      wseed = int(K.fixture()[f"{name}/weight_seed"])
    self.sd = synthetic.to_weightnorm_form(synthetic.make_state_dict(self.hp, seed=wseed))
    B, T = self.B, self.T
    g = torch.Generator().manual_seed(7700 + 10 * B + T)
    amp = torch.full((B,), 1.0 / LOUD)
    amp[LOUD_ROW] = 1.0
    self.mel = synthetic.make_mel(B, T, self.hp.n_mel_channels, seed=1234 + B + T)      # rows differ
    # training direction
    self.S = 256 * T - self.crop
    self.L = self.S // self.hp.n_group
    assert self.S % self.hp.n_group == 0
    self.wav = (torch.rand(B, self.S, generator=g) * 1.2 - 0.6) * amp[:, None]
    self.n_fwd = B * self.S
    self.scale_fwd = H.grad_scale(self.n_fwd)
    cot = amp * LOUD / self.n_fwd                                                       # 1 / N, the loud row 8 / N
    chans = synthetic.flow_channels(self.hp)
    self.r_z = torch.randn(B, self.hp.n_group, self.L, generator=g) * cot[:, None, None]
    self.r_ls = [torch.randn(B, c // 2, self.L, generator=g) * cot[:, None, None] for c in chans]
    self.c_ld = [(0.5 + 0.25 * k) * (-1.0) ** k / self.n_fwd for k in range(self.hp.n_flows)]
    # synthesis direction: 32 T columns per utterance
    Ls = 32 * T
    self.z_init = torch.randn(B, chans[-1], Ls, generator=g) * (2.0 * amp)[:, None, None]
    self.z_early = {k: torch.randn(B, self.hp.n_early_size, Ls, generator=g) * (2.0 * amp)[:, None, None]
                    for k in reversed(K.early_flows(self.hp))}
    self.n_inv = B * 256 * T
    self.scale_inv = H.grad_scale(self.n_inv)
    self.r_audio = torch.randn(B, 256 * T, generator=g) * (amp * LOUD / self.n_inv)[:, None]

  def rows(self, b):
    return slice(None) if b is None else slice(b, b + 1)

  def z_early_list(self, rows):
    """z_early as ``infer_differentiable`` takes it: descending flow index."""
    return [self.z_early[k][rows] for k in sorted(self.z_early, reverse=True)]


_cases = {}


def case(name):
  if name not in _cases:
    _cases[name] = Case(name)
  return _cases[name]


def train_loss(c, rows, z, log_s, log_det):
  """(z r_z).sum() + sum_k (log_s_k r_k).sum() + sum_k c_k log_det_k on the device and dtype of ``z``."""
  to = lambda t: t[rows].to(device=z.device, dtype=z.dtype)
  loss = (z * to(c.r_z)).sum()
  for ls, r in zip(log_s, c.r_ls):
    loss = loss + (ls * to(r)).sum()
  for ld, ck in zip(log_det, c.c_ld):
    loss = loss + ck * ld
  return loss


# ---------------------------------------------------------------- the oracle on the same calls
def oracle(c, direction, b=None, dtype=torch.float64, fault=None):
  """The call on the whole batch (``b`` None) or on utterance b alone, through the chain of tests/_hot.py in ``dtype``.
  {quantity: tensor}: z, log_s.k, log_det, d mel, d audio / audio, d mel, d z_init, d z_early.i, and p/<parameter>."""
  rows, P = c.rows(b), H.Prec(fault=fault)
  if direction == "inv":
    return H.run_infer(c.sd, c.mel[rows], c.z_init[rows], {k: v[rows] for k, v in c.z_early.items()}, SIGMA, c.cfg, P,
                       dtype, r=c.r_audio[rows])
  leaves = H._leaves(c.sd, dtype)
  m, a = c.mel[rows].to(dtype).requires_grad_(True), c.wav[rows].to(dtype).requires_grad_(True)
  z, log_s, log_det = H.forward(H.compose(leaves), m, a, c.cfg, P)
  names = list(leaves)
  gs = torch.autograd.grad(train_loss(c, rows, z, log_s, log_det), [leaves[n] for n in names] + [m, a])
  out = {"z": z.detach(), "log_det": torch.stack([x.detach() for x in log_det])}
  out.update({f"log_s.{k}": ls.detach() for k, ls in enumerate(log_s)})
  out.update({f"p/{n}": g for n, g in zip(names, gs[:len(names)])})
  out["d mel"], out["d audio"] = gs[-2], gs[-1]
  return out


def batch_and_singles(c, direction, dtype=torch.float64, fault=None):
  return oracle(c, direction, None, dtype, fault), [oracle(c, direction, b, dtype, fault) for b in range(c.B)]


# ---------------------------------------------------------------- the comparison
def row_quantities(result):
  """The per-utterance quantities of a result: everything but the parameter gradients and log_det."""
  return [q for q in result if not q.startswith("p/") and q != "log_det"]


def row_differences(batch, singles):
  """{quantity: [||batch[b] - single_b|| / ||single_b|| for every b]} in fp64."""
  out = {}
  for q in row_quantities(batch):
    out[q] = []
    for b, one in enumerate(singles):
      x, y = batch[q][b:b + 1].detach().double().cpu(), one[q].detach().double().cpu()
      assert x.shape == y.shape, (q, b)
      out[q].append(float((x - y).norm()) / max(float(y.norm()), 1e-300))
  return out


def additive_errors(batch, singles, hp=None):
  """{parameter: (||g(batch) - sum_b g(utterance b)||, ||g(batch)||)}, the sum formed in fp64 on the host.  With ``hp`` the
  tensors that are zero by construction (tests/_corners.py: structurally_zero) are left out."""
  out = {}
  for q, g in batch.items():
    if not q.startswith("p/") or (hp is not None and K.structurally_zero(hp, q[2:])):
      continue
    g = g.detach().double().cpu()
    total = torch.zeros_like(g)
    for one in singles:
      total += one[q].detach().double().cpu()
    out[q[2:]] = (float((g - total).norm()), float(g.norm()))
  return out


def worst_ratio(errs):
  """(worst err / norm, its parameter) of ``additive_errors``."""
  return max((e / max(n, 1e-300), q) for q, (e, n) in errs.items())


def measure_f32(name, direction):
  """The float32 oracle's own reorder ratio of a case: what ``F32_RATIO`` records."""
  c = case(name)
  batch, singles = batch_and_singles(c, direction, torch.float32)
  return worst_ratio(additive_errors(batch, singles, c.hp))


def check_additive(batch, singles, rel, what, hp):
  """Every parameter gradient: ||g(batch) - sum_b g(b)|| <= rel ||g(batch)|| + FLOOR, finite.  Prints the worst ratios and
  returns (misses, worst ratio); the tensors that are zero by construction are held to the floor like the others but
  left out of the printed ratios, which would be rounding over rounding."""
  errs = additive_errors(batch, singles)
  rows = sorted(((e / max(n, 1e-300), q, e, n) for q, (e, n) in errs.items()), reverse=True)
  for q, (e, n) in errs.items():
    assert e == e and n == n and n != float("inf"), f"{what}: {q}: not finite"
  misses = [(r, q) for r, q, e, n in rows if not e <= rel * n + FLOOR]
  rows = [x for x in rows if not K.structurally_zero(hp, x[1])]
  for r, q, e, n in rows[:4]:
    print(f"{what}: {q}: |g(batch) - sum g(single)| / |g(batch)| = {r:.3e} (err {e:.3e}, norm {n:.3e})")
  return misses, rows[0][0]


def check_logdet(batch, singles, what):
  """log_det_W_k of the batch against the fp64 sum of the single calls' values, 2^-22 relative."""
  ld = batch["log_det"].detach().double().cpu()
  total = sum(one["log_det"].detach().double().cpu() for one in singles)
  for k in range(ld.numel()):
    assert abs(float(ld[k]) - float(total[k])) <= LOGDET_TOL * abs(float(total[k])), (what, k, float(ld[k]), float(total[k]))


def rows_bit_for_bit(batch, singles, what):
  """Row b of every per-utterance quantity against the single call's, where the tensors are (the GPU tests: on the
  device); a mismatch is reported with the columns it covers (the first or last d columns of an utterance: guards;
  multiples of 64 / 128: tile seams)."""
  bad = []
  for q in row_quantities(batch):
    assert batch[q] is not None and bool(torch.isfinite(batch[q]).all()), f"{what}: {q}"
    for b, one in enumerate(singles):
      x, y = batch[q][b:b + 1], one[q]
      assert x.shape == y.shape, (what, q, b)
      if not torch.equal(x, y):
        cols = torch.nonzero((x != y).reshape(-1, x.shape[-1]).any(0)).flatten()
        bad.append(f"{q} row {b}: {int((x != y).sum())} of {x.numel()} differ, columns {int(cols[0])} .. {int(cols[-1])}, "
                   f"max |diff| {float((x - y).abs().max()):.3e}")
  assert not bad, f"{what}: the batch call differs from the batch-of-one calls:\n  " + "\n  ".join(bad[:24])


def compare(batch, singles, c, direction, what):
  """What the GPU tests assert of a batch call and its batch-of-one calls (module docstring)."""
  rows_bit_for_bit(batch, singles, what)
  if "log_det" in batch:
    check_logdet(batch, singles, what)
  if any(q.startswith("p/") for q in batch):
    rel = bound(c.name, direction)
    assert 0.0 < rel <= BOUND_LIMIT
    misses, worst = check_additive(batch, singles, rel, what, c.hp)
    print(f"{what}: worst additive ratio {worst:.3e}, bound {rel:.3e} (+ {FLOOR:g})")
    assert not misses, f"{what}: parameter gradients of the batch are not the sum of the single calls': {misses[:8]}"
