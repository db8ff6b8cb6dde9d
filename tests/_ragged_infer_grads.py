"""Shared by tests/test_gpu_infer_ragged.py and tests/test_infer_ragged_cpu.py: ``infer_differentiable(..., frames=)``, the
synthesis direction under autograd on a padded batch of utterances of different lengths.

The cases are those of tests/_batch_independence.py (rows differ, row 1 is ``LOUD``) with one frame count per utterance.
Utterance b is its CROP -- ``mel[b, :, :f]``, ``z_init[b, :, :32 f]``, ``z_early[k][b, :, :32 f]`` and the cotangent
``r_audio[b, :256 f]`` -- synthesised alone, and everything behind the count is NaN in the padded tensors the ragged call
gets.  The truth of an utterance is ``_hot.run_infer`` in fp64 on its crop: the reference has no ragged mode and needs none.

What the GPU tests assert, with the same explicit loss scale (``scale_inv`` of the padded batch, which is the automatic one)
in the ragged call and in every batch-of-one call:

* audio, d mel, d z_init and every d z_early[i] have the single call's bits in front of the count and are exactly 0 behind
  it;
* every parameter gradient is the fp64 sum of the GPU single calls' within ``FACTOR`` x ``F32_RATIO`` plus the suite's
  floor, and meets the fp64 oracle's sum over the crops at ``GRAD_TOL``.

``F32_RATIO`` is measured on the CPU oracle, not on the code under test: the worst per-tensor
``||sum_b g32(crop b) - sum_b g64(crop b)|| / ||sum_b g64(crop b)||`` of the float32 oracle (``measure_f32``), what float32
arithmetic alone does to these sums.  tests/test_infer_ragged_cpu.py measures it again.
"""
import torch

import _batch_independence as BI
import _corners as K
import _hot as H
from waveglow_amd import synthetic

NAN = float("nan")
FACTOR, FLOOR, BOUND_LIMIT = BI.FACTOR, BI.FLOOR, BI.BOUND_LIMIT
SIGMA = BI.SIGMA

# id: frame counts.  (B, T) are the case's own: (4, 13), (3, 5), (4, 13)
FRAMES = {
  # one full row; 160 columns end inside a 128-column tile and on a 32-column phase wrap; 32 columns are below every
  # dilation of 32 or more: every outer tap of those layers lands in padding or guard rows
  "c64_l8": [13, 5, 1, 9],
  # odd B (no half-batch split); the dilations 256 and 512 exceed every utterance
  "c64_l10": [2, 5, 3],
  "c256_l8": [7, 13, 4, 13],
}
# a second set of counts per case (the stale-workspace test runs it in between): every count differs from the first set's
FRAMES_2 = {"c64_l8": [6, 13, 11, 2], "c64_l10": [5, 1, 4], "c256_l8": [13, 2, 9, 5]}

# Worst per-tensor ratio of the float32 oracle (module docstring): the larger of a one-thread and a many-thread run.
F32_RATIO = {"c64_l8": 1.01e-6, "c64_l10": 1.03e-6, "c256_l8": 1.18e-6}


def bound(name):
  """Relative part of the GPU bound of every parameter gradient of a case (the floor comes on top)."""
  return FACTOR * F32_RATIO[name]


class Case:
  """A case of tests/_batch_independence.py with its frame counts: crops, and NaN-padded batch tensors."""

  def __init__(self, name, frames=None):
    self.c = BI.case(name)
    self.name, self.hp, self.cfg, self.B, self.T = name, self.c.hp, self.c.cfg, self.c.B, self.c.T
    self.frames = list(FRAMES[name] if frames is None else frames)
    assert len(self.frames) == self.B and all(1 <= f <= self.T for f in self.frames)
    self.scale = self.c.scale_inv                     # of the padded tensor: B * 256 * T samples
    self.sd = self.c.sd                               # weight-norm form
    self.keys = sorted(self.c.z_early, reverse=True)  # z_early as infer_differentiable takes it: descending flow index

  def dense_sd(self):
    """The same weights after remove_weightnorm (the state dict the weight-norm form was made from)."""
    return synthetic.make_state_dict(self.hp, seed=BI.CASES[self.name][4])

  def crop(self, b):
    """(mel, z_init, {k: z_early}, r_audio) of utterance b alone."""
    f, c = self.frames[b], self.c
    return (c.mel[b:b + 1, :, :f].clone(), c.z_init[b:b + 1, :, :32 * f].clone(),
            {k: v[b:b + 1, :, :32 * f].clone() for k, v in c.z_early.items()}, c.r_audio[b:b + 1, :256 * f].clone())

  def padded(self, fill=NAN, frames=None):
    """(mel, z_init, [z_early descending], r_audio) of the batch, ``fill`` behind every count (``frames``: other counts
    than the case's, 0 for an utterance that is all padding)."""
    c = self.c
    mel, zi, r = c.mel.clone(), c.z_init.clone(), c.r_audio.clone()
    ze = [c.z_early[k].clone() for k in self.keys]
    for b, f in enumerate(self.frames if frames is None else frames):
      mel[b, :, f:] = fill
      zi[b, :, 32 * f:] = fill
      r[b, 256 * f:] = fill
      for z in ze:
        z[b, :, 32 * f:] = fill
    return mel, zi, ze, r


_cases = {}


def case(name):
  if name not in _cases:
    _cases[name] = Case(name)
  return _cases[name]


# ---------------------------------------------------------------- the oracle on the crops
def oracle_crop(rc, b, dtype=torch.float64, sd=None):
  """``_hot.run_infer`` on utterance b alone: audio, d mel, d z_init, d z_early.i, p/<parameter>."""
  mel, zi, ze, r = rc.crop(b)
  return H.run_infer(rc.sd if sd is None else sd, mel, zi, ze, SIGMA, rc.cfg, H.EXACT, dtype, r=r)


def oracle_dense(rc, dtype=torch.float64):
  """The padded batch as a DENSE call (zeros for the cotangent behind the counts): what the flow computed before frames=."""
  c = rc.c
  r = rc.padded(0.0)[3]
  return H.run_infer(rc.sd, c.mel, c.z_init, c.z_early, SIGMA, rc.cfg, H.EXACT, dtype, r=r)


def param_sum(results):
  """{parameter: fp64 host sum over the results} of the p/ entries."""
  out = {}
  for one in results:
    for q, g in one.items():
      if q.startswith("p/"):
        g = g.detach().double().cpu()
        out[q] = out[q] + g if q in out else g.clone()
  return out


_sums = {}


def oracle_sum(name, dense=False):
  """fp64 oracle: {p/<parameter>: sum over the crops}, in weight-norm form or (``dense``) after remove_weightnorm.  Computed
  once per case and form."""
  if (name, dense) not in _sums:
    rc = case(name)
    sd = rc.dense_sd() if dense else None
    _sums[(name, dense)] = param_sum([oracle_crop(rc, b, torch.float64, sd) for b in range(rc.B)])
  return _sums[(name, dense)]


def measure_f32(name):
  """(worst ratio, its parameter): the float32 oracle's sum over the crops against the fp64 oracle's (``F32_RATIO``)."""
  rc = case(name)
  s64 = oracle_sum(name)
  s32 = param_sum([oracle_crop(rc, b, torch.float32) for b in range(rc.B)])
  worst = (0.0, "")
  for q, ref in s64.items():
    if K.structurally_zero(rc.hp, q[2:]):
      continue
    worst = max(worst, (float((s32[q] - ref).norm()) / max(float(ref.norm()), 1e-300), q[2:]))
  return worst


# ---------------------------------------------------------------- the comparison
def rows_bit_for_bit(rc, batch, singles, what, frames=None):
  """Every per-utterance quantity of the ragged call, where the tensors are: the single call's bits in front of the count,
  exact zeros behind it, everything finite.  The last axis of every quantity is time: ``unit`` entries per frame.  An entry
  None of ``singles``: that row is only held to the zeros behind its count."""
  frames = rc.frames if frames is None else frames
  bad = []
  for q in BI.row_quantities(batch):
    x = batch[q]
    assert x is not None and bool(torch.isfinite(x).all()), f"{what}: {q} is not finite"
    unit = x.shape[-1] // rc.T
    assert unit * rc.T == x.shape[-1], (q, x.shape)
    for b, one in enumerate(singles):
      n = unit * frames[b]
      front, back = x[b:b + 1, ..., :n], x[b:b + 1, ..., n:]
      if one is not None:
        y = one[q]
        assert front.shape == y.shape, (what, q, b, front.shape, y.shape)
        if not torch.equal(front, y):
          cols = torch.nonzero((front != y).reshape(-1, n).any(0)).flatten()
          bad.append(f"{q} row {b}: {int((front != y).sum())} of {y.numel()} differ, columns {int(cols[0])} .. {int(cols[-1])} "
                     f"of {n}, max |diff| {float((front - y).abs().max()):.3e}")
      if not torch.equal(back, torch.zeros_like(back)):
        bad.append(f"{q} row {b}: {int((back != 0).sum())} entries behind the count are not 0")
  assert not bad, f"{what}: the ragged call differs from the batch-of-one calls:\n  " + "\n  ".join(bad[:24])


def check_parity(grads, name, dense, tol, what):
  """Every parameter gradient of the ragged call against the fp64 oracle's sum over the crops: ||g - ref|| <= tol ||ref|| +
  FLOOR.  Prints the worst, returns the misses."""
  ref = oracle_sum(name, dense)
  assert set(grads) == set(ref), (what, sorted(set(grads) ^ set(ref))[:8])
  rows = []
  for q, r in ref.items():
    g = grads[q].detach().double().cpu()
    assert g.shape == r.shape and bool(torch.isfinite(g).all()), (what, q)
    rows.append((float((g - r).norm()), float(r.norm()), q))
  worst = sorted(((e / max(n, 1e-300), q, e, n) for e, n, q in rows if n > 0), reverse=True)
  for rel, q, e, n in worst[:4]:
    print(f"{what}: {q}: rel {rel:.3e} (err {e:.3e}, ref norm {n:.3e})")
  return [(q, e, n) for e, n, q in rows if not e <= tol * n + FLOOR]
