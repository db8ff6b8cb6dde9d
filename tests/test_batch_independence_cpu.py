"""CPU companion of tests/test_gpu_batch_independence.py (tests/_batch_independence.py).

* the oracle itself meets the contract the GPU tests assert: batch against batch-of-one calls, values and input gradients
  equal to fp64 rounding, parameter gradients additive;
* the recorded float32 reorder ratios (``F32_RATIO``, from which the GPU bound is made) against a fresh measurement;
* a planted neighbour leak (tests/_hot.py: the ("leak", k, i) fault -- in one layer of one flow the right-hand padding of
  utterance b reads the first d columns of utterance b + 1) breaks "batch against singles" on the leaking utterances by a
  wide factor over the new bounds, while against the unfaulted oracle -- what every ``GRAD_TOL`` comparison of the suite
  amounts to -- it moves only the printed number of gradient tensors beyond ``GRAD_TOL``.
"""
import math

import pytest
import torch

import _batch_independence as BI
from _cases import GRAD_TOL
from waveglow_amd import synthetic

NAME = "c64_l8"                       # the first c64 case
MAIN = ("leak", 1, 0)                 # d = 1 in flow 1: the leak the present suite sees least of
FAULTS = (MAIN, ("leak", 1, 7))       # ... and the widest dilated tap, d = 128
WIDE = 10.0                           # "by a wide factor": the breach is at least this many times the bound it breaks
SETS = sorted(BI.F32_RATIO)


@pytest.fixture(scope="module")
def clean():
  """{direction: (batch result, [single results])} of the unfaulted fp64 oracle: computed once, never changed."""
  c = BI.case(NAME)
  return {d: BI.batch_and_singles(c, d) for d in BI.DIRECTIONS}


def test_cases_are_the_ones_that_expose_a_leak():
  c = BI.case("c64_l8")
  assert (c.B, c.L, c.S % 256) == (4, 413, 256 - 24) and 128 < c.L                     # a partial last frame
  c10 = BI.case("c64_l10")
  assert (c10.B, c10.L) == (3, 160) and c10.L < 256 < 512 == 2 ** (c10.hp.n_layers - 1)  # outer taps beyond the utterance
  assert BI.case("c256_l8").hp.n_channels == 256 and BI.case("c256_l8").L == 413
  assert synthetic.flow_channels(BI.case("c2").hp) == [8, 6, 4, 2]
  for name in BI.CASES:
    c = BI.case(name)
    for scale, n in ((c.scale_fwd, c.n_fwd), (c.scale_inv, c.n_inv)):
      assert math.log2(scale).is_integer() and 2 ** -0.5 <= scale / n <= 2 ** 0.5      # the power of two next to N
    rms = lambda t: t.flatten(1).pow(2).mean(1).sqrt()
    for t in [c.wav, c.r_z, c.z_init, c.r_audio] + c.r_ls + list(c.z_early.values()):
      r = rms(t)
      quiet = torch.cat([r[:BI.LOUD_ROW], r[BI.LOUD_ROW + 1:]])
      assert float((r[BI.LOUD_ROW] / quiet).min()) > 0.8 * BI.LOUD and float((r[BI.LOUD_ROW] / quiet).max()) < 1.25 * BI.LOUD
    for t in (c.mel, c.wav, c.z_init, c.r_z, c.r_audio):
      for b in range(1, c.B):
        assert not torch.equal(t[b] / t[b].abs().max(), t[0] / t[0].abs().max())       # no row is a scaled copy


@pytest.mark.parametrize("direction", BI.DIRECTIONS)
def test_unfaulted_oracle_meets_the_contract(direction, clean):
  """fp64: every row of every value and input gradient equals its batch-of-one call to rounding, every parameter gradient
  is the sum of the single calls', log_det_W adds up."""
  c = BI.case(NAME)
  batch, singles = clean[direction]
  diffs = BI.row_differences(batch, singles)
  assert len(diffs) == (7 if direction == "fwd" else 4)
  for q, d in diffs.items():
    print(f"{NAME}/{direction} fp64: {q}: worst row difference {max(d):.2e}")
    assert max(d) <= BI.ROW_TOL_64, (q, d)
  worst = BI.worst_ratio(BI.additive_errors(batch, singles, c.hp))
  print(f"{NAME}/{direction} fp64: worst additive ratio {worst[0]:.2e} ({worst[1]})")
  assert worst[0] <= BI.ROW_TOL_64
  if direction == "fwd":
    BI.check_logdet(batch, singles, NAME)


@pytest.mark.parametrize("name,direction", SETS)
def test_float32_reorder_ratios_still_hold(name, direction):
  """The constants the GPU bound is made of, measured again on the float32 oracle.  Thread count and blocking change the
  accumulation order, so two hosts do not measure the same figure: the recorded one must be within a factor of two above
  and four below a fresh one -- then the GPU bound (4 x recorded) is at least twice and at most sixteen times what the
  reference does to itself here -- and the bound must stay below GRAD_TOL / 50."""
  fresh, q = BI.measure_f32(name, direction)
  rec = BI.F32_RATIO[(name, direction)]
  print(f"{name}/{direction}: float32 reorder ratio {fresh:.3e} ({q}), recorded {rec:.3e}, GPU bound {BI.bound(name, direction):.3e}")
  assert fresh <= 2.0 * rec and rec <= 4.0 * fresh
  assert 0.0 < BI.bound(name, direction) <= BI.BOUND_LIMIT


@pytest.mark.parametrize("direction", BI.DIRECTIONS)
def test_planted_leak_breaks_the_contract_and_hides_from_grad_tol(direction, clean):
  c = BI.case(NAME)
  batch, singles = clean[direction]
  # a call on one utterance has no neighbour: the fault changes nothing there, the clean singles serve every fault
  one = BI.oracle(c, direction, 0, fault=MAIN)
  for q, t in one.items():
    assert float((t - singles[0][q]).norm()) <= BI.ROW_TOL_64 * float(singles[0][q].norm()), q
  value = "z" if direction == "fwd" else "audio"
  grads = [q for q in batch if q.startswith("p/") or q.startswith("d ")]
  rel = BI.bound(NAME, direction)
  for fault in FAULTS:
    leaky = BI.oracle(c, direction, fault=fault)
    what = f"{NAME}/{direction} {fault}"
    # (2) batch against singles
    diffs = BI.row_differences(leaky, singles)
    # Values: utterance b reads b + 1, the last one keeps its zeros and its values.  Gradients: the backward of that read
    # hands utterance b's gradient to the columns of b + 1 it read, so the last utterance's input gradients move as well
    # (and the first one's through its changed forward): no row of an input gradient is spared.
    for q, d in diffs.items():
      if not q.startswith("d "):
        assert d[c.B - 1] <= BI.ROW_TOL_64, (what, q, d)
    row_factor = min(max(d[b] for d in diffs.values()) for b in range(c.B - 1)) / BI.ROW_TOL_64
    for q in (value, "d mel"):
      print(f"{what}: {q}: row differences " + " ".join(f"{v:.2e}" for v in diffs[q]))
      assert min(diffs[q][:c.B - (0 if q == "d mel" else 1)]) >= WIDE * BI.ROW_TOL_64, (what, q, diffs[q])
    errs = BI.additive_errors(leaky, singles, c.hp)
    n_over = sum(1 for e, n in errs.values() if e > rel * n + BI.FLOOR)
    worst, wq = BI.worst_ratio(errs)
    print(f"{what}: leaking rows differ from their single calls by at least {row_factor:.1e} x the fp64 equality bound "
          f"(on the GPU the bound is 0: {min(diffs[value][:c.B - 1]) * 2 ** 24:.0f} fp32 ulps); {n_over} of {len(errs)} parameter "
          f"gradients beyond the additive bound {rel:.2e}, worst {worst:.2e} = {worst / rel:.0f} x the bound ({wq})")
    assert row_factor >= WIDE and worst >= WIDE * rel and n_over >= 1
    with pytest.raises(AssertionError, match="differs from the batch-of-one calls"):      # the GPU tests' own comparison
      BI.compare(leaky, singles, c, direction, what)
    with pytest.raises(AssertionError, match="not the sum of the single calls"):           # ... and its additive half alone
      BI.compare({q: t for q, t in leaky.items() if q.startswith("p/")}, singles, c, direction, what)
    # (3) what a GRAD_TOL comparison against the unfaulted oracle sees of the same fault
    seen = [q for q in grads
            if float((leaky[q] - batch[q]).norm()) > GRAD_TOL * float(batch[q].norm()) + BI.FLOOR]
    moved = max(float((leaky[q] - batch[q]).norm()) / max(float(batch[q].norm()), 1e-300) for q in grads)
    v_rms = float((leaky[value] - batch[value]).pow(2).mean().sqrt())
    print(f"{what}: {len(seen)} of {len(grads)} gradient tensors beyond GRAD_TOL against the unfaulted oracle "
          f"(worst {moved:.2e}); {value} moved by {v_rms:.2e} rms")
    if fault == MAIN:
      assert len(seen) <= len(grads) // 20, seen
