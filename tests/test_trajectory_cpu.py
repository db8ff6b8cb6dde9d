"""CPU: the K-step trajectory fixtures (tests/golden/make_golden_trajectory.py -- the reference's own training loop)
against the oracle, and the sharpness of the bounds that tests/test_gpu_trajectory.py takes from them."""
import numpy as np
import torch

from _cases import Trajectory, oracle_cfg_from_hp, sub_errors


def test_oracle_adam_trajectory_reproduces_the_reference_loop():
  """oracle.grads_ref + torch.optim.Adam, K steps on the two alternating batches, against the c64 Adam leg.  The GPU tests
  use the oracle at trained weights and grant the HIP path the fixture's yardsticks, so the oracle must sit an order of
  magnitude inside them: every loss, the global update and every tensor the fixture keeps whole to ONE TENTH of the
  yardstick (fp32 against fp64 of this loop: 1.7e-7 in the loss, 5.8e-6 in the global update)."""
  from oracle import torch_oracle as O
  tr = Trajectory("c64", "adam")
  cfg = oracle_cfg_from_hp(tr.hp)
  sd0 = tr.state_dict()
  assert sorted(sd0) == sorted(tr.names)
  theta = {k: v.clone() for k, v in sd0.items()}
  opt = torch.optim.Adam(list(theta.values()), lr=tr.lr)
  data = tr.batches()
  losses = []
  for k in range(tr.K):
    loss, grads = O.grads_ref(theta, data[k % 2][0], data[k % 2][1], cfg, 1.0)
    losses.append(float(loss))
    for name, p in theta.items():
      p.grad = grads[name]
    opt.step()
  losses.append(float(O.grads_ref(theta, data[0][0], data[0][1], cfg, 1.0)[0]))
  lerr = np.abs(np.array(losses) - tr.loss)
  print("loss error per step", " ".join(f"{e:.1e}" for e in lerr))
  delta = {k: theta[k] - sd0[k] for k in theta}
  per, glob = sub_errors(delta, tr.dsub, tr.full, tr.nmin)
  print(f"global update error {glob:.3e} (a tenth of the yardstick: {tr.yard_global_random / 10:.3e})")
  tr.check(losses, delta, "oracle")            # the GPU tests' own bounds, through the same code
  for k in range(tr.K + 1):
    assert lerr[k] <= tr.yard_loss[k] / 10, (k, lerr[k], tr.yard_loss[k])
  assert glob <= tr.yard_global_random / 10
  worst, n_full = 0.0, 0
  for name in tr.names:
    ref = tr.dfull(name)
    if ref is None:
      continue
    n_full += 1
    err = float((delta[name].flatten().double() - ref.double()).norm())
    worst = max(worst, err / max(tr.dnorm[name], 1e-30) / max(tr.yard[name], 1e-30))
    assert err <= tr.yard[name] / 10 * tr.dnorm[name], (name, err, tr.yard[name], tr.dnorm[name])
  assert n_full > 100
  print(f"{n_full} whole tensors: worst error / yardstick {worst:.2e}")


def test_bounds_cannot_hide_a_dropped_or_stale_step():
  """Fixture only.  The reference's loop with the update of step 5 dropped, and with step 5 run on step 4's weights,
  moves the loss and the global update by the recorded fault figures; the bounds of the GPU tests are at most half of
  each, so neither fault passes them.  Recorded: Adam skip 7.0e-2 / 1.2e-1, stale 7.1e-2 / 7.8e-2 (bounds 2.0e-3 /
  3.7e-2); SGD skip 2.3e-2 / 1.0e-1, stale 2.2e-2 / 2.2e-3 (bounds 2.0e-3 / 4.9e-3).
  One figure cannot be separated by any bound: SGD's update is the plain sum of the gradients, and a gradient taken one
  step early changes that sum by 2.2e-3 -- less than the 4.9e-3 of the fixed-direction yardstick, which the bound cannot
  go below.  In the SGD leg the stale step is caught by the loss (ten times its bound), and by the update in the Adam leg;
  that both hold is asserted instead."""
  for leg in ("adam", "sgd"):
    tr = Trajectory("c64", leg)
    assert set(tr.faults) == {"skip", "stale"}
    loss_bound = max(tr.loss_bound(k) for k in range(tr.K + 1))
    for fault, (f_loss, f_global) in tr.faults.items():
      print(f"{leg}/{fault}: loss bound {loss_bound:.3e} vs fault {f_loss:.3e};  "
            f"global bound {tr.global_bound():.3e} vs fault {f_global:.3e}")
      assert loss_bound <= f_loss / 2
      if (leg, fault) != ("sgd", "stale"):
        assert tr.global_bound() <= f_global / 2
    # and the yardsticks are what the generator says they are: a 5e-3 gradient error does more than nothing
    assert 0 < tr.yard_global_random and 0 < tr.yard_global_fixed and all(v > 0 for v in tr.yard.values())
