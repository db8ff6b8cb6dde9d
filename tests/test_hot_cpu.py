"""CPU: the hot-weight family (tests/_hot.py, tests/golden/hot_*.npz) -- weights at the dynamic range of a trained vocoder.

* the regime: every case really has saturated gates, ``log_s`` of several units and ill-conditioned 1x1 matrices with a
  non-zero logdet, and the fp32 oracle still agrees with the fp64 oracle there (conditions on the INPUTS of the GPU tests);
* the oracle pinned to the reference's own outputs and gradients at these weights (make_golden_hot.py);
* the gap the family closes, on record: planted faults that the cold-weight bounds of the existing suite cannot see
  and the hot bounds of tests/test_gpu_hot.py see by at least a factor of two.
"""
import ast

import numpy as np
import pytest
import torch

import _hot as H
from _cases import GRAD_TOL, oracle_cfg_from_hp
from oracle import torch_oracle as O
from waveglow_amd import synthetic
from waveglow_amd.hparams import HParams

SETS = [(n, d) for n in H.IDS for d in H.DIRECTIONS]
# two fp32 evaluations (the reference's modules, the oracle's functional form) of a function whose fp32 evaluation is within
# 1e-4 of fp64 (the regime condition below) are within 2e-4 of each other
REF_TOL = 2e-4


@pytest.fixture(scope="module")
def regimes():
  return {(n, d): H.regime(n, d, H.hot_state_dict(n, d)) for n, d in SETS}


def test_cases_and_fixture_agree():
  for name in H.IDS:
    fx = H.fixture(name)
    over, B, T, wseed, heats = H.CASES[name]
    assert dict(ast.literal_eval(str(fx["hp_json"]))) == over
    assert (int(fx["B"]), int(fx["T"]), int(fx["weight_seed"])) == (B, T, wseed)
    assert tuple(int(v) for v in fx["yard_draws"]) == H.YARD_SEEDS
    # L = 160 ... 192 columns: one full 128-column tile and an edge, or three 64-column tiles
    assert T in (5, 6)
  hp = HParams(**H.CASES["hot_f2e"][0])
  assert synthetic.flow_channels(hp) == [8, 6]                      # a 1x1 step below 8 channels
  assert synthetic.flow_channels(HParams(**H.CASES["hot_f6"][0])) == [8, 8, 6, 6, 4, 4]


@pytest.mark.parametrize("name,direction", SETS)
def test_weights_regenerate(name, direction):
  """hot_state_dict asserts the crc; the multipliers and the calibrated tensors are really in it."""
  c = H.Hot(name, direction)
  cold = synthetic.make_state_dict(c.hp, seed=c.wseed)
  s_end, _, gate = c.heat
  assert torch.equal(c.sd["WN.0.end.weight"], cold["WN.0.end.weight"] * s_end)
  assert torch.equal(c.sd["WN.0.in_layers.0.weight"], cold["WN.0.in_layers.0.weight"] * gate)
  assert torch.equal(c.sd["WN.0.res_skip_layers.0.weight"], cold["WN.0.res_skip_layers.0.weight"])
  assert not torch.equal(c.sd["convinv.0.conv.weight"], cold["convinv.0.conv.weight"])


@pytest.mark.parametrize("name,direction", SETS)
def test_regime(name, direction, regimes):
  st = regimes[(name, direction)]
  print(name, direction, {k: (np.round(v, 2).tolist() if isinstance(v, list) else round(v, 3)) for k, v in st.items()})
  H.assert_regime(st, direction, f"{name}/{direction}")
  c = H.Hot(name, direction)
  for key, v in st.items():                                          # what the generator saw
    np.testing.assert_allclose(np.array(v), c.get(f"regime/{key}"), rtol=1e-9, err_msg=key)


def test_some_inference_case_reaches_the_unclamped_sigmoid_exponent(regimes):
  """b < -88.7: E2 = 2^(-b log2 e) overflows to inf in inference (kernels.hip: gate_act), 1 / inf = 0."""
  lowest = {n: regimes[(n, "inv")]["b_min"] for n in H.IDS}
  print(lowest)
  assert min(lowest.values()) < -88.7


@pytest.mark.parametrize("name,direction", SETS)
def test_fp32_oracle_agrees_with_fp64_oracle(name, direction):
  worst = H.oracle_agreement(name, direction, H.hot_state_dict(name, direction))
  print(f"{name}/{direction}: worst relative L2 between the fp32 and the fp64 oracle {worst[0]:.2e} ({worst[1]})")
  assert worst[0] <= 1e-4, worst


def test_f6_yardstick_figures():
  """hot_f6 is as cool as the regime conditions allow.  Its value yardsticks are below 2 %; no heat
  that keeps log_s std >= 0.7 in all six flows brought every GRADIENT yardstick below 2 % on all three draws, which is
  recorded in DESIGN.md section 8.  What the fixture holds is pinned here so that a regenerated fixture cannot drift."""
  for direction, group in (("fwd", "train"), ("inv", "infer"), ("inv", "synth")):
    y = H.Hot("hot_f6", direction).yard(group)
    values = {q: v for q, v in y.items() if not (q.startswith("p/") or q.startswith("d "))}
    grads = {q: v for q, v in y.items() if q not in values}
    print(direction, group, "values", max(values.values()), "gradients", max(grads.values()) if grads else None)
    assert max(values.values()) <= H.F6_LIMIT
    assert not grads or max(grads.values()) <= 0.05


def test_rounding_realisations_spread_with_depth():
  """The yardstick is ONE realisation (round to nearest) of the fp16 roundings per input draw.  Other realisations of the
  same roundings -- every rounded value moved by up to half an fp16 ulp first -- stay inside 3 x yardstick on the one-flow
  hot_f1 and leave it on the six-flow hot_f6: there the error of a single gradient tensor moves by up to 10 x between
  realisations (the forward error of a flow is amplified by e^{log_s} of every flow behind it).  So on hot_f6 a path
  with the documented precision and different rounding points, such as the kernels, can miss 3 x yardstick on single
  tensors without being wrong; tests/test_gpu_hot.py: KNOWN_LIMITS, DESIGN.md sections 4a and 8."""
  beyond = {}
  for name in ("hot_f1", "hot_f6"):
    c = H.Hot(name, "fwd")
    ref = H.exact("fwd", c.sdn, c.inputs, c.cfg)
    del ref["log_det"]
    gen = torch.Generator().manual_seed(0)
    beyond[name] = []
    for rep in range(3):
      got = H.emulated("fwd", c.sdn, c.inputs, c.cfg, dither=gen)
      miss = H.check(got, ref, c.yard("train"), f"{name} realisation {rep}", quiet=True, finite=False)
      print(f"{name} realisation {rep}: {len(miss)} of {len(ref)} quantities beyond 3 x yardstick; worst {miss[:2]}")
      beyond[name].append(len(miss))
  assert max(beyond["hot_f1"]) == 0
  assert max(beyond["hot_f6"]) >= 10


# ---------------------------------------------------------------- the oracle pinned to the reference at hot weights
@pytest.mark.parametrize("name", H.IDS)
def test_infer_matches_reference_bitwise(name):
  c = H.Hot(name, "inv")
  with torch.no_grad():
    audio = O.infer_ref(c.sd, c.mel, c.z_init, c.z_early, c.sigma, c.cfg)
  ref = torch.from_numpy(c.get("audio"))
  assert audio.shape == ref.shape == (c.B, 256 * c.T)
  assert torch.equal(audio, ref), float((audio - ref).abs().max())
  with torch.no_grad():
    a64 = H.infer({k: v.double() for k, v in c.sd.items()}, c.mel.double(), c.z_init.double(),
                  {k: v.double() for k, v in c.z_early.items()}, c.sigma, c.cfg)
  assert float((a64 - ref).norm() / ref.norm()) <= 1e-4             # the fp64 restatement of _hot.py is the same function
  if name == "hot_f1":
    ref_n = torch.from_numpy(c.get("audio_from_weightnorm_ckpt"))
    assert float((ref_n - ref).norm() / ref.norm()) <= REF_TOL


@pytest.mark.parametrize("name", H.IDS)
def test_forward_and_loss_match_reference_bitwise(name):
  c = H.Hot(name, "fwd")
  with torch.no_grad():
    z, log_s, log_det = O.forward_ref(c.sd, c.mel, c.wav, c.cfg)
    loss = O.loss_ref(z, log_s, log_det, sigma=1.0)
  assert torch.equal(z, torch.from_numpy(c.get("fwd_z")))
  for k, ls in enumerate(log_s):
    assert torch.equal(ls, torch.from_numpy(c.get(f"fwd_log_s_{k}"))), k
  ld = np.array([float(x) for x in log_det], dtype=np.float32)
  np.testing.assert_array_equal(ld, c.get("fwd_log_det"))
  assert float(np.abs(ld).min()) >= 0.1 * c.B * (c.wav.shape[1] // 8)   # B L logdet W: no longer zero
  assert np.float32(float(loss)) == c.get("fwd_loss")


@pytest.mark.parametrize("name", H.IDS)
def test_training_gradients_match_reference(name):
  c = H.Hot(name, "fwd")
  loss, grads = O.grads_ref(c.sdn, c.mel, c.wav, c.cfg, 1.0)
  assert abs(float(loss) - float(c.get("loss"))) <= 1e-5 * max(1.0, abs(float(c.get("loss"))))
  names = [str(n) for n in c.get("grad_names")]
  assert sorted(names) == sorted(grads)
  norm, head = c.get("grad_norm"), c.get("grad_head")
  worst = 0.0
  for i, n in enumerate(names):
    g = grads[n]
    assert abs(float(g.norm()) - norm[i]) <= REF_TOL * norm[i] + 1e-9, n
    k = min(8, g.numel())
    assert float((g.flatten()[:k] - torch.from_numpy(head[i, :k])).norm()) <= REF_TOL * norm[i] + 1e-9, n
    if f"fwd/full/{n}" in c.fx.files:
      r = torch.from_numpy(c.get(f"full/{n}"))
      rel = float((g - r).norm()) / max(float(r.norm()), 1e-30)
      worst = max(worst, rel)
      assert rel <= REF_TOL, (n, rel)
  print(f"{name}: worst whole-tensor deviation from the reference's backward {worst:.2e}")
  from test_oracle_input_grads import input_grads_ref
  _, g_mel, g_audio = input_grads_ref(c.sdn, c.mel, c.wav, c.cfg)
  for g, key in ((g_mel, "mel_grad"), (g_audio, "audio_grad")):
    r = torch.from_numpy(c.get(key))
    assert float((g - r).norm()) <= REF_TOL * float(r.norm()), key


# ---------------------------------------------------------------- planted faults: cold bounds blind, hot bounds not
FAULTS = {"winv_t": "inv", "logdet_grad": "fwd", "no_logdet": "fwd", "clamp4": "both", "clamp_b4": "both"}
COLD = ("cold", dict(n_channels=64, n_layers=4, n_flows=6, n_early_every=2), 2, 6, 5)


def _cold_errors(direction, fault):
  """Emulated-with-fault against the fp64 oracle at ordinary synthetic weights, measured as the existing tests measure."""
  name, over, B, T, wseed = COLD
  H.CASES[name] = (over, B, T, wseed, {})
  try:
    inputs = H.make_inputs(name, direction)
    r = None if direction == "fwd" else H.cotangent(name)
  finally:
    del H.CASES[name]
  hp = HParams(**over)
  sdn = synthetic.to_weightnorm_form(synthetic.make_state_dict(hp, seed=wseed))
  cfg = oracle_cfg_from_hp(hp)
  ref = H.exact(direction, sdn, inputs, cfg, r=r)
  return H.errors(H.emulated(direction, sdn, inputs, cfg, fault=fault, r=r), ref), ref


def _inside_cold_bounds(e, ref):
  """RMS_TOL / FWD_TOL / the loss bound / GRAD_TOL of test_gpu_parity.py, test_gpu_train.py, test_gpu_infer_grads.py."""
  for q, (err, den) in e.items():
    n = ref[q].numel() ** 0.5
    if q == "audio":
      assert err / n <= 1e-3, (q, err / n)
    elif q == "z" or q.startswith("log_s."):
      assert err / n <= 2e-3, (q, err / n)
    elif q == "loss":
      assert err <= 2e-3 * max(1.0, den), (q, err)
    elif q == "log_det":
      assert err <= 1e-3, (q, err)
    else:
      assert err <= GRAD_TOL * den + 1e-7, (q, err / max(den, 1e-30))


@pytest.mark.parametrize("fault", list(FAULTS))
def test_planted_fault_is_invisible_cold_and_visible_hot(fault):
  dirs = H.DIRECTIONS if FAULTS[fault] == "both" else (FAULTS[fault],)
  for d in dirs:
    e, ref = _cold_errors(d, fault)
    _inside_cold_bounds(e, ref)
    print(f"{fault} cold {d}: inside every cold bound; worst relative error "
          f"{max(err / max(den, 1e-30) for err, den in e.values()):.2e}")
  seen = []
  for name in ("hot_f1", "hot_f2e"):
    for d in dirs:
      c = H.Hot(name, d)
      r = None if d == "fwd" else H.cotangent(name)
      ref = H.exact(d, c.sdn, c.inputs, c.cfg, r=r)
      got = H.emulated(d, c.sdn, c.inputs, c.cfg, fault=fault, r=r)
      if "log_det" in ref:                                           # the emulation leaves it exact under every fault
        del ref["log_det"]
      miss = H.check(got, ref, c.yard("train" if d == "fwd" else "synth"), f"{fault} {name}/{d}",
                     factor=2.0 * H.BOUND_FACTOR, quiet=True, finite=False)
      print(f"{fault} hot {name}/{d}: {len(miss)} quantities beyond 2 x the hot bound; worst {miss[:2]}")
      seen += miss
  if fault == "clamp4":
    # tanh(4) = 0.99933: clamping the ARGUMENT at +-4 moves a saturated gate by less than the fp16 rounding of acts
    # (2^-11), so no bound built on the fp16 design can see it -- cold or hot.  On record; clamp_b4, the same clamp on
    # the sigmoid's argument (sigmoid(-4) = 0.018 where a closed gate has 0), is the gate fault that separates
    # (DESIGN.md section 4).
    assert not seen
    return
  assert seen, f"{fault}: no quantity of hot_f1 / hot_f2e exceeds twice the hot bound"
