"""CPU: the depth / flow-layout corners (tests/_corners.py) -- the oracle pinned to the reference's own outputs and
gradients (tests/golden/flow_corners.npz, make_golden_corners.py), with the bounds of test_oracle_golden.py and
test_oracle_input_grads.py, and the host bookkeeping of every layout."""
import ast
import ctypes as C

import numpy as np
import pytest
import torch

import _corners as K
from _corners import Corner
from oracle import torch_oracle as O
from test_infer_grads_cpu import early_channel_map
from test_oracle_input_grads import ORACLE_TOL, input_grads_ref
from waveglow_amd import _lib, build, synthetic
from waveglow_amd.model import WaveGlow

# id: (flow widths c_k, early-output flows, {flow: channel offset in forward's z}, early channels in all)
EXPECTED = {
  "l1": ([8, 8, 6, 6], [2], {2: 0}, 2),
  "l1_c128": ([8, 6], [1], {1: 0}, 2),
  "l1_c256": ([8, 6], [1], {1: 0}, 2),
  "l1_c512": ([8, 6], [1], {1: 0}, 2),
  "f1": ([8], [], {}, 0),
  "l1f1": ([8], [], {}, 0),
  "e4": ([8, 4], [1], {1: 0}, 4),
  "e6": ([8, 2], [1], {1: 0}, 6),
  "c2": ([8, 6, 4, 2], [1, 2, 3], {1: 0, 2: 2, 3: 4}, 6),
  "ee3": ([8, 8, 8, 6, 6], [3], {3: 0}, 2),
  "e0": ([8, 8, 8], [1, 2], {1: 0, 2: 0}, 0),
}


def test_every_layout_is_in_the_fixture_and_the_table():
  assert list(EXPECTED) == K.IDS
  fx = K.fixture()
  for name in K.IDS:
    assert f"{name}/audio" in fx.files and f"{name}/grad_norm" in fx.files, name
    assert dict(ast.literal_eval(str(fx[f"{name}/hp_json"]))) == K.LAYOUTS[name]
  for name in K.NORMED_AUDIO_IDS:
    assert f"{name}/audio_from_weightnorm_ckpt" in fx.files


@pytest.mark.parametrize("name", K.IDS)
def test_weight_generator_is_stable(name):
  c = Corner(name)
  assert K.weights_crc(c.sd) == int(c.get("weights_crc32"))


@pytest.mark.parametrize("name", K.IDS)
def test_infer_matches_reference_bitwise(name):
  c = Corner(name)
  with torch.no_grad():
    audio = O.infer_ref(c.sd, c.mel, c.z_init, c.z_early, c.sigma, c.oracle_cfg())
  assert audio.shape == c.audio.shape == (K.B, 256 * K.T)
  assert torch.equal(audio, c.audio), float((audio - c.audio).abs().max())
  if name in K.NORMED_AUDIO_IDS:
    # the reference through its own fold differs from the dense-weight run only by fold rounding (test_oracle_golden.py)
    ref = torch.from_numpy(c.get("audio_from_weightnorm_ckpt"))
    assert float((ref - c.audio).abs().max()) < 5e-4


@pytest.mark.parametrize("name", K.IDS)
def test_forward_and_loss_match_reference_bitwise(name):
  c = Corner(name)
  widths = EXPECTED[name][0]
  with torch.no_grad():
    z, log_s, log_det = O.forward_ref(c.sd, c.mel, c.wav, c.oracle_cfg())
    loss = O.loss_ref(z, log_s, log_det, sigma=1.0)
  L = c.wav.shape[1] // 8
  assert z.shape == (K.B, 8, L) and len(log_s) == len(widths)
  assert torch.equal(z, torch.from_numpy(c.get("fwd_z")))
  for k, ls in enumerate(log_s):
    assert ls.shape == (K.B, widths[k] // 2, L), k
    assert torch.equal(ls, torch.from_numpy(c.get(f"fwd_log_s_{k}"))), k
  np.testing.assert_array_equal(np.array([float(x) for x in log_det], dtype=np.float32), c.get("fwd_log_det"))
  assert np.float32(float(loss)) == c.get("fwd_loss")


@pytest.mark.parametrize("name", K.IDS)
def test_training_gradients_match_reference(name):
  """Loss, every parameter gradient (norm and first 8 values, the bounds of test_oracle_golden.py) and the full input
  gradients (ORACLE_TOL of test_oracle_input_grads.py) of the reference's own backward; and the weight seed's criterion."""
  c = Corner(name)
  sdn = c.sd_normed()
  loss, grads = O.grads_ref(sdn, c.mel, c.wav, c.oracle_cfg(), 1.0)
  ref = c.grad_summary()
  assert abs(float(loss) - float(c.get("loss"))) <= 1e-7
  assert list(grads) == list(sdn) and set(grads) == set(ref)
  for pname, g in grads.items():
    norm, head = ref[pname]
    assert abs(float(g.norm()) - norm) <= 2e-5 * max(1.0, norm), pname
    n = min(8, g.numel())
    np.testing.assert_allclose(g.flatten()[:n].numpy(), head[:n].numpy(), rtol=2e-4, atol=1e-7, err_msg=pname)
  assert K.seed_is_good(c.hp, grads), "a gradient's norm is below MIN_GRAD_NORM: take the next weight seed"
  assert c.wseed == K.FIRST_SEED[name] or not K.seed_is_good(
      c.hp, O.grads_ref(synthetic.to_weightnorm_form(synthetic.make_state_dict(c.hp, seed=c.wseed - 1)), c.mel, c.wav,
                        c.oracle_cfg(), 1.0)[1])
  for pname, g in grads.items():
    if K.structurally_zero(c.hp, pname):
      assert float(g.norm()) <= 1e-9, pname       # d v of a one-column weight-normed conv: rounding only
  loss2, g_mel, g_audio = input_grads_ref(sdn, c.mel, c.wav, c.oracle_cfg())
  assert np.float32(loss2) == c.get("loss")
  for g, key in ((g_mel, "mel_grad"), (g_audio, "audio_grad")):
    r = torch.from_numpy(c.get(key))
    assert g.shape == r.shape
    err = float((g - r).norm()) / float(r.norm())
    print(f"{name} {key}: rel {err:.3e}")
    assert err <= ORACLE_TOL, key


@pytest.mark.parametrize("name", K.IDS)
def test_host_bookkeeping(name):
  """flow_channels of the module, the weight generator and the oracle; n_early_flows; the channel map of the early outputs
  (checked against what forward(infer(z)) returns); the noise shapes _draw_noise makes; the library's expected tensors."""
  c = Corner(name)
  hp, cfg = c.hp, c.oracle_cfg()
  widths, early, cmap, n_e = EXPECTED[name]
  model = WaveGlow(hp)
  assert model.flow_channels() == widths == synthetic.flow_channels(hp) == cfg.flow_channels()
  assert model.n_early_flows() == len(early) and cfg.early_flows() == early == K.early_flows(hp)
  assert model.n_remaining_channels == widths[-1] == hp.n_group - n_e
  assert early_channel_map(cfg) == (cmap, n_e)
  assert [m.conv.weight.shape[0] for m in model.convinv] == widths
  assert [w.start.weight.shape[1] for w in model.WN] == [x // 2 for x in widths]
  assert [w.end.weight.shape[0] for w in model.WN] == widths
  assert set(c.z_early) == set(early) and c.z_init.shape == (K.B, widths[-1], 32 * K.T)
  # P of the inverse identity (tests/test_infer_grads_cpu.py): forward(infer(z)) = sigma * [early outputs..., z_init]
  with torch.no_grad():
    z, _, _ = O.forward_ref(c.sd, c.mel, c.audio, cfg)
  want = torch.zeros_like(z)
  for k, off in cmap.items():
    want[:, off:off + hp.n_early_size] = c.sigma * c.z_early[k]
  want[:, n_e:] = c.sigma * c.z_init
  assert float((z - want).norm() / want.norm()) <= 1e-4
  # the draws of infer: [B, n_rem, L], then one [B, n_early_size, L] per early flow
  for T in (1, 7):
    zi, ze = model._draw_noise(torch.zeros(3, hp.n_mel_channels, T))
    assert zi.shape == (3, widths[-1], 32 * T) and [tuple(t.shape) for t in ze] == [(3, hp.n_early_size, 32 * T)] * len(early)
  given = [torch.ones(3, hp.n_early_size, 32) for _ in early]
  zi, ze = model._draw_noise(torch.zeros(3, hp.n_mel_channels, 1), None, given)
  assert ze is given and zi.shape == (3, widths[-1], 32)
  # the library's view: one expected tensor per dense state_dict key, in dense_state() order
  build.build_library()
  lib = _lib.load()
  h = C.c_void_p()
  wcfg = _lib.WgConfig(hp.n_mel_channels, hp.n_flows, hp.n_group, hp.n_early_every, hp.n_early_size, hp.n_layers,
                       hp.n_channels, hp.kernel_size, 1024, 256)
  rc = lib.wg_create(C.byref(wcfg), 0, C.byref(h))
  if name == "e0":
    # zero-channel early outputs are outside the envelope: refused by the library and by the Python layer
    assert rc == -1 and b"n_early_size" in lib.wg_last_error()
    with pytest.raises(_lib.WgError, match="n_early_size"):
      model._get_engine(torch.device("cuda", 0))
    return
  assert rc == 0, lib.wg_last_error()
  names = [lib.wg_expected_tensor_name(h, i).decode() for i in range(lib.wg_num_expected_tensors(h))]
  lib.wg_destroy(h)
  dense = WaveGlow.remove_weightnorm(WaveGlow(hp)).dense_state()
  assert names == list(dense) and set(names) == set(WaveGlow.remove_weightnorm(WaveGlow(hp)).state_dict())
  assert len(names) == 2 + hp.n_flows * (7 + 4 * hp.n_layers) and set(names) == set(c.sd)
  for n in names:
    assert tuple(dense[n].shape) == tuple(c.sd[n].shape), n
