"""GPU: the depth / flow-layout corners of the envelope (tests/_corners.py) in every direction.

``n_layers = 1`` (the first WN layer is also the last: the a0-fold first-layer kernel without a residual output, MODE 3 on
the ``d out`` plane alone, ``layer_wgrad`` with ``i == 0 == nl - 1``) at every kernel width; ``n_flows = 1`` (no early output,
no hand-over between flows); 4- and 6-channel early outputs and the flow width 2 (one coupling channel, the 2x2 device
inverse, a 2-row end conv); an ``n_early_every`` that does not divide ``n_flows``.  ``n_early_size = 0`` is refused.

Yardsticks: tests/golden/flow_corners.npz, written by the reference itself (make_golden_corners.py), and the CPU fp32 oracle,
pinned to that fixture in tests/test_flow_corners_cpu.py.  Every bound is the one the existing test of the same direction
uses, through that test's own helpers.
"""
import numpy as np
import pytest
import torch

import _corners as K
import test_gpu_infer_grads as IG
import test_gpu_infer_weight_grads as WGT
import test_gpu_recompute as RC
from _cases import oracle_cfg_from_hp, rms
from _corners import Corner
from test_gpu_input_grads import _close, _model as _ig_model, _step as _ig_step
from test_gpu_parity import RMS_TOL, ROUND_TRIP_TOL, _round_trip, build_model, gpu_infer
from test_gpu_train import GRAD_TOL, _check, _gpu_step
from test_oracle_input_grads import input_grads_ref
from waveglow_amd import synthetic
from waveglow_amd._lib import WgError
from waveglow_amd.hparams import HParams
from waveglow_amd.model import WaveGlow, WaveGlowLoss

pytestmark = pytest.mark.gpu

RUN = [n for n in K.IDS if n != "e0"]          # e0 (zero-channel early outputs): test_zero_channel_early_outputs_are_refused
WIDE = ["l1_c128", "l1_c256", "l1_c512"]


@pytest.fixture(autouse=True)
def _poisoned_gradient_buffers(monkeypatch):
  """Gradient buffers start from NaN: an entry the library never writes makes grad_finite false."""
  monkeypatch.setenv("WG_TRAIN_POISON_GRADS", "1")


def _setup(name, B, T, crop, normed=True):
  """Model state and inputs of a layout at another shape (the fixture's weight seed)."""
  c = Corner(name)
  mel, wav = K.make_inputs(c.hp, B, T, crop)
  return c, (c.sd_normed() if normed else c.sd), mel, wav


def _infer_case(c, B, T):
  mel = synthetic.make_mel(B, T, seed=T)
  z_init, z_early = synthetic.make_noise(c.hp, B, 32 * T, seed=100 + T)
  return mel, z_init, z_early


# ------------------------------------------------------------------ inference
@pytest.mark.parametrize("name", RUN)
def test_infer_fixture_fp32(name):
  c = Corner(name)
  out = gpu_infer(build_model(c.hp, c.sd), c.mel, c.z_init, c.z_early, c.sigma)
  err = rms(out - c.audio)
  print(f"{name} infer B{K.B} T{K.T} vs reference: rms err {err:.3e} (signal rms {rms(c.audio):.3f})")
  assert out.shape == c.audio.shape and torch.isfinite(out).all()
  assert err <= RMS_TOL
  if name in K.NORMED_AUDIO_IDS:
    ref = torch.from_numpy(c.get("audio_from_weightnorm_ckpt"))
    out_n = gpu_infer(build_model(c.hp, c.sd, normed=True), c.mel, c.z_init, c.z_early, c.sigma)
    print(f"{name} from the weight-normed form: rms err {rms(out_n - ref):.3e}")
    assert rms(out_n - ref) <= RMS_TOL


@pytest.mark.parametrize("name,dtype", [(n, torch.float32) for n in RUN] + [(n, torch.float16) for n in K.L1_IDS])
def test_infer_oracle(name, dtype):
  """B 3 x T 37 (L = 1184: several tiles, an edge tile), fp32 I/O; fp16 I/O against the oracle on the fp16-rounded inputs."""
  from oracle import torch_oracle as O
  c = Corner(name)
  B, T = 3, 37
  mel, z_init, z_early = _infer_case(c, B, T)
  rnd = lambda t: t.to(dtype).float()
  with torch.no_grad():
    ref = O.infer_ref(c.sd, rnd(mel), rnd(z_init), {k: rnd(v) for k, v in z_early.items()}, c.sigma, c.oracle_cfg())
  out = gpu_infer(build_model(c.hp, c.sd), mel, z_init, z_early, c.sigma, dtype)
  err = rms(out - ref)
  print(f"{name} infer B{B} T{T} {dtype} vs oracle: rms err {err:.3e} (signal rms {rms(ref):.3f})")
  assert out.shape == (B, 256 * T) and torch.isfinite(out).all()
  assert err <= RMS_TOL


# ------------------------------------------------------------------ no-grad forward
@pytest.mark.parametrize("name", RUN)
def test_forward_fixture(name):
  """As test_gpu_parity.test_forward_golden; the log_s channel counts are the layout's own (4 / 3 / 2 / 1)."""
  c = Corner(name)
  widths = synthetic.flow_channels(c.hp)
  model = build_model(c.hp, c.sd)
  with torch.no_grad():
    z, log_s, log_det = model((c.mel.cuda(), c.wav.cuda()))
  torch.cuda.synchronize()
  z_ref = torch.from_numpy(c.get("fwd_z"))
  L = c.wav.shape[1] // 8
  assert z.shape == z_ref.shape == (K.B, 8, L) and len(log_s) == len(log_det) == c.hp.n_flows
  ez = rms(z.cpu() - z_ref)
  assert ez <= 1e-3 * max(1.0, rms(z_ref)), ez
  worst = 0.0
  for k, ls in enumerate(log_s):
    ref = torch.from_numpy(c.get(f"fwd_log_s_{k}"))
    assert ls.shape == ref.shape == (K.B, widths[k] // 2, L), k
    worst = max(worst, rms(ls.cpu() - ref))
    assert rms(ls.cpu() - ref) <= 1e-3, (k, rms(ls.cpu() - ref))
  ld = np.array([float(x) for x in log_det], dtype=np.float32)
  np.testing.assert_allclose(ld, c.get("fwd_log_det"), atol=2e-3)
  ref_out = (z_ref.cuda(), [torch.from_numpy(c.get(f"fwd_log_s_{k}")).cuda() for k in range(len(log_s))],
             [torch.tensor(float(v)) for v in c.get("fwd_log_det")])
  loss_ref_inputs = float(WaveGlowLoss(1.0)(ref_out, None))
  fwd_loss = float(c.get("fwd_loss"))
  assert abs(loss_ref_inputs - fwd_loss) <= 2e-6 * max(1.0, abs(fwd_loss))
  loss_ours = float(WaveGlowLoss(1.0)((z, log_s, log_det), None))
  print(f"{name} forward: z rms err {ez:.3e}, worst log_s rms err {worst:.3e}, loss {loss_ours:.6f} vs {fwd_loss:.6f}")
  assert abs(loss_ours - fwd_loss) <= 2e-3


# ------------------------------------------------------------------ training step
def _check_summary(name, grads, c):
  """Norm and first values of every gradient against what the reference wrote down (as for cfg4_b2 in test_gpu_train.py)."""
  ref = c.grad_summary()
  assert set(ref) == set(grads)
  worst = (0.0, "")
  for pname, (ref_norm, head) in ref.items():
    g = grads[pname]
    dev = abs(float(g.norm()) - ref_norm)
    assert dev <= GRAD_TOL * ref_norm + 1e-7, pname
    n = min(8, g.numel())
    err = float((g.flatten()[:n] - head[:n]).norm())
    assert err <= GRAD_TOL * max(float(head[:n].norm()), 1e-3 * ref_norm) + 1e-7, pname
    worst = max(worst, (dev / max(ref_norm, 1e-12), pname))
  print(f"{name}: {len(ref)} gradients vs the reference's summary: worst norm deviation {worst[0]:.2e} ({worst[1]})")


@pytest.mark.parametrize("name", RUN)
def test_train_step_fixture(name):
  """The fixture's step (B 2, T 6, weight-normed): loss and every parameter gradient against the reference's own backward,
  and in full against the oracle (pinned to the same fixture on the CPU)."""
  from oracle import torch_oracle as O
  c = Corner(name)
  sdn = c.sd_normed()
  loss, y, grads = _gpu_step(c.hp, sdn, c.mel, c.wav)
  ref_loss = float(c.get("loss"))
  print(f"{name}: loss gpu {loss:.6f} reference {ref_loss:.6f}")
  assert abs(loss - ref_loss) <= 2e-3 * max(1.0, abs(ref_loss))
  widths = synthetic.flow_channels(c.hp)
  assert [tuple(t.shape) for t in y[1]] == [(K.B, w // 2, c.wav.shape[1] // 8) for w in widths]
  _check_summary(name, grads, c)
  _, g_ref = O.grads_ref(sdn, c.mel, c.wav, c.oracle_cfg(), 1.0)
  assert K.seed_is_good(c.hp, g_ref)
  _check(grads, g_ref, name)


@pytest.mark.parametrize("name,normed", [(n, True) for n in RUN] + [("l1", False), ("e6", False)])
def test_train_step_oracle(name, normed):
  """B 2, T 9, 40 samples cropped (L = 283, not a multiple of anything); dense weights after remove_weightnorm on l1, e6."""
  from oracle import torch_oracle as O
  c, sd, mel, wav = _setup(name, 2, 9, 40, normed)
  loss_ref, g_ref = O.grads_ref(sd, mel, wav, c.oracle_cfg(), 1.0)
  # the weight seed's criterion (tests/_corners.py), from the oracle alone, at this shape too
  assert K.seed_is_good(c.hp, g_ref), sorted((float(g.norm()), n) for n, g in g_ref.items())[:3]
  if normed:
    loss, _, grads = _gpu_step(c.hp, sd, mel, wav)
  else:
    model = WaveGlow.remove_weightnorm(WaveGlow(c.hp))
    model.load_state_dict(sd)
    model = model.to("cuda:0").train()
    lt = WaveGlowLoss(1.0)(model((mel.cuda(), wav.cuda())), None)
    lt.backward()
    torch.cuda.synchronize()
    assert bool(model.grad_finite)
    loss, grads = float(lt.detach()), {n: p.grad.detach().float().cpu() for n, p in model.named_parameters()}
  print(f"{name} normed={normed}: loss gpu {loss:.6f} oracle {float(loss_ref):.6f}")
  assert abs(loss - float(loss_ref)) <= 2e-3 * max(1.0, abs(float(loss_ref)))
  _check(grads, g_ref, f"{name} normed={normed}")


@pytest.mark.parametrize("name", RUN)
def test_input_grads(name):
  """mel.grad / audio.grad against the reference's own backward and the oracle, trainable and frozen (bit-identical)."""
  c = Corner(name)
  sdn = c.sd_normed()
  model = _ig_model(c.hp, sdn)
  loss, g_mel, g_audio, pg = _ig_step(model, c.mel, c.wav)
  assert abs(loss - float(c.get("loss"))) <= 2e-3 * max(1.0, abs(float(c.get("loss"))))
  _close(g_mel, torch.from_numpy(c.get("mel_grad")), f"{name} d mel vs reference")
  _close(g_audio, torch.from_numpy(c.get("audio_grad")), f"{name} d audio vs reference")
  _, o_mel, o_audio = input_grads_ref(sdn, c.mel, c.wav, c.oracle_cfg())
  _close(g_mel, o_mel, f"{name} d mel vs oracle")
  _close(g_audio, o_audio, f"{name} d audio vs oracle")
  assert g_mel.shape == c.mel.shape and g_audio.shape == c.wav.shape
  _, f_mel, f_audio, fpg = _ig_step(_ig_model(c.hp, sdn, frozen=True), c.mel, c.wav)
  assert torch.equal(f_mel, g_mel) and torch.equal(f_audio, g_audio)
  assert all(g is None for g in fpg.values()) and all(g is not None for g in pg.values())


# ------------------------------------------------------------------ gradients through synthesis
def _r(c):
  return torch.randn(c.audio.shape, generator=torch.Generator().manual_seed(11)) / c.audio.numel()


@pytest.mark.parametrize("name", RUN)
def test_infer_differentiable_frozen(name):
  """d mel, d z_init and every d z_early (each with the layout's own channel count) against autograd through infer_ref."""
  c = Corner(name)
  model = IG._frozen(c.hp, c.sd)
  r = _r(c)
  o_mel, o_zi, o_ze = IG._oracle_grads(c, r)
  mel, zi, ze = IG._inputs(c)
  assert len(ze) == len(K.early_flows(c.hp)) and all(z.shape == (K.B, c.hp.n_early_size, 32 * K.T) for z in ze)
  audio = model.infer_differentiable(mel, c.sigma, z_init=zi, z_early=ze)
  (audio * r.cuda()).sum().backward()
  torch.cuda.synchronize()
  assert bool(model.grad_finite)
  assert rms(audio.detach().cpu() - c.audio) <= RMS_TOL
  for what, g, ref in [("d mel", mel.grad, o_mel), ("d z_init", zi.grad, o_zi)] + \
                      [(f"d z_early[{i}]", z.grad, o) for i, (z, o) in enumerate(zip(ze, o_ze))]:
    assert g is not None and g.shape == ref.shape, what
    e = IG._rel(g.cpu(), ref)
    print(f"{name} {what} {tuple(g.shape)}: rel {e:.3e}")
    assert e <= GRAD_TOL, what
  assert all(p.grad is None for p in model.parameters())


@pytest.mark.parametrize("name", RUN)
def test_infer_differentiable_weight_grads(name):
  """weight_grads=True on the weight-normed model: every parameter gradient against autograd through infer_ref; the audio
  and the input gradients bit-identical to the frozen call's."""
  c = Corner(name)
  r = _r(c)
  o_par, o_mel, o_zi, o_ze = WGT._oracle_grads(c, True, r)
  audio, grads, g_mel, g_zi, g_ze, model = WGT._run(c, True, r)
  assert set(grads) == set(o_par) and len(grads) == len(list(model.parameters()))
  for pname, ref in o_par.items():
    assert grads[pname] is not None and grads[pname].shape == ref.shape, pname
  small = min((float(g.norm()), n) for n, g in o_par.items() if not K.structurally_zero(c.hp, n))
  print(f"{name}: smallest oracle gradient norm {small[0]:.3e} ({small[1]})")
  _check({n: g.float().cpu() for n, g in grads.items()}, o_par, f"{name} synthesis")
  for what, g, ref in [("d mel", g_mel, o_mel), ("d z_init", g_zi, o_zi)] + \
                      [(f"d z_early[{i}]", z, o) for i, (z, o) in enumerate(zip(g_ze, o_ze))]:
    assert g is not None and g.shape == ref.shape, what
    e = WGT._rel(g.cpu(), ref)
    print(f"{name} {what}: rel {e:.3e}")
    assert e <= GRAD_TOL, what
  frozen = WGT._model(c.hp, c.sd, True, trainable=False)
  mel, zi, ze = WGT._inputs(c)
  a_frozen = frozen.infer_differentiable(mel, c.sigma, z_init=zi, z_early=ze)
  (a_frozen * r.cuda()).sum().backward()
  torch.cuda.synchronize()
  assert torch.equal(audio, a_frozen.detach())
  assert torch.equal(mel.grad, g_mel) and torch.equal(zi.grad, g_zi)
  assert all(torch.equal(z.grad, g) for z, g in zip(ze, g_ze))


# ------------------------------------------------------------------ n_layers = 1: every launch variant
@pytest.mark.parametrize("name", WIDE)
def test_one_layer_both_tile_widths(name, monkeypatch):
  """WG_FORCE_BN 128 and 64: inference bit-identical between the two (as test_layer_tile_widths_agree_c256) and within the
  bar of the oracle; the training step against the oracle under each."""
  from oracle import torch_oracle as O
  c = Corner(name)
  B, T = 3, 37
  mel, z_init, z_early = _infer_case(c, B, T)
  with torch.no_grad():
    ref = O.infer_ref(c.sd, mel, z_init, z_early, c.sigma, c.oracle_cfg())
  _, sdn, tmel, twav = _setup(name, 2, 9, 40)
  loss_ref, g_ref = O.grads_ref(sdn, tmel, twav, c.oracle_cfg(), 1.0)
  outs = {}
  for bn in ("128", "64"):
    monkeypatch.setenv("WG_FORCE_BN", bn)
    outs[bn] = gpu_infer(build_model(c.hp, c.sd), mel, z_init, z_early, c.sigma)
    print(f"{name} bn{bn}: infer rms err {rms(outs[bn] - ref):.3e}")
    assert rms(outs[bn] - ref) <= RMS_TOL
    loss, _, grads = _gpu_step(c.hp, sdn, tmel, twav)
    assert abs(loss - float(loss_ref)) <= 2e-3 * max(1.0, abs(float(loss_ref)))
    _check(grads, g_ref, f"{name} bn{bn}")
  assert torch.equal(outs["128"], outs["64"]), float((outs["128"] - outs["64"]).abs().max())


@pytest.mark.parametrize("B,T", [(1, 40), (2, 37)])
def test_one_layer_deep_prefetch_equals_one_step_ring(B, T, monkeypatch):
  """l1_c256: the deep-prefetch variant of the first-layer / no-residual kernel against WG_DISABLE_DEEP=1, bit for bit."""
  c = Corner("l1_c256")
  model = build_model(c.hp, c.sd)
  mel, z_init, z_early = _infer_case(c, B, T)
  ze = [z_early[k].cuda() for k in sorted(z_early, reverse=True)]
  with torch.no_grad():
    monkeypatch.delenv("WG_DISABLE_DEEP", raising=False)
    deep = model.infer_with_noise(mel.cuda(), z_init.cuda(), ze, c.sigma)
    monkeypatch.setenv("WG_DISABLE_DEEP", "1")
    ring = model.infer_with_noise(mel.cuda(), z_init.cuda(), ze, c.sigma)
  torch.cuda.synchronize()
  assert torch.isfinite(deep).all() and float(deep.abs().max()) > 1e-3
  assert torch.equal(deep, ring), float((deep - ring).abs().max())


def test_one_layer_start_fold_and_stored_x0_agree(monkeypatch):
  """l1_c256 with and without the start fold (WG_NO_START_FOLD=1): both within the bar, and within half of it of each other."""
  from oracle import torch_oracle as O
  c = Corner("l1_c256")
  mel, z_init, z_early = _infer_case(c, 2, 37)
  with torch.no_grad():
    ref = O.infer_ref(c.sd, mel, z_init, z_early, c.sigma, c.oracle_cfg())
  out_fold = gpu_infer(build_model(c.hp, c.sd), mel, z_init, z_early, c.sigma)
  monkeypatch.setenv("WG_NO_START_FOLD", "1")
  out_x0 = gpu_infer(build_model(c.hp, c.sd), mel, z_init, z_early, c.sigma)
  monkeypatch.delenv("WG_NO_START_FOLD")
  e_fold, e_x0, d = rms(out_fold - ref), rms(out_x0 - ref), rms(out_fold - out_x0)
  print(f"l1_c256 fold {e_fold:.3e} stored x0 {e_x0:.3e} between them {d:.3e}")
  assert e_fold <= RMS_TOL and e_x0 <= RMS_TOL
  assert d <= 0.5 * RMS_TOL


@pytest.mark.parametrize("dtype", [torch.float32, torch.float16])
def test_one_layer_round_trip_full_size(dtype):
  """forward(infer(z)) = the injected noise at HParams(n_layers=1), B 16 x T 864: the two-tiles-per-workgroup launch of the
  fold / no-residual kernel (an eighth of the layers of test_flow_round_trip_full_size)."""
  hp = HParams(n_layers=1)
  model = build_model(hp, synthetic.make_state_dict(hp, seed=0))
  err = _round_trip(model, 16, 864, 0.6, dtype)
  print(f"n_layers=1 round trip {dtype}: rms err {err:.3e}")
  assert err <= ROUND_TRIP_TOL[dtype]


# ------------------------------------------------------------------ ragged inference
@pytest.mark.parametrize("name", ["l1_c256", "e6"])
def test_ragged_batch_equals_batch_of_one_calls(name):
  c = Corner(name)
  hp = c.hp
  model = build_model(hp, c.sd)
  lens = [37, 5, 64, 21]
  Tm, B = max(lens), len(lens)
  mel = torch.full((B, 80, Tm), -11.5)
  zi0, ze0 = synthetic.make_noise(hp, 1, 32)
  z_init = torch.zeros(B, zi0.shape[1], 32 * Tm)
  z_e = {k: torch.zeros(B, v.shape[1], 32 * Tm) for k, v in ze0.items()}
  assert all(v.shape[1] == hp.n_early_size for v in z_e.values())
  singles = []
  for b, T in enumerate(lens):
    m1 = synthetic.make_mel(1, T, seed=40 + b)
    zi, ze = synthetic.make_noise(hp, 1, 32 * T, seed=70 + b)
    mel[b, :, :T] = m1[0]
    z_init[b, :, :32 * T] = zi[0]
    for k in z_e:
      z_e[k][b, :, :32 * T] = ze[k][0]
    singles.append(gpu_infer(model, m1, zi, ze, 0.8))
    mel[b, :, T:] = 3.0                      # garbage behind the utterance must not matter
    z_init[b, :, 32 * T:] = 7.0
  dev = torch.device("cuda:0")
  with torch.no_grad():
    out = model.infer_with_noise(mel.to(dev), z_init.to(dev), [z_e[k].to(dev) for k in sorted(z_e, reverse=True)], 0.8,
                                 frames=torch.tensor(lens, dtype=torch.int32))
  torch.cuda.synchronize()
  out = out.cpu()
  for b, T in enumerate(lens):
    assert torch.equal(out[b, :256 * T], singles[b][0]), b
    if T < Tm:
      assert float(out[b, 256 * T:].abs().max()) == 0.0, b


# ------------------------------------------------------------------ recompute
@pytest.mark.parametrize("name", ["f1", "l1f1", "l1", "e6"])
def test_recompute_equals_full_save(name):
  """The recompute mode keeps two flows: with one flow, with one layer, and with a 6-channel peel -- the training step and
  infer_differentiable, by the rules of test_gpu_recompute.py.  At these depths the
  mode saves no memory (the two slots hold every flow, or one layer's planes weigh less than the fp32 d spect accumulator);
  it runs all the same, without a replay where there are at most two flows."""
  c, sdn, mel, wav = _setup(name, 2, 7, 24)
  out_f, g_f = RC._train_step(c.hp, sdn, mel, wav, False)
  out_r, g_r = RC._train_step(c.hp, sdn, mel, wav, True)
  RC._check_modes(out_r, g_r, out_f, g_f, name)
  res = {rc: RC._synthesis(c.hp, sdn, mel, rc) for rc in (False, True)}
  RC._check_synthesis(res[True], res[False], name)


# ------------------------------------------------------------------ n_early_size = 0
def test_zero_channel_early_outputs_are_refused():
  """e0: zero-channel early tensors are outside the envelope (README).  Every direction says so before
  anything is launched, and the device is usable afterwards."""
  c = Corner("e0")
  ze = [c.z_early[k].cuda() for k in sorted(c.z_early, reverse=True)]
  assert [tuple(z.shape) for z in ze] == [(K.B, 0, 32 * K.T)] * 2
  model = build_model(c.hp, c.sd)
  with pytest.raises(WgError, match="n_early_size"):
    model.infer_with_noise(c.mel.cuda(), c.z_init.cuda(), ze, c.sigma)
  with pytest.raises(WgError, match="n_early_size"):
    model.infer(c.mel.cuda(), c.sigma)
  with pytest.raises(WgError, match="n_early_size"), torch.no_grad():
    model((c.mel.cuda(), c.wav.cuda()))
  with pytest.raises(WgError, match="n_early_size"):
    model.infer_differentiable(c.mel.cuda().requires_grad_(True), c.sigma)
  trainable = WaveGlow(c.hp)
  trainable.load_state_dict(c.sd_normed())
  trainable = trainable.to("cuda:0").train()
  with pytest.raises(WgError, match="n_early_size"):
    trainable((c.mel.cuda(), c.wav.cuda()))
  # one good call behind the refusals
  good = Corner("c2")
  out = gpu_infer(build_model(good.hp, good.sd), good.mel, good.z_init, good.z_early, good.sigma)
  assert rms(out - good.audio) <= RMS_TOL
