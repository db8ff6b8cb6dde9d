"""GPU: activation recomputation (``WaveGlow.recompute_activations``, include/waveglow_amd.h: WG_TRAIN_RECOMPUTE).

Yardstick: the default full-save mode on the same seeded inputs and weights.  The forward writes the same planes to two
flow slots, and the backward replays every other flow's forward bit for bit, so z, log_s, the audio of
``infer_differentiable`` and every gradient that does not go through d spect must be ``torch.equal`` to the default mode.
d spect is summed flow by flow in fp32 instead of in one GEMM over every layer: the gradients behind it (upsample weight
and bias, mel) agree to 1e-4 relative L2.
"""
import os
import socket

import numpy as np
import pytest
import torch

from waveglow_amd import synthetic
from waveglow_amd._lib import WgError
from waveglow_amd.hparams import HParams
from waveglow_amd.model import WaveGlow, WaveGlowLoss

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
GRAD_TOL = 5e-3          # tests/test_gpu_train.py: parity of the training direction with the reference
DSPECT_TOL = 1e-4        # relative L2 of the gradients behind d spect, recompute vs full save
UPSAMPLE = ("upsample.weight", "upsample.bias")


@pytest.fixture(autouse=True)
def _poisoned_gradient_buffers(monkeypatch):
  """Gradient buffers start from NaN: an entry the library leaves unwritten in either mode makes grad_finite false."""
  monkeypatch.setenv("WG_TRAIN_POISON_GRADS", "1")


def _setup(over, B, T, wseed, crop=96):
  hp = HParams(**over)
  sd = synthetic.to_weightnorm_form(synthetic.make_state_dict(hp, seed=wseed))
  mel = synthetic.make_mel(B, T, seed=1234 + B + T)
  g = torch.Generator().manual_seed(99 + T)
  wav = torch.rand(B, 256 * T - crop, generator=g) * 0.6 - 0.3
  return hp, sd, mel, wav


def _model(hp, sd, recompute):
  model = WaveGlow(hp)
  model.load_state_dict(sd)
  model = model.to("cuda:0").train()
  model.recompute_activations = recompute
  return model


def _train_step(hp, sd, mel, wav, recompute, model=None):
  model = model if model is not None else _model(hp, sd, recompute)
  model.zero_grad()
  y = model((mel.cuda(), wav.cuda()))
  WaveGlowLoss(1.0)(y, None).backward()
  torch.cuda.synchronize()
  assert bool(model.grad_finite), "an entry of the (NaN-poisoned) gradient buffer was left unwritten"
  out = [y[0].detach().cpu()] + [t.detach().cpu() for t in y[1]]
  grads = {n: p.grad.detach().cpu().clone() for n, p in model.named_parameters()}
  return out, grads


def _rel(a, b):
  return float((a.double() - b.double()).norm() / max(float(b.double().norm()), 1e-30))


def _check_modes(out_r, g_r, out_f, g_f, what):
  """Forward outputs and every gradient equal, except those behind d spect (the upsample) within DSPECT_TOL."""
  for i, (a, b) in enumerate(zip(out_r, out_f)):
    assert torch.equal(a, b), f"{what}: forward output {i} differs between the modes"
  for name in g_f:
    if name in UPSAMPLE:
      rel = _rel(g_r[name], g_f[name])
      print(f"{what}: {name} rel {rel:.3e}")
      assert rel <= DSPECT_TOL, f"{what}: {name}: {rel:.3e}"
    else:
      assert torch.equal(g_r[name], g_f[name]), f"{what}: {name} differs between the modes"


def test_trainable_c64_equal_to_full_save():
  """Trainable weight-normed c64 model (the c64_grads fixture's configuration): recompute equals full save."""
  over = dict(n_channels=64, n_layers=4, n_flows=6, n_early_every=2)
  hp, sd, mel, wav = _setup(over, 2, 12, 5)
  out_f, g_f = _train_step(hp, sd, mel, wav, False)
  out_r, g_r = _train_step(hp, sd, mel, wav, True)
  _check_modes(out_r, g_r, out_f, g_f, "c64")
  fx = np.load(os.path.join(HERE, "golden", "c64_grads.npz"))
  for name in UPSAMPLE:
    if f"full/{name}" in fx.files:
      ref = torch.from_numpy(fx[f"full/{name}"])
      assert float((g_r[name] - ref).norm()) <= GRAD_TOL * float(ref.norm()) + 1e-7, name
    ref_norm = float(fx[f"norm/{name}"])
    assert abs(float(g_r[name].norm()) - ref_norm) <= GRAD_TOL * ref_norm + 1e-7, name


def test_configs3_step_equal_and_memory():
  """configs[3] shapes (256 channels, batch 32 x 63 frames, 16 000 samples), synthetic weights: one training step per
  mode on separate model instances.  Same equalities; the library's workspace figure and the measured peak memory."""
  hp, sd, mel, wav = _setup(dict(), 32, 63, 7, crop=256 * 63 - 16000)
  probe = _model(hp, sd, False)
  full_b = probe.gradient_workspace_bytes(32, 63, 16000)
  rec_b = probe.gradient_workspace_bytes(32, 63, 16000, recompute=True)
  assert probe.gradient_workspace_bytes(32, 63, 16000, recompute=False) == full_b
  print(f"workspace full {full_b / 2**30:.2f} GiB recompute {rec_b / 2**30:.2f} GiB ({rec_b / full_b:.3f})")
  assert rec_b <= 0.3 * full_b
  del probe
  peaks = {}
  res = {}
  for recompute in (True, False):
    model = _model(hp, sd, recompute)
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    res[recompute] = _train_step(hp, sd, mel, wav, recompute, model)
    peaks[recompute] = torch.cuda.max_memory_allocated()
    del model
    torch.cuda.empty_cache()
  print(f"peak allocated full {peaks[False] / 2**30:.2f} GiB recompute {peaks[True] / 2**30:.2f} GiB "
        f"({peaks[True] / peaks[False]:.3f})")
  assert peaks[True] <= 0.35 * peaks[False]
  _check_modes(*res[True], *res[False], "configs[3]")


@pytest.mark.parametrize("channels,over", [
    (128, dict(n_layers=2, n_flows=4, n_early_every=1, n_early_size=2)),
    (512, dict(n_layers=8, n_flows=4, n_early_every=2)),
    (128, dict(n_layers=8, n_flows=5, n_early_every=2)),
])
def test_other_widths_and_flow_layouts(channels, over):
  """128 / 512 channels, 2 / 8 layers, early outputs every flow (h_k = 4, 3, 2, 1) or every two, an odd flow count:
  the training step and infer_differentiable in both modes."""
  hp, sd, mel, wav = _setup(dict(over, n_channels=channels), 2, 7, 13, crop=24)
  out_f, g_f = _train_step(hp, sd, mel, wav, False)
  out_r, g_r = _train_step(hp, sd, mel, wav, True)
  _check_modes(out_r, g_r, out_f, g_f, f"c{channels} {over}")
  res = {rc: _synthesis(hp, sd, mel, rc) for rc in (False, True)}
  _check_synthesis(res[True], res[False], f"c{channels} {over}")


def test_frozen_likelihood_loss_input_gradients():
  """A frozen model as a likelihood loss: audio.grad equal, mel.grad (through d spect) within 1e-4."""
  hp, sd, mel, wav = _setup(dict(), 2, 9, 3, crop=40)
  grads = {}
  for recompute in (False, True):
    model = _model(hp, sd, recompute).requires_grad_(False)
    m, a = mel.cuda().requires_grad_(True), wav.cuda().requires_grad_(True)
    y = model((m, a))
    WaveGlowLoss(1.0)(y, None).backward()
    torch.cuda.synchronize()
    assert bool(model.grad_finite)
    grads[recompute] = (y[0].detach().cpu(), m.grad.cpu(), a.grad.cpu())
  assert torch.equal(grads[True][0], grads[False][0])
  assert torch.equal(grads[True][2], grads[False][2]), "audio.grad differs between the modes"
  rel = _rel(grads[True][1], grads[False][1])
  print(f"mel.grad rel {rel:.3e}")
  assert rel <= DSPECT_TOL


def _synthesis(hp, sd, mel, recompute):
  model = _model(hp, sd, recompute).eval().requires_grad_(False)
  B, _, T = mel.shape
  L = 256 * T // hp.n_group
  g = torch.Generator().manual_seed(7 + T)
  m = mel.cuda().requires_grad_(True)
  zi = torch.randn(B, model.n_remaining_channels, L, generator=g).cuda().requires_grad_(True)
  n_early = sum(1 for k in range(hp.n_flows) if k % hp.n_early_every == 0 and k > 0)
  ze = [torch.randn(B, hp.n_early_size, L, generator=g).cuda().requires_grad_(True) for _ in range(n_early)]
  audio = model.infer_differentiable(m, 0.8, z_init=zi, z_early=ze)
  w = torch.linspace(-1.0, 1.0, audio.shape[1], device=audio.device)
  (audio * w).mean().backward()
  torch.cuda.synchronize()
  assert bool(model.grad_finite)
  return audio.detach().cpu(), m.grad.cpu(), zi.grad.cpu(), [z.grad.cpu() for z in ze]


def _check_synthesis(r, f, what):
  assert torch.equal(r[0], f[0]), f"{what}: audio differs between the modes"
  assert torch.equal(r[2], f[2]), f"{what}: z_init.grad differs"
  for i, (a, b) in enumerate(zip(r[3], f[3])):
    assert torch.equal(a, b), f"{what}: z_early[{i}].grad differs"
  rel = _rel(r[1], f[1])
  print(f"{what}: mel.grad rel {rel:.3e}")
  assert rel <= DSPECT_TOL


def test_infer_differentiable_equal_and_refusals():
  """infer_differentiable at full depth (256 channels, 12 flows): audio and the noise gradients equal, mel.grad within
  1e-4; the refusals of the default mode (trainable weights, a second backward) hold in recompute mode."""
  hp, sd, mel, _ = _setup(dict(), 2, 9, 3)
  res = {rc: _synthesis(hp, sd, mel, rc) for rc in (False, True)}
  _check_synthesis(res[True], res[False], "c256")
  model = _model(hp, sd, True)                                  # trainable parameters
  with pytest.raises(WgError):
    model.infer_differentiable(mel.cuda().requires_grad_(True), 1.0)
  model.requires_grad_(False)
  audio = model.infer_differentiable(mel.cuda().requires_grad_(True), 1.0)
  loss = audio.square().mean()
  loss.backward(retain_graph=True)
  with pytest.raises((WgError, RuntimeError)):
    loss.backward()


def test_flow_ranges_under_data_parallel_single_rank():
  """Data-parallel mode cuts the backward into one call per flow (wg_train_backward with flow_hi = flow_lo):
  each call replays its own flow, the call of flow 0 finishes d spect.  Equal to the single-call recompute backward."""
  import torch.distributed as dist
  from waveglow_amd.train import enable_data_parallel
  over = dict(n_channels=64, n_layers=3, n_flows=6, n_early_every=2)
  hp, sd, mel, wav = _setup(over, 2, 6, 2)
  out_ref, g_ref = _train_step(hp, sd, mel, wav, True)
  model = _model(hp, sd, True)
  s = socket.socket()
  s.bind(("127.0.0.1", 0))
  port = s.getsockname()[1]
  s.close()
  dist.init_process_group("nccl", init_method=f"tcp://127.0.0.1:{port}", rank=0, world_size=1,
                          device_id=torch.device("cuda:0"))
  try:
    assert enable_data_parallel(model, force=True)
    out, g = _train_step(hp, sd, mel, wav, True, model)
  finally:
    dist.destroy_process_group()
  for name in g_ref:
    assert torch.equal(g[name], g_ref[name]), name


def test_two_outstanding_forwards_one_per_mode():
  """Gradient accumulation across modes: a full-save forward and a recompute forward outstanding at once, backward in
  reverse order.  Each gives what its own single run gives; the pool keeps one workspace per mode."""
  over = dict(n_channels=64, n_layers=3, n_flows=4, n_early_every=2)
  hp, sd, mel, wav = _setup(over, 2, 6, 2)
  _, single_f = _train_step(hp, sd, mel, wav, False)
  _, single_r = _train_step(hp, sd, mel, wav, True)
  model = _model(hp, sd, False)
  crit = WaveGlowLoss(1.0)
  l_full = crit(model((mel.cuda(), wav.cuda())), None)
  model.recompute_activations = True
  l_rec = crit(model((mel.cuda(), wav.cuda())), None)
  model.zero_grad()
  l_rec.backward()
  torch.cuda.synchronize()
  g_rec = {n: p.grad.detach().cpu().clone() for n, p in model.named_parameters()}
  model.zero_grad()
  l_full.backward()
  torch.cuda.synchronize()
  g_full = {n: p.grad.detach().cpu().clone() for n, p in model.named_parameters()}
  for name in single_f:
    assert torch.equal(g_rec[name], single_r[name]), f"recompute: {name}"
    assert torch.equal(g_full[name], single_f[name]), f"full save: {name}"
  pool = model._engine._train_pool
  assert sorted(e["flags"] for e in pool) == [0, 1] and not any(e["busy"] for e in pool)
  # alternating modes reuse the two workspaces
  for recompute in (False, True, False):
    model.recompute_activations = recompute
    crit(model((mel.cuda(), wav.cuda())), None).backward()
  assert len(model._engine._train_pool) == 2


def test_stream_ordering_serial_vs_streams(monkeypatch):
  """Recompute mode with the launches on the caller's stream alone (WG_TRAIN_SERIAL=1) and on the default streams (two
  forward chains, the weight-gradient and slab-reduction streams): equal gradients.  This does not prove the absence of
  a race; it shows that the ordering code runs."""
  over = dict(n_channels=64, n_layers=8, n_flows=4, n_early_every=2)
  hp, sd, mel, wav = _setup(over, 4, 11, 9, crop=56)
  monkeypatch.setenv("WG_TRAIN_HALVES", "2")
  monkeypatch.setenv("WG_TRAIN_SERIAL", "1")
  out_s, g_s = _train_step(hp, sd, mel, wav, True)
  monkeypatch.setenv("WG_TRAIN_SERIAL", "0")
  for rep in range(2):
    out_c, g_c = _train_step(hp, sd, mel, wav, True)
    for a, b in zip(out_c, out_s):
      assert torch.equal(a, b)
    for name in g_s:
      assert torch.equal(g_c[name], g_s[name]), f"{name}: streams differ from the serial run (rep {rep})"


@pytest.mark.parametrize("force_bn", ["128", "64"])
def test_forced_layer_tile_width(force_bn, monkeypatch):
  """WG_FORCE_BN pins the WN-layer tile width of the forward; the replay must read the same width."""
  monkeypatch.setenv("WG_FORCE_BN", force_bn)
  hp, sd, mel, wav = _setup(dict(n_layers=3, n_flows=4, n_early_every=2), 3, 11, 4, crop=56)
  out_f, g_f = _train_step(hp, sd, mel, wav, False)
  out_r, g_r = _train_step(hp, sd, mel, wav, True)
  _check_modes(out_r, g_r, out_f, g_f, f"bn{force_bn}")
