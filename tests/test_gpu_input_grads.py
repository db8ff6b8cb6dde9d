"""GPU: gradients of ``WaveGlow.forward`` w.r.t. its INPUTS (mel, audio), with trainable and with frozen weights.

The reference's forward is plain autograd (model.py:178-221): after ``WaveGlowLoss(model((mel, audio))).backward()``
``mel.grad`` and ``audio.grad`` are set as well.  Yardsticks: tests/golden/c64_input_grads.npz (the reference's own
backward, make_golden_input_grads.py) and the CPU oracle (pinned to that fixture in test_oracle_input_grads.py).
Tolerance as for the parameter gradients (test_gpu_train.py): ``||g - g_ref|| <= 5e-3 ||g_ref||`` per tensor.
"""
import ast
import os

import numpy as np
import pytest
import torch

from _cases import GOLDEN, oracle_cfg_from_hp
from test_oracle_input_grads import input_grads_ref
from waveglow_amd import synthetic
from waveglow_amd._lib import WgError
from waveglow_amd.hparams import HParams
from waveglow_amd.model import WaveGlow, WaveGlowLoss

pytestmark = pytest.mark.gpu

GRAD_TOL = 5e-3


@pytest.fixture(autouse=True)
def _poisoned_gradient_buffers(monkeypatch):
  """Parameter AND input gradient buffers start from NaN: an entry the library never writes makes grad_finite false."""
  monkeypatch.setenv("WG_TRAIN_POISON_GRADS", "1")


def _fixture():
  fx = np.load(os.path.join(GOLDEN, "c64_input_grads.npz"))
  hp = HParams(**dict(ast.literal_eval(str(fx["hp_json"]))))
  sd = synthetic.to_weightnorm_form(synthetic.make_state_dict(hp, seed=int(fx["weight_seed"])))
  return fx, hp, sd


def _model(hp, sd, frozen=False):
  model = WaveGlow(hp)
  model.load_state_dict(sd)
  model = model.to("cuda:0").train()
  if frozen:
    model.requires_grad_(False)
  return model


def _step(model, mel, wav, mel_rg=True, audio_rg=True):
  """One forward + WaveGlowLoss + backward; (loss, d mel or None, d audio or None, {name: p.grad or None})."""
  model.zero_grad(set_to_none=True)
  m = mel.cuda().requires_grad_(mel_rg)
  a = wav.cuda().requires_grad_(audio_rg)
  loss = WaveGlowLoss(1.0)(model((m, a)), None)
  loss.backward()
  torch.cuda.synchronize()
  assert bool(model.grad_finite), "the library left an entry of a (NaN-poisoned) gradient buffer unwritten"
  get = lambda t: None if t.grad is None else t.grad.detach().cpu()
  return float(loss.detach()), get(m), get(a), {n: get(p) for n, p in model.named_parameters()}


def _close(g, ref, what):
  assert g is not None, f"{what}: no gradient"
  assert g.shape == ref.shape, what
  assert torch.isfinite(g).all(), what
  err, den = float((g - ref).norm()), float(ref.norm())
  print(f"{what}: rel {err / max(den, 1e-30):.3e} (err {err:.3e}, ref norm {den:.3e})")
  assert err <= GRAD_TOL * den, f"{what}: error {err:.3e} vs norm {den:.3e}"


@pytest.mark.parametrize("case", ["c64", "c64_odd"])
def test_input_grads_trainable_and_frozen_match_reference(case):
  """(1) trainable: d mel / d audio against the reference fixture and the oracle; the parameter gradients are bit-identical
  to a step whose inputs need no gradient.  (2) the same model frozen: bit-identical input gradients, no p.grad.
  (5) the samples the unfold drops get exactly 0, and the gradients have the inputs' shapes."""
  fx, hp, sd = _fixture()
  mel, wav = torch.from_numpy(fx[f"{case}/mel"]), torch.from_numpy(fx[f"{case}/audio"])
  model = _model(hp, sd)
  loss, g_mel, g_audio, pg = _step(model, mel, wav)
  assert abs(loss - float(fx[f"{case}/loss"])) <= 2e-3 * max(1.0, abs(float(fx[f"{case}/loss"])))
  _close(g_mel, torch.from_numpy(fx[f"{case}/mel_grad"]), f"{case} d mel vs reference")
  _close(g_audio, torch.from_numpy(fx[f"{case}/audio_grad"]), f"{case} d audio vs reference")
  _, o_mel, o_audio = input_grads_ref(sd, mel, wav, oracle_cfg_from_hp(hp))
  _close(g_mel, o_mel, f"{case} d mel vs oracle")
  _close(g_audio, o_audio, f"{case} d audio vs oracle")
  assert g_mel.shape == mel.shape and g_audio.shape == wav.shape
  keep = wav.shape[1] - wav.shape[1] % hp.n_group
  assert bool((g_audio[:, keep:] == 0).all())
  # parameter gradients do not depend on whether the inputs want theirs
  _, n_mel, n_audio, pg0 = _step(model, mel, wav, mel_rg=False, audio_rg=False)
  assert n_mel is None and n_audio is None
  for name, g in pg.items():
    assert torch.equal(g, pg0[name]), name
  # frozen weights: the data-gradient chain alone gives the same input gradients, and no parameter gradient
  frozen = _model(hp, sd, frozen=True)
  _, f_mel, f_audio, fpg = _step(frozen, mel, wav)
  assert torch.equal(f_mel, g_mel)
  assert torch.equal(f_audio, g_audio)
  assert all(g is None for g in fpg.values())


def test_mel_only_and_audio_only():
  """(3) one input at a time, trainable and frozen: the same values as with both."""
  fx, hp, sd = _fixture()
  mel, wav = torch.from_numpy(fx["c64/mel"]), torch.from_numpy(fx["c64/audio"])
  _, g_mel, g_audio, _ = _step(_model(hp, sd), mel, wav)
  for frozen in (False, True):
    model = _model(hp, sd, frozen=frozen)
    _, m_only, a_none, _ = _step(model, mel, wav, mel_rg=True, audio_rg=False)
    assert a_none is None and torch.equal(m_only, g_mel)
    _, m_none, a_only, _ = _step(model, mel, wav, mel_rg=False, audio_rg=True)
    assert m_none is None and torch.equal(a_only, g_audio)


@pytest.mark.parametrize("over,B,T,crop", [
    (dict(n_channels=128, n_layers=2, n_flows=2, n_early_every=1, n_early_size=2), 2, 7, 24),
    (dict(n_channels=512, n_layers=2, n_flows=2, n_early_every=1, n_early_size=2), 2, 7, 24),
    (dict(n_channels=64, n_layers=2, n_flows=3, n_early_every=2, n_mel_channels=32), 3, 8, 40)])
def test_input_grads_other_widths_against_oracle(over, B, T, crop):
  """(4) the shapes of the existing width tests: 128 / 512 channels at small depth, 32 mel channels (one 32-row block of
  the transposed upsample)."""
  hp = HParams(**over)
  sd = synthetic.to_weightnorm_form(synthetic.make_state_dict(hp, seed=13))
  mel = synthetic.make_mel(B, T, n_mel=hp.n_mel_channels, seed=1234 + B + T)
  wav = torch.rand(B, 256 * T - crop, generator=torch.Generator().manual_seed(99 + T)) * 0.6 - 0.3
  _, o_mel, o_audio = input_grads_ref(sd, mel, wav, oracle_cfg_from_hp(hp))
  for frozen in (False, True):
    _, g_mel, g_audio, _ = _step(_model(hp, sd, frozen=frozen), mel, wav)
    _close(g_mel, o_mel, f"{over} frozen={frozen} d mel")
    _close(g_audio, o_audio, f"{over} frozen={frozen} d audio")


def test_full_size_directional_derivatives_of_the_inputs():
  """(6) configs[3] shapes (256 channels, 16 000 samples, 63 frames, B = 8), frozen weights: the central finite difference
  of the no-grad loss along mel.grad and along audio.grad matches their norms."""
  hp = HParams()
  sd = synthetic.to_weightnorm_form(synthetic.make_state_dict(hp, seed=7))
  B = 8
  mel = synthetic.make_mel(B, 63, seed=1234 + B + 63).cuda()
  wav = (torch.rand(B, 16000, generator=torch.Generator().manual_seed(99 + 63)) * 0.6 - 0.3).cuda()
  model = _model(hp, sd, frozen=True)
  crit = WaveGlowLoss(1.0)
  m, a = mel.clone().requires_grad_(True), wav.clone().requires_grad_(True)
  crit(model((m, a)), None).backward()
  assert bool(model.grad_finite)
  for name, x, g in (("mel", mel, m.grad), ("audio", wav, a.grad)):
    gnorm = float(g.double().norm())
    assert np.isfinite(gnorm) and gnorm > 0
    d = g / gnorm

    def loss_at(eps):
      xs = (x + eps * d, wav) if name == "mel" else (mel, x + eps * d)
      with torch.no_grad():
        return float(crit(model(xs), None))

    # a step of 2 % of the input's norm: the no-grad pass reads mel as fp16 (spacing 4e-3 at |x| ~ 5), so a step that
    # moves each entry by less than that is rounded away instead of measured
    eps = 0.02 * float(x.double().norm())
    fd = (loss_at(eps) - loss_at(-eps)) / (2 * eps)
    print(f"d {name}: finite difference {fd:.5e}  vs  |grad| {gnorm:.5e}")
    assert abs(fd - gnorm) <= 0.03 * gnorm


def test_input_grads_under_single_rank_data_parallel(monkeypatch):
  """(7) one-rank RCCL data parallel: input gradients equal the plain path (they are not all-reduced), the parameter
  gradients are unchanged, and a frozen model issues no collective at all."""
  import socket
  import torch.distributed as dist
  from waveglow_amd.train import enable_data_parallel
  fx, hp, sd = _fixture()
  mel, wav = torch.from_numpy(fx["c64/mel"]), torch.from_numpy(fx["c64/audio"])
  _, g_mel, g_audio, pg = _step(_model(hp, sd), mel, wav)
  _, f_mel, f_audio, _ = _step(_model(hp, sd, frozen=True), mel, wav)
  s = socket.socket()
  s.bind(("127.0.0.1", 0))
  port = s.getsockname()[1]
  s.close()
  dist.init_process_group("nccl", init_method=f"tcp://127.0.0.1:{port}", rank=0, world_size=1,
                          device_id=torch.device("cuda:0"))
  calls = []
  real = dist.all_reduce
  monkeypatch.setattr(dist, "all_reduce", lambda *a, **k: calls.append(1) or real(*a, **k))
  try:
    model = _model(hp, sd)
    assert enable_data_parallel(model, force=True)
    _, d_mel, d_audio, dpg = _step(model, mel, wav)
    assert len(calls) == hp.n_flows + 1
    frozen = _model(hp, sd, frozen=True)
    assert enable_data_parallel(frozen, force=True)
    calls.clear()
    _, df_mel, df_audio, dfpg = _step(frozen, mel, wav)
    assert calls == []
  finally:
    dist.destroy_process_group()
  assert torch.equal(d_mel, g_mel) and torch.equal(d_audio, g_audio)
  for name, g in pg.items():
    assert torch.equal(dpg[name], g), name
  assert torch.equal(df_mel, f_mel) and torch.equal(df_audio, f_audio)
  assert all(g is None for g in dfpg.values())


def test_frozen_unsupported_width_raises():
  """(8) a frozen 96-channel model (a width the training direction does not take) with mel.requires_grad raises instead
  of returning outputs without a graph."""
  hp = HParams(n_channels=96, n_layers=2, n_flows=2, n_early_every=1, n_early_size=2)
  sd = synthetic.to_weightnorm_form(synthetic.make_state_dict(hp, seed=3))
  model = _model(hp, sd, frozen=True)
  mel = synthetic.make_mel(1, 6, seed=2).cuda().requires_grad_(True)
  wav = torch.rand(1, 256 * 6, generator=torch.Generator().manual_seed(1)).cuda() * 0.6 - 0.3
  with pytest.raises(WgError):
    model((mel, wav))
