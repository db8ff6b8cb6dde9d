"""Resident tile walk of wn_layer_kernel (WG_RESIDENT, read per launch): a workgroup walks its share of its XCD label's run
tile by tile instead of ending after a pair.  Every tile computes what it computed before, so the forced resident launch
must agree BIT FOR BIT with today's launch (WG_RESIDENT=0) at every way the walk can break up -- whole pairs, a pair cut in
the middle, single tiles -- and for the first-layer, regular and last-layer instantiations, which every flow contains."""
import functools
import os

import pytest
import torch

from _cases import oracle_cfg_from_hp, rms
from test_gpu_parity import RMS_TOL, build_model, gpu_infer
from waveglow_amd import synthetic
from waveglow_amd.hparams import HParams

pytestmark = pytest.mark.gpu

SIGMA = 0.6


class _Env:
  """Environment inside the block.  The library reads WG_RESIDENT per launch; WG_FORCE_BN is read once, when a model's
  engine is created (wg_create, at the model's first inference call) -- so a model belongs to ONE tile width, and its first
  call has to happen inside the block that sets it (``_case`` keys its models by the width for that reason)."""

  def __init__(self, resident, force_bn=None):
    self.new = {"WG_RESIDENT": str(resident), "WG_FORCE_BN": force_bn}

  def __enter__(self):
    self.old = {k: os.environ.get(k) for k in self.new}
    for k, v in self.new.items():
      if v is None:
        os.environ.pop(k, None)
      else:
        os.environ[k] = v

  def __exit__(self, *exc):
    for k, v in self.old.items():
      if v is None:
        os.environ.pop(k, None)
      else:
        os.environ[k] = v


@functools.lru_cache(maxsize=None)
def _case(channels, B, T, force_bn):
  """(hp, sd, model, mel, z_init, z_early): 4 flows; B = 3, T = 50 at 256 channels is the shape of
  test_layer_tile_widths_agree_c256 -- 64 tiles of 128 columns, 8 per XCD label.  The model is new (no engine yet) and is
  only ever run under WG_FORCE_BN = force_bn."""
  hp = HParams(n_channels=channels, n_flows=4, n_early_every=2)
  sd = synthetic.make_state_dict(hp, seed=9)
  mel = synthetic.make_mel(B, T, seed=1)
  z_init, z_early = synthetic.make_noise(hp, B, 32 * T, seed=2)
  return hp, sd, build_model(hp, sd), mel, z_init, z_early


@functools.lru_cache(maxsize=None)
def _audio(channels, B, T, resident, force_bn):
  _, _, model, mel, z_init, z_early = _case(channels, B, T, force_bn)
  with _Env(resident, force_bn):
    out = gpu_infer(model, mel, z_init, z_early, SIGMA)
  assert torch.isfinite(out).all() and float(out.abs().max()) > 1e-3
  return out


@pytest.mark.parametrize("wgs", [8, 16, 24, 64])
def test_every_kind_of_walk_c256(wgs):
  """8 tiles per label: 8 workgroups walk eight tiles each, 16 four; 24 gives a label's workgroups 3, 3 and 2 tiles (the
  unrolled pair breaks in the middle); 64 one tile each (the pair's second half never runs)."""
  base = _audio(256, 3, 50, 0, "128")
  out = _audio(256, 3, 50, wgs, "128")
  assert torch.equal(out, base), float((out - base).abs().max())


def test_resident_walk_against_oracle_c256():
  """The forced path is right, not merely equal to something."""
  from oracle import torch_oracle as O
  hp, sd, _, mel, z_init, z_early = _case(256, 3, 50, "128")
  with torch.no_grad():
    ref = O.infer_ref(sd, mel, z_init, z_early, SIGMA, oracle_cfg_from_hp(hp))
  err = rms(_audio(256, 3, 50, 8, "128") - ref)
  print(f"resident walk vs oracle: rms err {err:.3e}")
  assert err <= RMS_TOL


def test_ragged_lengths_c256():
  """Per-utterance frame counts: column masks and the mel-row gather when a workgroup crosses utterances and phases."""
  hp, sd, model, mel, z_init, z_early = _case(256, 4, 40, "128")
  frames = torch.tensor([40, 17, 1, 33], dtype=torch.int32)
  ze = [z_early[k].cuda() for k in sorted(z_early, reverse=True)]
  outs = {}
  for wgs in (0, 8):
    with _Env(wgs, "128"), torch.no_grad():
      outs[wgs] = model.infer_with_noise(mel.cuda(), z_init.cuda(), ze, SIGMA, frames=frames).float().cpu()
  assert float(outs[0].abs().max()) > 1e-3
  assert torch.equal(outs[8], outs[0]), float((outs[8] - outs[0]).abs().max())


def test_one_layer_corner_c256():
  """n_layers = 1: the first layer is the last one -- the gathered first-layer K-step without a residual output."""
  from _corners import Corner
  c = Corner("l1_c256")
  model = build_model(c.hp, c.sd)
  outs = {}
  for wgs in (0, 8):
    with _Env(wgs, "128"):
      outs[wgs] = gpu_infer(model, c.mel, c.z_init, c.z_early, c.sigma)
  assert torch.isfinite(outs[0]).all() and float(outs[0].abs().max()) > 1e-3
  assert torch.equal(outs[8], outs[0]), float((outs[8] - outs[0]).abs().max())


@pytest.mark.parametrize("channels,force_bn,wgs", [(64, "128", 8), (64, "64", 8), (256, "64", 8), (512, None, 16)])
def test_other_widths(channels, force_bn, wgs):
  """64 channels at both tile widths (a model per width: 32 tiles of 128 columns, 64 of 64) and 512 channels (64-column
  tiles: 64 of them, four per workgroup at 16); 256 channels on 64-column tiles, where WG_RESIDENT=0 is the two-step-deep
  prefetch kernel and the walk the one-step ring.  None of these takes the walk by default; the forced launch must
  still agree with theirs bit for bit."""
  base = _audio(channels, 2, 40, 0, force_bn)
  out = _audio(channels, 2, 40, wgs, force_bn)
  assert torch.equal(out, base), float((out - base).abs().max())


def test_graph_replay_c256():
  """Captured with WG_RESIDENT=8 set before the capture: the replay equals the direct call (and the walk of WG_RESIDENT=0)."""
  hp, sd, _, mel, z_init, z_early = _case(256, 3, 50, "128")
  model = build_model(hp, sd)                     # a model of its own: nothing captured under another setting
  ze = [z_early[k].cuda() for k in sorted(z_early, reverse=True)]
  with _Env(8, "128"), torch.no_grad():
    direct = model.infer_with_noise(mel.cuda(), z_init.cuda(), ze, SIGMA)
    graphed = model.infer_with_noise(mel.cuda(), z_init.cuda(), ze, SIGMA, graph=True)
    again = model.infer_with_noise(mel.cuda(), z_init.cuda(), ze, SIGMA, graph=True)
  torch.cuda.synchronize()
  assert torch.equal(direct, graphed) and torch.equal(direct, again)
  assert torch.equal(direct.float().cpu(), _audio(256, 3, 50, 0, "128"))
