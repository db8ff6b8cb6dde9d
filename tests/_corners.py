"""Shared by the flow-corner tests and tests/golden/make_golden_corners.py: the depth / flow-layout corners of the
envelope (``n_layers = 1``, ``n_flows = 1``, 4- and 6-channel early outputs, flow width 2, an ``n_early_every`` that does not
divide ``n_flows``, zero-channel early outputs) and how the inputs of tests/golden/flow_corners.npz are rebuilt from its
seeds."""
import os
import zlib

import numpy as np
import torch

from waveglow_amd import synthetic
from waveglow_amd.hparams import HParams

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
FIXTURE = os.path.join(GOLDEN, "flow_corners.npz")

_W = dict(n_layers=1, n_flows=2, n_early_every=1, n_early_size=2)
# id: HParams overrides
LAYOUTS = {
  "l1": dict(n_channels=64, n_layers=1, n_flows=4, n_early_every=2),              # first = last WN layer
  "l1_c128": dict(n_channels=128, **_W),                                         # ... at every kernel width
  "l1_c256": dict(n_channels=256, **_W),
  "l1_c512": dict(n_channels=512, **_W),
  "f1": dict(n_channels=64, n_layers=3, n_flows=1, n_early_every=4),              # one flow, n_early_every > n_flows
  "l1f1": dict(n_channels=64, n_layers=1, n_flows=1, n_early_every=1),            # both
  "e4": dict(n_channels=64, n_layers=3, n_flows=2, n_early_every=1, n_early_size=4),   # 4-channel peel, c = 4
  "e6": dict(n_channels=64, n_layers=3, n_flows=2, n_early_every=1, n_early_size=6),   # 6-channel peel, c = 2, h = 1
  "c2": dict(n_channels=64, n_layers=2, n_flows=4, n_early_every=1, n_early_size=2),   # widths 8, 6, 4, 2 in one model
  "ee3": dict(n_channels=64, n_layers=2, n_flows=5, n_early_every=3),             # n_early_every does not divide n_flows
  "e0": dict(n_channels=64, n_layers=2, n_flows=3, n_early_every=1, n_early_size=0),   # zero-channel early tensors
}
IDS = list(LAYOUTS)
L1_IDS = [i for i in IDS if i.startswith("l1")]
NORMED_AUDIO_IDS = ("l1", "e6")          # infer from the weight-normed checkpoint form is stored for these
B, T, SIGMA = 2, 6, 0.7                  # the fixture's shape
# Weight seeds.  A seed is taken only if every parameter gradient of the fixture's training step has an fp32-oracle norm of at
# least MIN_GRAD_NORM: below 2e-5 the absolute floor of the gradient bound (5e-3 ||g_ref|| + 1e-7) would decide the outcome
# instead of the relative part; at 1e-4 the floor is at most a fifth of the bound.  One tensor is exempt because no seed can
# help it: the direction v of a start conv with ONE input channel (h = 1).  Its weight-normed rows are g sign(v), so d v is
# identically zero (the oracle gives ~1e-11 of rounding), and the floor is the right bound for it: the library must write
# zeros.  make_golden_corners.py walks the seeds upward from FIRST_SEED[id] until the criterion holds and stores the one it
# took; the CPU test re-checks it on the oracle.
MIN_GRAD_NORM = 1e-4
FIRST_SEED = {name: 31 + i for i, name in enumerate(IDS)}


def structurally_zero(hp, pname):
  """True for ``WN.k.start...original1`` of a flow with one coupling channel (see above)."""
  parts = pname.split(".")
  return (parts[0] == "WN" and parts[2] == "start" and pname.endswith("original1")
          and synthetic.flow_channels(hp)[int(parts[1])] == 2)


def seed_is_good(hp, grads):
  """The criterion above on {parameter name: fp32 gradient}."""
  return all(float(g.norm()) >= MIN_GRAD_NORM for n, g in grads.items() if not structurally_zero(hp, n))


def early_flows(hp):
  return [k for k in range(hp.n_flows) if k % hp.n_early_every == 0 and k > 0]


def weights_crc(sd):
  crc = 0
  for key in sorted(sd):
    crc = zlib.crc32(sd[key].numpy().tobytes(), crc)
  return crc


def replay_noise(hp, n_batch, L, seed):
  """The draws of the reference's ``infer`` (model.py:234-244, :260-271) replayed from the global CPU RNG."""
  torch.manual_seed(seed)
  z_init = torch.FloatTensor(n_batch, synthetic.flow_channels(hp)[-1], L).normal_()
  z_early = {}
  for k in reversed(early_flows(hp)):
    z_early[k] = torch.FloatTensor(n_batch, hp.n_early_size, L).normal_()
  return z_init, z_early


def make_inputs(hp, n_batch, n_frames, crop=96):
  """(mel, waveform of 256 T - crop samples) as the other fixtures seed them."""
  mel = synthetic.make_mel(n_batch, n_frames, hp.n_mel_channels, seed=1234 + n_batch + n_frames)
  g = torch.Generator().manual_seed(99 + n_frames)
  wav = torch.rand(n_batch, 256 * n_frames - crop, generator=g) * 0.6 - 0.3
  return mel, wav


def noise_seed(n_frames):
  return 4321 + n_frames


def pack_f32(a):
  """fp32 [...] -> uint8 [4, ...], byte planes first: the same bits, but the sign / exponent bytes lie together and deflate
  well, which keeps the fixture below the size of the largest one under tests/golden/ (lossless; unpack_f32 undoes it)."""
  a = np.ascontiguousarray(a, dtype=np.float32)
  return np.ascontiguousarray(np.moveaxis(a.view(np.uint8).reshape(a.shape + (4,)), -1, 0))


def unpack_f32(u):
  return np.ascontiguousarray(np.moveaxis(u, 0, -1)).view(np.float32)[..., 0]


_npz = None


def fixture():
  global _npz
  if _npz is None:
    _npz = np.load(FIXTURE, allow_pickle=False)
  return _npz


class Corner:
  """One layout of the fixture, with the attributes of ``_cases.Case`` (hp, sd, mel, z_init, z_early, sigma, audio,
  oracle_cfg) so that the helpers written for ``Case`` take it, plus ``wav`` (the forward pass's waveform) and ``get``."""

  def __init__(self, name):
    self.name = name
    self.npz = fixture()
    self.over = LAYOUTS[name]
    self.hp = HParams(**self.over)
    self.wseed = int(self.get("weight_seed"))
    self.sigma = float(self.get("sigma"))
    self.sd = synthetic.make_state_dict(self.hp, seed=self.wseed)
    self.mel, self.wav = make_inputs(self.hp, B, T)
    self.z_init, self.z_early = replay_noise(self.hp, B, 32 * T, int(self.get("noise_seed")))
    self.audio = torch.from_numpy(self.get("audio"))

  def get(self, key):
    a = self.npz[f"{self.name}/{key}"]
    return unpack_f32(a) if a.dtype == np.uint8 else a

  def has(self, key):
    return f"{self.name}/{key}" in self.npz.files

  def grad_summary(self):
    """{parameter name: (norm, first values)} of the reference's own backward."""
    names, norm, head = self.get("grad_names"), self.get("grad_norm"), self.get("grad_head")
    return {str(n): (float(norm[i]), torch.from_numpy(head[i])) for i, n in enumerate(names)}

  def sd_normed(self):
    return synthetic.to_weightnorm_form(self.sd)

  def oracle_cfg(self):
    from _cases import oracle_cfg_from_hp
    return oracle_cfg_from_hp(self.hp)
