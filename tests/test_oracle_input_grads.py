"""The CPU oracle's INPUT gradients (autograd through oracle.torch_oracle.forward_ref / loss_ref) against the reference's
own ``loss.backward()`` with ``mel`` and ``audio`` requiring grad (tests/golden/c64_input_grads.npz,
make_golden_input_grads.py).  The oracle is the yardstick of tests/test_gpu_input_grads.py for the shapes no fixture
covers, so it is pinned here.  The loss is bit-identical; the input gradients are not (the two autograd graphs sum the
contributions to d spect / d audio in different orders): measured ||g - g_ref|| / ||g_ref|| = 1.6e-6 for d mel and
1.9e-7 for d audio, held to ORACLE_TOL."""
import ast
import os

import numpy as np
import pytest
import torch

from _cases import GOLDEN, oracle_cfg_from_hp
from waveglow_amd import synthetic
from waveglow_amd.hparams import HParams

ORACLE_TOL = 2e-6


def input_grads_ref(sd_weightnorm, mel, audio, cfg, sigma=1.0):
  """(loss, d mel, d audio) of forward_ref -> loss_ref -> backward on CPU fp32 (the weights composed with
  torch._weight_norm(v, g, 0), as the parametrization does)."""
  from oracle import torch_oracle as O
  dense = {}
  for k, v in sd_weightnorm.items():
    if k.endswith("parametrizations.weight.original1"):
      base = k[:-len("parametrizations.weight.original1")]
      dense[base + "weight"] = torch._weight_norm(v, sd_weightnorm[base + "parametrizations.weight.original0"], 0)
    elif not k.endswith("parametrizations.weight.original0"):
      dense[k] = v
  mel = mel.detach().clone().requires_grad_(True)
  audio = audio.detach().clone().requires_grad_(True)
  loss = O.loss_ref(*O.forward_ref(dense, mel, audio, cfg), sigma)
  g_mel, g_audio = torch.autograd.grad(loss, [mel, audio])
  return float(loss.detach()), g_mel, g_audio


@pytest.mark.parametrize("case", ["c64", "c64_odd"])
def test_oracle_input_grads_match_reference_fixture(case):
  fx = np.load(os.path.join(GOLDEN, "c64_input_grads.npz"))
  over = dict(ast.literal_eval(str(fx["hp_json"])))
  hp = HParams(**over)
  sd = synthetic.to_weightnorm_form(synthetic.make_state_dict(hp, seed=int(fx["weight_seed"])))
  mel, audio = torch.from_numpy(fx[f"{case}/mel"]), torch.from_numpy(fx[f"{case}/audio"])
  loss, g_mel, g_audio = input_grads_ref(sd, mel, audio, oracle_cfg_from_hp(hp))
  assert g_mel.shape == mel.shape and g_audio.shape == audio.shape
  assert loss == float(fx[f"{case}/loss"])
  for g, key in ((g_mel, "mel_grad"), (g_audio, "audio_grad")):
    ref = torch.from_numpy(fx[f"{case}/{key}"])
    assert float((g - ref).norm()) <= ORACLE_TOL * float(ref.norm()), key
  # the samples the unfold drops (model.py:195) and the mel frames whose columns were all trimmed get exactly 0
  keep = audio.shape[1] - audio.shape[1] % hp.n_group
  assert bool((g_audio[:, keep:] == 0).all())
