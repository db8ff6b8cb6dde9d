"""Golden INPUT gradients from the reference's own training step (build container only; imports the reference).

  python tests/golden/make_golden_input_grads.py

WaveGlow.forward (model.py:178-221, weight-normed parameters) -> WaveGlowLoss (train.py:31-45) -> loss.backward() on
CPU fp32 with ``mel`` and ``audio`` requiring grad: the full ``mel.grad`` and ``audio.grad`` of

  c64      the c64 case of make_golden_grads.py (audio_len = 256 T - 96);
  c64_odd  the same model with audio_len % 8 != 0 and not a multiple of 256 (the unfold drops the last samples, and
           the spectrogram is trimmed inside a frame: model.py:188-189, :195).
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.abspath(os.path.join(HERE, "..", "..")))
from _ref_import import import_reference  # noqa: E402
from waveglow_amd.hparams import HParams  # noqa: E402
from waveglow_amd import synthetic  # noqa: E402

ref_model, ref_hparams, ref_train = import_reference()

OVER = dict(n_channels=64, n_layers=4, n_flows=6, n_early_every=2)
B, T, WSEED = 2, 12, 5
# name: audio samples
CASES = {"c64": 256 * T - 96, "c64_odd": 256 * T - 301}

hp = HParams(**OVER)
sd = synthetic.make_state_dict(hp, seed=WSEED)
model = ref_model.WaveGlow(ref_hparams.HParams(**OVER))
model.load_state_dict(synthetic.to_weightnorm_form(sd))
model.train()
out = {"hp_json": np.array(repr(OVER)), "weight_seed": np.array(WSEED, dtype=np.int64)}
for name, S in CASES.items():
  mel = synthetic.make_mel(B, T, seed=1234 + B + T).requires_grad_(True)
  g = torch.Generator().manual_seed(99 + T)
  wav = (torch.rand(B, S, generator=g) * 0.6 - 0.3).requires_grad_(True)
  model.zero_grad()
  loss = ref_train.WaveGlowLoss(sigma=1.0)(model((mel, wav)), None)
  loss.backward()
  out[f"{name}/mel"] = mel.detach().numpy().copy()
  out[f"{name}/audio"] = wav.detach().numpy().copy()
  out[f"{name}/loss"] = np.array(float(loss), dtype=np.float32)
  out[f"{name}/mel_grad"] = mel.grad.numpy().copy()
  out[f"{name}/audio_grad"] = wav.grad.numpy().copy()
  print(name, "S", S, "loss", float(loss), "|d mel|", float(mel.grad.norm()), "|d audio|", float(wav.grad.norm()))
np.savez_compressed(os.path.join(HERE, "c64_input_grads.npz"), **out)
