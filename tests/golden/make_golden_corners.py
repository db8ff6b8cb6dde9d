"""Golden vectors of the depth / flow-layout corners from the REFERENCE's own model code (build container only).

  python tests/golden/make_golden_corners.py

For every layout of tests/_corners.py (``n_layers = 1`` at every kernel width, ``n_flows = 1``, 4- and 6-channel early
outputs, flow width 2, an ``n_early_every`` that does not divide ``n_flows``, zero-channel early outputs) at B = 2, T = 6, as
make_golden.py and make_golden_grads.py / make_golden_input_grads.py do for their cases:

  audio                        ``WaveGlow.infer`` (model.py:223-274), noise drawn from the seeded global CPU RNG
  audio_from_weightnorm_ckpt   the same from the weight-normed checkpoint form (l1, e6)
  fwd_z, fwd_log_s_k, fwd_log_det, fwd_loss
                               ``WaveGlow.forward`` (model.py:178-221) + ``WaveGlowLoss`` (train.py:31-45), dense weights,
                               on a waveform of 256 T - 96 samples
  loss, grad_names, grad_norm, grad_head
                               the weight-normed model's training step (train.py:190-196): loss, and the L2 norm and first
                               8 values of every parameter gradient of its own ``loss.backward()``
  mel_grad, audio_grad         the full input gradients of that backward

Everything ``waveglow_amd.synthetic`` and the seeds regenerate (weights, mel, waveform, noise) is stored as a seed, with a
crc32 of the weights.  One file, tests/golden/flow_corners.npz, keys ``<layout>/<name>``; data only.  fp32 tensors are stored
as uint8 byte planes (tests/_corners.py: pack_f32 / unpack_f32, lossless) because they deflate better that way.
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.abspath(os.path.join(HERE, "..")))
sys.path.insert(0, os.path.abspath(os.path.join(HERE, "..", "..")))
from _ref_import import import_reference  # noqa: E402
import _corners as K  # noqa: E402
from waveglow_amd.hparams import HParams  # noqa: E402
from waveglow_amd import synthetic  # noqa: E402

ref_model, ref_hparams, ref_train = import_reference()
torch.set_num_threads(8)


def dense_model(over, sd, normed=False):
  model = ref_model.WaveGlow(ref_hparams.HParams(**over))
  if normed:
    model.load_state_dict(synthetic.to_weightnorm_form(sd))
    model = ref_model.WaveGlow.remove_weightnorm(model)
  else:
    model = ref_model.WaveGlow.remove_weightnorm(model)
    model.load_state_dict(sd)
  return model.eval()


def train_step(over, sd, mel, wav):
  """The reference's training step on the weight-normed parameters; (loss, {name: grad}, mel.grad, audio.grad)."""
  model = ref_model.WaveGlow(ref_hparams.HParams(**over))
  model.load_state_dict(synthetic.to_weightnorm_form(sd))
  model.train()
  mel = mel.clone().requires_grad_(True)
  wav = wav.clone().requires_grad_(True)
  model.zero_grad()
  loss = ref_train.WaveGlowLoss(sigma=1.0)(model((mel, wav)), None)
  loss.backward()
  return float(loss), {n: p.grad.detach() for n, p in model.named_parameters()}, mel.grad, wav.grad


def run(name, over):
  hp = HParams(**over)
  mel, wav = K.make_inputs(hp, K.B, K.T)
  # the first weight seed whose gradients all clear the floor criterion (tests/_corners.py: MIN_GRAD_NORM)
  wseed = K.FIRST_SEED[name]
  while True:
    sd = synthetic.make_state_dict(hp, seed=wseed)
    loss_t, grads, g_mel, g_wav = train_step(over, sd, mel, wav)
    if K.seed_is_good(hp, grads):
      break
    wseed += 1
    assert wseed < K.FIRST_SEED[name] + 16, name
  out = {"weight_seed": np.array(wseed), "weights_crc32": np.array(K.weights_crc(sd), dtype=np.uint32),
         "sigma": np.array(K.SIGMA, dtype=np.float32), "noise_seed": np.array(K.noise_seed(K.T)),
         "hp_json": np.array(repr(sorted(over.items())))}
  with torch.no_grad():
    model = dense_model(over, sd)
    torch.manual_seed(K.noise_seed(K.T))
    audio = model.infer(mel, sigma=K.SIGMA)
    out["audio"] = audio.numpy()
    if name in K.NORMED_AUDIO_IDS:
      model_n = dense_model(over, sd, normed=True)          # built BEFORE seeding: its constructor draws from the same RNG
      torch.manual_seed(K.noise_seed(K.T))
      out["audio_from_weightnorm_ckpt"] = model_n.infer(mel, sigma=K.SIGMA).numpy()
    z, log_s_list, log_det_list = model((mel, wav))
    # snapshot before the loss: train.py:38-42 accumulates IN PLACE into log_det_W_list[0]
    out["fwd_log_det"] = np.array([float(x) for x in log_det_list], dtype=np.float32)
    loss = ref_train.WaveGlowLoss(sigma=1.0)((z, log_s_list, log_det_list), None)
    out["fwd_z"] = z.numpy()
    for k, ls in enumerate(log_s_list):
      out[f"fwd_log_s_{k}"] = ls.numpy()
    out["fwd_loss"] = np.array(float(loss), dtype=np.float32)
  out["loss"] = np.array(loss_t, dtype=np.float32)
  # one array each for all parameters (an archive member per value would cost more than the values): names in
  # named_parameters() order, norms, and the first 8 values (zero-padded where a tensor has fewer)
  out["grad_names"] = np.array(list(grads))
  out["grad_norm"] = np.array([float(g.norm()) for g in grads.values()], dtype=np.float32)
  head = np.zeros((len(grads), 8), dtype=np.float32)
  for i, g in enumerate(grads.values()):
    v = g.flatten()[:8].numpy()
    head[i, :v.size] = v
  out["grad_head"] = head
  out["mel_grad"] = g_mel.numpy().copy()
  out["audio_grad"] = g_wav.numpy().copy()
  print(f"{name}: weight seed {wseed} audio rms {float(audio.pow(2).mean().sqrt()):.4f} fwd loss {float(loss):.5f} "
        f"train loss {loss_t:.5f} params {len(grads)} min |grad| {min(float(g.norm()) for g in grads.values()):.3e}")
  # every fp32 tensor (not the scalars) goes in as byte planes: tests/_corners.py pack_f32
  return {f"{name}/{k}": (K.pack_f32(v) if v.dtype == np.float32 and v.ndim >= 1 else v) for k, v in out.items()}


if __name__ == "__main__":
  everything = {}
  for name, over in K.LAYOUTS.items():
    everything.update(run(name, over))
  np.savez_compressed(K.FIXTURE, **everything)
  print("wrote", K.FIXTURE, os.path.getsize(K.FIXTURE), "bytes")
