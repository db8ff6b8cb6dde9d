"""Golden vectors at TRAINED-checkpoint dynamic range from the REFERENCE's own model code (build container only).

  python tests/golden/make_golden_hot.py [hot_f1] [hot_f2e] [hot_c256] [hot_f6]

For every case of tests/_hot.py and both weight sets ("fwd": calibrated for analysis, "inv": for synthesis), one file
tests/golden/<case>.npz, data only, keys ``<set>/...``:

  heat, weights_crc32, w/<key>    (s_end, cond, gate), the crc32 of the full dense state dict, and the calibrated tensors
                                  (every ``convinv.k.conv.weight`` and ``WN.k.end.bias``) -- the rest of the weights is
                                  ``synthetic.make_state_dict(weight_seed)`` times the multipliers (_hot.hot_state_dict)
  regime/...                      the statistics _hot.regime measured (they are asserted here and again in test_hot_cpu.py)
  fwd/fwd_z, fwd_log_s_k, fwd_log_det, fwd_loss
                                  ``WaveGlow.forward`` (model.py:178-221) + ``WaveGlowLoss`` (train.py:31-45), dense weights
  fwd/loss, grad_names, grad_norm, grad_sum, grad_head, full/<name>, mel_grad, audio_grad
                                  the weight-normed model's training step (train.py:190-196): norm, sum and first 8 values
                                  of every parameter gradient, the whole gradient of tensors of at most 4096 elements, and
                                  the input gradients
  inv/audio                       ``WaveGlow.infer`` (model.py:223-274), noise drawn from the seeded global CPU RNG
  inv/audio_from_weightnorm_ckpt  the same from the weight-normed checkpoint form (hot_f1)
  <set>/yard/<group>/names, rel, rel_draws
                                  the yardstick: relative L2 error of _hot.emulated against the fp64 oracle per compared
                                  quantity -- the max over the three input draws of _hot.YARD_SEEDS, and the three values.
                                  Groups: fwd/yard/train (one training step, weight-norm form), inv/yard/infer (audio, dense
                                  weights), inv/yard/synth (audio and every gradient through synthesis, weight-norm form)

The inputs are stored as seeds (_hot.make_inputs).  Members are written with a fixed timestamp, so a second run gives the
same bytes.
"""
import io
import os
import sys
import zipfile

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.abspath(os.path.join(HERE, "..")))
sys.path.insert(0, os.path.abspath(os.path.join(HERE, "..", "..")))
import make_golden_corners as MC  # noqa: E402  (imports the reference; its dense_model / train_step are the recipes)
import _corners as K  # noqa: E402
import _hot as H  # noqa: E402
from waveglow_amd import synthetic  # noqa: E402

torch.set_num_threads(8)
FULL = 4096


def save_npz(path, arrays):
  """np.savez_compressed with a fixed member timestamp (numpy stamps the wall clock)."""
  with zipfile.ZipFile(path, "w", zipfile.ZIP_DEFLATED) as zf:
    for key, val in arrays.items():
      buf = io.BytesIO()
      np.lib.format.write_array(buf, np.asanyarray(val), allow_pickle=False)
      info = zipfile.ZipInfo(key + ".npy", date_time=(1980, 1, 1, 0, 0, 0))
      info.compress_type = zipfile.ZIP_DEFLATED
      info.external_attr = 0o644 << 16
      zf.writestr(info, buf.getvalue())


def yardstick(name, direction, sd, r):
  """(names, rel[max over draws], rel per draw) of emulated vs the fp64 oracle on the draws of H.YARD_SEEDS."""
  cfg = H.oracle_cfg_from_hp(H.HParams(**H.CASES[name][0]))
  per = []
  for draw in H.YARD_SEEDS:
    inputs = H.make_inputs(name, direction, draw)
    e = H.errors(H.emulated(direction, sd, inputs, cfg, r=r), H.exact(direction, sd, inputs, cfg, r=r))
    names = list(e)
    per.append([err / max(den, 1e-30) for err, den in e.values()])
  per = np.array(per, dtype=np.float64)
  assert np.isfinite(per).all(), (name, direction, [n for n, v in zip(names, per.max(0)) if not np.isfinite(v)])
  return np.array(names), per.max(0).astype(np.float32), per.astype(np.float32)


def run(name):
  over, B, T, wseed, heats = H.CASES[name]
  out = {"hp_json": np.array(repr(sorted(over.items()))), "weight_seed": np.array(wseed), "B": np.array(B), "T": np.array(T),
         "sigma": np.array(H.SIGMA, dtype=np.float32), "crop": np.array(H.CROP), "noise_seed": np.array(H.noise_seed(T)),
         "yard_draws": np.array(H.YARD_SEEDS)}
  for d in H.DIRECTIONS:
    sd = H.calibrate(name, d)
    sdn = synthetic.to_weightnorm_form(sd)
    st = H.regime(name, d, sd)
    H.assert_regime(st, d, f"{name}/{d}")
    agree = H.oracle_agreement(name, d, sd)
    assert agree[0] <= 1e-4, agree
    print(f"{name}/{d} {heats[d]}: max |a| {st['a_max']:.1f} max |b| {st['b_absmax']:.1f} min b {st['b_min']:.1f} "
          f"share |a| > 4 {st['a_gt4']:.2f} log_s std {min(st['log_s_std']):.2f} .. {max(st['log_s_std']):.2f} "
          f"max {st['log_s_max']:.1f} cond {min(st['cond']):.1f} .. {max(st['cond']):.1f} "
          f"min |logdet| {min(abs(v) for v in st['logdet']):.2f}; fp32 vs fp64 oracle {agree[0]:.1e} ({agree[1]})", flush=True)
    rec = {"heat": np.array(heats[d], dtype=np.float64), "weights_crc32": np.array(K.weights_crc(sd), dtype=np.uint32)}
    for key in H.calibrated_keys(H.HParams(**over)):
      rec[f"w/{key}"] = sd[key].numpy()
    for key, v in st.items():
      rec[f"regime/{key}"] = np.array(v, dtype=np.float64)
    inputs = H.make_inputs(name, d)
    if d == "fwd":
      mel, wav = inputs
      with torch.no_grad():
        model = MC.dense_model(over, sd)
        z, log_s_list, log_det_list = model((mel, wav))
        rec["fwd_log_det"] = np.array([float(x) for x in log_det_list], dtype=np.float32)   # before the in-place loss
        loss = MC.ref_train.WaveGlowLoss(sigma=1.0)((z, log_s_list, log_det_list), None)
        rec["fwd_z"] = z.numpy()
        for k, ls in enumerate(log_s_list):
          rec[f"fwd_log_s_{k}"] = ls.numpy()
        rec["fwd_loss"] = np.array(float(loss), dtype=np.float32)
      loss_t, grads, g_mel, g_wav = MC.train_step(over, sd, mel, wav)
      rec["loss"] = np.array(loss_t, dtype=np.float32)
      rec["grad_names"] = np.array(list(grads))
      rec["grad_norm"] = np.array([float(g.norm()) for g in grads.values()], dtype=np.float32)
      rec["grad_sum"] = np.array([float(g.double().sum()) for g in grads.values()], dtype=np.float32)
      head = np.zeros((len(grads), 8), dtype=np.float32)
      for i, (n, g) in enumerate(grads.items()):
        v = g.flatten()[:8].numpy()
        head[i, :v.size] = v
        if g.numel() <= FULL:
          rec[f"full/{n}"] = g.numpy().copy()
      rec["grad_head"] = head
      rec["mel_grad"], rec["audio_grad"] = g_mel.numpy().copy(), g_wav.numpy().copy()
      groups = [("train", sdn, None)]
      print(f"  reference: fwd loss {float(loss):.5f} train loss {loss_t:.5f} z rms {float(z.pow(2).mean().sqrt()):.3f}")
    else:
      mel = inputs[0]
      with torch.no_grad():
        model = MC.dense_model(over, sd)
        torch.manual_seed(H.noise_seed(T))
        audio = model.infer(mel, sigma=H.SIGMA)
        rec["audio"] = audio.numpy()
        if name == "hot_f1":
          model_n = MC.dense_model(over, sd, normed=True)      # built before seeding: its constructor draws too
          torch.manual_seed(H.noise_seed(T))
          rec["audio_from_weightnorm_ckpt"] = model_n.infer(mel, sigma=H.SIGMA).numpy()
      groups = [("infer", sd, None), ("synth", sdn, H.cotangent(name))]
      print(f"  reference: audio rms {float(audio.pow(2).mean().sqrt()):.3f} max {float(audio.abs().max()):.2f}")
    for group, weights, r in groups:
      names, rel, per = yardstick(name, d, weights, r)
      rec[f"yard/{group}/names"], rec[f"yard/{group}/rel"], rec[f"yard/{group}/rel_draws"] = names, rel, per
      order = np.argsort(-rel)
      vals = " ".join(f"{names[i]} {rel[i]:.2e}" for i in range(len(names)) if not str(names[i]).startswith("p/"))
      print(f"  yard {group}: {vals}")
      print(f"  yard {group}: worst " + ", ".join(f"{names[i]} {rel[i]:.2e} ({per[:, i].min():.2e} .. {per[:, i].max():.2e})"
                                                 for i in order[:4]) + f"; median {np.median(rel):.2e}", flush=True)
      if name == "hot_f6":
        over_limit = [(str(names[i]), float(rel[i])) for i in order if rel[i] > H.F6_LIMIT]
        print(f"  hot_f6 {group}: {len(over_limit)} of {len(names)} quantities above {H.F6_LIMIT}: {over_limit[:6]}")
    out.update({f"{d}/{k}": v for k, v in rec.items()})
  save_npz(H.fixture_path(name), out)
  print(name, "written", os.path.getsize(H.fixture_path(name)), "bytes", flush=True)


if __name__ == "__main__":
  for name in (sys.argv[1:] or H.IDS):
    run(name)
