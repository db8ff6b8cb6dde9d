"""Host-side (no GPU) checks of the drop-in boundary: names, shapes, formats, error behaviour."""
import dataclasses
import json
import os

import numpy as np
import pytest
import torch

from waveglow_amd import synthetic
from waveglow_amd.audio import convert_wav, is_overamp, normalize_wav
from waveglow_amd.checkpoint import CheckpointWaveglow
from waveglow_amd.hparams import HParams, overwrite_custom_hparams, split_hparams_string
from waveglow_amd.model import WaveGlow
from waveglow_amd.sharding import shard_list, shard_range

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
ROOT = os.path.abspath(os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
KEYS = json.load(open(os.path.join(GOLDEN, "state_dict_keys.json")))


@pytest.mark.parametrize("tag", ["default", "c64_f4"])
def test_state_dict_keys_and_shapes_match_reference(tag):
  """Fixture = the reference's own state_dict (tests/golden/make_state_dict_keys.py): 686 keys weight-normed,
  470 after remove_weightnorm for the default hparams."""
  fx = KEYS[tag]
  m = WaveGlow(HParams(**fx["hparams"]))
  got = {k: list(v.shape) for k, v in m.state_dict().items()}
  assert got == fx["weight_normed"]
  assert sum(p.numel() for p in m.parameters()) == fx["n_params_weight_normed"]
  m = WaveGlow.remove_weightnorm(m)
  got = {k: list(v.shape) for k, v in m.state_dict().items()}
  assert got == fx["weight_norm_removed"]
  if tag == "default":
    assert len(fx["weight_normed"]) == 686 and len(fx["weight_norm_removed"]) == 470


def test_dense_state_names_are_the_470_key_form():
  fx = KEYS["c64_f4"]
  m = WaveGlow(HParams(**fx["hparams"]))
  with torch.no_grad():
    dense = m.dense_state()
  assert {k: list(v.shape) for k, v in dense.items()} == fx["weight_norm_removed"]


def test_weightnorm_fold_matches_dense_weights():
  hp = HParams(n_channels=64, n_flows=4, n_early_every=2, n_layers=3)
  sd = synthetic.make_state_dict(hp, seed=2)
  m = WaveGlow(hp)
  m.load_state_dict(synthetic.to_weightnorm_form(sd))
  with torch.no_grad():
    dense = m.dense_state()
  for k, v in sd.items():
    assert torch.allclose(dense[k], v, rtol=1e-5, atol=1e-7), k


def test_legacy_weight_g_weight_v_checkpoint_keys_load():
  """NVIDIA-era checkpoints store weight norm as ``weight_g`` / ``weight_v``."""
  hp = HParams(n_channels=64, n_flows=4, n_early_every=2, n_layers=3)
  sd = synthetic.to_weightnorm_form(synthetic.make_state_dict(hp, seed=3))
  legacy = {}
  for k, v in sd.items():
    k = k.replace("parametrizations.weight.original0", "weight_g").replace("parametrizations.weight.original1", "weight_v")
    legacy[k] = v
  m = WaveGlow(hp)
  m.load_state_dict(legacy)
  assert torch.equal(m.WN[1].in_layers[2].parametrizations.weight.original1, sd["WN.1.in_layers.2.parametrizations.weight.original1"])


def test_custom_hparams_follow_reference_semantics():
  hp = HParams()
  assert split_hparams_string("n_channels=512,sigma=0.6") == {"n_channels": "512", "sigma": "0.6"}
  hp2 = overwrite_custom_hparams(hp, {"n_channels": "512", "sigma": "0.6"})
  assert hp2.n_channels == 512 and isinstance(hp2.n_channels, int) and hp2.sigma == 0.6
  assert overwrite_custom_hparams(hp, None) is hp
  with pytest.raises(Exception):
    overwrite_custom_hparams(hp, {"no_such_param": "1"})     # utils.py:53-54: bare Exception
  assert overwrite_custom_hparams(hp, {"window": ""}).window is None   # utils.py:76-82
  # field names are the checkpoint format
  for name in ("segment_length", "n_mel_channels", "n_flows", "n_group", "n_early_every", "n_early_size", "n_layers",
               "n_channels", "kernel_size", "sampling_rate", "filter_length", "hop_length", "learning_rate", "sigma"):
    assert name in {f.name for f in dataclasses.fields(HParams)}


def test_checkpoint_roundtrip_reference_format(tmp_path):
  hp = HParams(n_channels=64, n_flows=4, n_early_every=2, n_layers=3)
  m = WaveGlow(hp)
  opt = torch.optim.Adam(m.parameters(), lr=hp.learning_rate)
  ck = CheckpointWaveglow.from_instances(m, opt, hp, iteration=7)
  path = tmp_path / "7.pt"
  ck.save(path)
  raw = torch.load(path, weights_only=True)
  assert set(raw) == {"state_dict", "optimizer", "learning_rate", "iteration", "hparams"}   # checkpoint.py:13-20
  ck2 = CheckpointWaveglow.load(path, torch.device("cpu"))
  assert ck2.iteration == 7 and ck2.get_hparams() == hp
  raw["hparams"]["some_future_field"] = 1
  assert CheckpointWaveglow(**raw).get_hparams() == hp     # unknown keys dropped (checkpoint.py:22-28)
  m2 = WaveGlow(ck2.get_hparams())
  m2.load_state_dict(ck2.state_dict)


def test_shard_ranges_partition_the_list():
  for n in (0, 1, 7, 8, 9, 256):
    for w in (1, 2, 3, 8):
      spans = [shard_range(n, r, w) for r in range(w)]
      assert spans[0][0] == 0 and spans[-1][1] == n
      assert all(spans[i][1] == spans[i + 1][0] for i in range(w - 1))
      sizes = [e - s for s, e in spans]
      assert max(sizes) - min(sizes) <= 1
  assert shard_list(list("abcde"), 1, 2) == ["d", "e"]


def test_wav_helpers():
  x = np.array([0.5, -0.25, 0.1], dtype=np.float32)
  n = normalize_wav(x)
  assert np.max(np.abs(n)) == 1.0 and not is_overamp(n)
  assert is_overamp(np.array([1.5], dtype=np.float32))
  i16 = convert_wav(n, np.int16)
  assert i16.dtype == np.int16 and i16[0] == 32767 and i16[1] == -16384
  assert np.array_equal(normalize_wav(np.zeros(4, dtype=np.float32)), np.zeros(4, dtype=np.float32))


def test_synthetic_inputs_are_deterministic():
  hp = HParams()
  a, b = synthetic.make_mel(2, 5), synthetic.make_mel(2, 5)
  assert torch.equal(a, b) and a.min() >= -11.5 and a.max() <= 2.0
  z, ze = synthetic.make_noise(hp, 2, 160)
  assert z.shape == (2, 4, 160) and sorted(ze) == [4, 8] and ze[8].shape == (2, 2, 160)
  assert synthetic.flow_channels(hp) == [8, 8, 8, 8, 6, 6, 6, 6, 4, 4, 4, 4]


def test_stft_oracle_is_self_consistent():
  """oracle/stft_oracle.py (numpy restatement of stft.py / denoiser.py): the STFT pair reconstructs perfectly,
  strength 0 is the identity, and the host-side bases handed to the library equal the oracle's."""
  from oracle import stft_oracle as S
  from waveglow_amd.denoiser import stft_bases
  fwd, inv, wsq = S.bases()
  x = np.random.default_rng(0).standard_normal((2, 256 * 9)) * 0.3
  re, im = S.transform(x, fwd)
  assert re.shape == (2, 513, 10)
  assert np.abs(S.inverse(re, im, inv, wsq) - x).max() < 1e-12
  assert np.abs(S.denoise(x, np.ones(513), 0.0, fwd, inv, wsq) - x).max() < 1e-12
  d = S.denoise(x, np.full(513, 1e3), 1.0, fwd, inv, wsq)      # everything subtracted away
  assert np.abs(d).max() < 1e-9
  f32, i32, w32 = stft_bases()
  assert f32.flags["C_CONTIGUOUS"] and i32.flags["C_CONTIGUOUS"]
  np.testing.assert_allclose(f32, fwd, atol=1e-6)
  np.testing.assert_allclose(i32, inv, atol=1e-6)
  np.testing.assert_allclose(w32, wsq, atol=1e-6)


def test_training_weight_packing_reproduces_the_reference_forward():
  """Host logic of the training direction (tests/_packing.py: pack_weights) without the GPU: a plain-torch
  evaluation of exactly the matrices the library receives -- (pos,pos) permutation, tap-major K, cond slice as a
  K-segment, W_end folded into the skip rows, per-phase upsample matrices -- must reproduce the oracle's forward."""
  import torch
  from oracle import torch_oracle as O
  from _cases import oracle_cfg_from_hp
  from waveglow_amd import synthetic
  from waveglow_amd.hparams import HParams
  from waveglow_amd.model import WaveGlow
  from _packing import _perms, pack_weights, pos_perm, to_fragments, to_pos_order
  hp = HParams(n_channels=64, n_layers=3, n_flows=4, n_early_every=2)
  sd = synthetic.to_weightnorm_form(synthetic.make_state_dict(hp, seed=2))
  model = WaveGlow(hp)
  model.load_state_dict(sd)
  B, T = 2, 5
  mel = synthetic.make_mel(B, T, seed=9)
  S = 256 * T - 64
  wav = torch.rand(B, S, generator=torch.Generator().manual_seed(1)) * 0.6 - 0.3
  with torch.no_grad():
    C_, nl, M8 = hp.n_channels, hp.n_layers, hp.n_mel_channels * 8
    pm_ = _perms(C_, M8, torch.device("cpu"))
    packed = pack_weights(model)
    w1, b1, w2, b2, wes, wup, bup, start5, out_init, w1x1 = to_pos_order(packed, pm_)
    back = to_pos_order(to_pos_order(packed, pm_), pm_, inverse=True)       # the gradient path's inverse gathers
    assert all(torch.equal(a, b) for a, b in zip(packed, back))
    L = S // 8
    pc, pm = pos_perm(C_), pos_perm(M8)
    # upsample + squeeze through the per-phase matrices: spect[pos][b][t], t = 32 q + p
    melp = torch.nn.functional.pad(mel, (3, 0))                               # frames q-3 .. q
    spect = torch.zeros(M8, B, L)
    for t in range(L):
      p, q = t % 32, t // 32
      taps = torch.stack([torch.nn.functional.pad(melp[:, :, q + 3 - j], (0, 128 - hp.n_mel_channels)) for j in range(4)], 1)
      spect[:, :, t] = wup[p] @ taps.reshape(B, 512).t() + bup[:, None]
    audio = wav.view(B, L, 8).permute(0, 2, 1)                                # [B, 8, L]
    outs, log_s_all = [], []
    for k in range(model.n_flows):
      if k % hp.n_early_every == 0 and k > 0:
        outs.append(audio[:, :hp.n_early_size])
        audio = audio[:, hp.n_early_size:]
      c = audio.shape[1]
      h = c // 2
      audio = torch.einsum("rc,bcl->brl", w1x1[k, :c, :c], audio)
      a0, a1 = audio[:, :h], audio[:, h:]
      x = torch.einsum("pj,bjl->pbl", start5[k, :h].t(), a0) + start5[k, 4][:, None, None]     # [C pos, B, L]
      out = out_init[k][:, None, None].expand(8, B, L).clone()
      for i in range(nl):
        fl, d = k * nl + i, 2 ** i
        xp = torch.nn.functional.pad(x, (d, d))
        kin = torch.cat([xp[:, :, 0:L], xp[:, :, d:d + L], xp[:, :, 2 * d:2 * d + L], spect], 0)  # K = tap0|tap1|tap2|spect
        pre = torch.einsum("mk,kbl->mbl", w1[fl], kin) + b1[fl][:, None, None]
        acts = torch.tanh(pre[:C_]) * torch.sigmoid(pre[C_:])
        if i < nl - 1:
          x = x + torch.einsum("mk,kbl->mbl", w2[fl], acts) + b2[fl][:, None, None]
        out = out + torch.einsum("mk,kbl->mbl", wes[fl], acts)
      b_, ls = out[:h].permute(1, 0, 2), out[h:2 * h].permute(1, 0, 2)
      audio = torch.cat([a0, torch.exp(ls) * a1 + b_], 1)
      log_s_all.append(ls)
    outs.append(audio)
    z = torch.cat(outs, 1)
    dense = {k_: v.detach() for k_, v in model.dense_state().items()}
    z_ref, ls_ref, _ = O.forward_ref(dense, mel, wav, oracle_cfg_from_hp(hp))
  assert float((z - z_ref).abs().max()) < 2e-4
  for a, b in zip(log_s_all, ls_ref):
    assert float((a - b).abs().max()) < 2e-4
  # fragment order: element (t, b, s, h, r, j) = mat[32 b + chan_to_pos(r)][64 t + 32 h + 8 s + j]
  m = torch.arange(64 * 128, dtype=torch.float32).reshape(64, 128)
  f = to_fragments(m)
  c2p = lambda r: 16 * ((r >> 2) & 1) + 4 * (r >> 3) + (r & 3)
  for (t, b, s_, h_, r, j) in [(0, 0, 0, 0, 0, 0), (1, 1, 2, 1, 5, 3), (1, 0, 3, 0, 31, 7)]:
    assert float(f[t, b, s_, h_, r, j]) == float(m[32 * b + c2p(r), 64 * t + 32 * h_ + 8 * s_ + j])


def test_checkpoint_cadence_and_resume_bookkeeping():
  """utils.py:361-470 restated in waveglow_amd/training.py: which iterations save, and where a resumed run continues."""
  from waveglow_amd.training import (SaveIterationSettings, check_save_it, get_continue_batch_iteration,
                                     get_continue_epoch, iteration_to_batch_iteration, iteration_to_epoch, skip_batch)
  st = SaveIterationSettings(epochs=2, batch_iterations=5, save_first_iteration=True, save_last_iteration=True,
                             iters_per_checkpoint=3, epochs_per_checkpoint=1)
  saves = [it for it in range(1, 11) if check_save_it(iteration_to_epoch(it, 5), it, st)]
  assert saves == [1, 3, 5, 6, 9, 10]            # first, every 3rd, the last batch of every epoch, the last
  st2 = SaveIterationSettings(epochs=3, batch_iterations=4, save_first_iteration=False, save_last_iteration=False,
                              iters_per_checkpoint=0, epochs_per_checkpoint=2)
  assert [it for it in range(1, 13) if check_save_it(iteration_to_epoch(it, 4), it, st2)] == [8]
  assert iteration_to_epoch(1, 5) == 0 and iteration_to_epoch(5, 5) == 0 and iteration_to_epoch(6, 5) == 1
  assert iteration_to_batch_iteration(6, 5) == 0 and iteration_to_batch_iteration(10, 5) == 4
  # a checkpoint of iteration 7 with 5 batches per epoch continues in epoch 1 at batch 2
  assert get_continue_epoch(7, 5) == 1 and get_continue_batch_iteration(7, 5) == 2
  assert skip_batch(continue_batch_iteration=2, batch_iteration=1) and not skip_batch(continue_batch_iteration=2, batch_iteration=2)
  assert get_continue_epoch(0, 5) == 0 and get_continue_batch_iteration(0, 5) == 0


def test_slaney_mel_filterbank_and_mel_oracle():
  """librosa.filters.mel restated (taco_stft.py:66-73 calls it with sr 22050, n_fft 1024, 80 mels, 0-8000 Hz):
  closed-form anchors of the Slaney scale, triangle/area properties, and the numpy mel oracle on a pure tone."""
  import numpy as np
  from waveglow_amd.taco_stft import _hz_to_mel, _mel_to_hz, slaney_mel_filterbank
  from oracle import stft_oracle as S
  assert abs(float(_hz_to_mel(1000.0)) - 15.0) < 1e-12                      # linear part: 200/3 Hz per mel
  assert abs(float(_hz_to_mel(8000.0)) - (15.0 + np.log(8.0) / (np.log(6.4) / 27.0))) < 1e-9
  assert abs(float(_mel_to_hz(_hz_to_mel(4321.0))) - 4321.0) < 1e-9
  fb = slaney_mel_filterbank(22050, 1024, 80, 0.0, 8000.0)
  assert fb.shape == (80, 513) and fb.dtype == np.float32 and (fb >= 0).all()
  freqs = np.linspace(0, 11025, 513)
  assert (fb[:, freqs > 8000.0] == 0).all() and fb[:, 0].sum() == 0         # nothing above fmax; first triangle starts at 0 Hz
  centres = freqs[fb.argmax(axis=1)]
  assert (np.diff(centres) > 0).all()
  # Slaney normalisation: every triangle has (continuous) unit area -> discrete area within the bin quantisation
  area = fb.sum(axis=1) * (freqs[1] - freqs[0])
  assert np.all(np.abs(area - 1.0) < 0.35) and abs(area[40:].mean() - 1.0) < 0.02
  t = np.arange(8192) / 22050.0
  tone = 0.5 * np.sin(2 * np.pi * 2000.0 * t)[None, :]
  mel = S.mel_spectrogram(tone, fb)
  assert mel.shape == (1, 80, 8192 // 256 + 1)
  peak = int(mel[0, :, 10].argmax())
  assert abs(centres[peak] - 2000.0) < 80.0
  assert mel.min() >= np.log(1e-5) - 1e-12


def test_nvidia_state_dict_conversion(tmp_path):
  """converter/convert.py:37-94 on the safe route: a legacy ``weight_g / weight_v`` state_dict file becomes a checkpoint in
  the reference's dict format (published hparams, iteration 580000) that loads into the model; a pickled module is refused."""
  import torch
  from waveglow_amd import synthetic
  from waveglow_amd.checkpoint import CheckpointWaveglow
  from waveglow_amd.converter import convert_glow, convert_glow_files
  from waveglow_amd.hparams import HParams
  from waveglow_amd.model import WaveGlow
  hp = HParams(n_channels=64)                     # NVIDIA-shaped (12 flows, 8 layers) but narrow to keep the test light
  sd = synthetic.to_weightnorm_form(synthetic.make_state_dict(hp, seed=1))
  legacy = {}
  for k, v in sd.items():                          # old torch.nn.utils.weight_norm names
    k = k.replace("parametrizations.weight.original0", "weight_g").replace("parametrizations.weight.original1", "weight_v")
    legacy[k] = v
  src = tmp_path / "nvidia_like.pt"
  torch.save({"model": legacy}, src)
  ck = convert_glow(src)
  assert ck.iteration == 580000 and ck.get_hparams().n_flows == 12 and ck.get_hparams().segment_length == 16000
  m = WaveGlow(hp)
  m.load_state_dict(ck.state_dict)
  for k, v in m.state_dict().items():
    assert torch.equal(v, sd[k]), k
  dst = tmp_path / "580000.pt"
  convert_glow_files(src, dst, keep_orig=False)
  assert dst.is_file() and not src.exists()
  assert CheckpointWaveglow.load(dst, torch.device("cpu")).iteration == 580000
  bad = tmp_path / "module.pt"
  torch.save({"model": torch.nn.Linear(2, 2)}, bad)   # a pickled module: refused, never executed
  try:
    convert_glow(bad)
    assert False, "a pickled module must be refused"
  except RuntimeError as ex:
    assert "plain-tensor" in str(ex)


def test_wav_helpers_match_reference_fixture(tmp_path):
  """normalize_wav / convert_wav / float_to_wav / is_overamp against outputs of the reference's own audio_utils.py
  (tests/golden/make_golden_audio.py): bit-exact, incl. the bytes of the written wav file and the inputs the reference
  rejects with an AssertionError."""
  import os
  import numpy as np
  import pytest
  from waveglow_amd import audio as A
  fx = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "audio_utils.npz"))
  names = sorted({k.split("/")[0] for k in fx.files})
  assert len(names) == 9
  n_assert = 0
  for name in names:
    x = fx[f"{name}/in"]
    assert bool(A.is_overamp(x)) == bool(fx[f"{name}/is_overamp"]), name
    if bool(fx[f"{name}/normalize_asserts"]):
      n_assert += 1
      with pytest.raises(AssertionError):
        A.normalize_wav(x.copy())
      normalized = None
    else:
      normalized = A.normalize_wav(x.copy())
      ref = fx[f"{name}/normalized"]
      assert normalized.dtype == ref.dtype and np.array_equal(normalized, ref), name
    if x.dtype in (np.float32, np.float64):
      got = A.convert_wav(x.copy(), np.int16)
      assert got.dtype == np.int16 and np.array_equal(got, fx[f"{name}/as_int16"]), name
      p = tmp_path / f"{name}.wav"
      A.float_to_wav(normalized if normalized is not None else x, p)
      assert np.array_equal(np.frombuffer(p.read_bytes(), dtype=np.uint8), fx[f"{name}/wav_bytes"]), name
    else:
      got = A.convert_wav(x.copy(), np.float32)
      assert got.dtype == np.float32 and np.array_equal(got, fx[f"{name}/as_float32"]), name
  assert n_assert >= 1


def test_wn_kernel_fragment_orders():
  """The A-fragment orders of the WN-layer kernel as the training direction packs them on the device
  (tests/_packing.py: wn_forward_fragments, plain_fragments; include/waveglow_amd.h: wg_train_weights a1 / a1c / a2 /
  es / wat / wbt): every element of the packed tensors against the documented index map, on matrices whose entries encode
  their own (row, column)."""
  import torch
  from _packing import K_SIGM_SCALE, K_TANH_SCALE, _perms, plain_fragments, pos_perm, wn_forward_fragments
  Cc, M8, NW, FL = 64, 128, 2, 2
  MB = Cc // (32 * NW)
  pm = _perms(Cc, M8, torch.device("cpu"))
  K1 = 3 * Cc + M8
  rows = torch.arange(2 * Cc, dtype=torch.float32)
  cols = torch.arange(K1, dtype=torch.float32)
  w1 = (rows[:, None] * 0.001 + cols[None, :] * 1e-6 + 0.25).expand(FL, -1, -1).clone()
  w1[1] += 0.125
  b1 = torch.arange(FL * 2 * Cc, dtype=torch.float32).view(FL, 2 * Cc) * 0.01
  w2 = (torch.arange(Cc, dtype=torch.float32)[:, None] * 0.01 + torch.arange(Cc, dtype=torch.float32)[None, :] * 1e-4).expand(FL, -1, -1).clone()
  wes = (torch.arange(8, dtype=torch.float32)[:, None] * 0.1 + torch.arange(Cc, dtype=torch.float32)[None, :] * 1e-3).expand(FL, -1, -1).clone()
  a1, a1c, b1s, a2, es = wn_forward_fragments(w1, b1, w2, wes, pm, NW)
  nK = K1 // 64
  a = torch.cat([a1, a1c], 1).view(FL, nK, 2, NW, 2 * MB, 2, 64, 8)
  kpos = pm.k1                                            # natural K index stored at K position P
  scale = lambda m: K_TANH_SCALE if m < Cc else K_SIGM_SCALE
  for (f, ks, u1, w, mt, k2, lane, j) in [(0, 0, 0, 0, 0, 0, 0, 0), (1, 3, 1, 1, 1, 1, 37, 5), (0, nK - 1, 1, 0, 1, 0, 63, 7), (1, 1, 0, 1, 0, 1, 31, 2)]:
    r, hh = lane & 31, lane >> 5
    m = (0 if mt < MB else Cc) + 32 * (w * MB + (mt % MB)) + r
    P = 64 * ks + 32 * u1 + 16 * k2 + 8 * hh + j
    want = (w1[f, m, kpos[P]] * scale(m)).half()
    assert a[f, ks, u1, w, mt, k2, lane, j] == want, (f, ks, u1, w, mt, k2, lane, j)
  assert torch.allclose(b1s[1, 5], b1[1, 5] * K_TANH_SCALE) and torch.allclose(b1s[0, Cc + 3], b1[0, Cc + 3] * K_SIGM_SCALE)
  a2v = a2.view(FL, NW, MB, Cc // 16, 64, 8)
  pc = pos_perm(Cc)
  for (f, w, mb, k16, lane, j) in [(0, 0, 0, 0, 0, 0), (1, 1, 0, 3, 45, 6)]:
    r, hh = lane & 31, lane >> 5
    assert a2v[f, w, mb, k16, lane, j] == w2[f, 32 * (w * MB + mb) + r, pc[16 * k16 + 8 * hh + j]].half()
  esv = es.view(FL, Cc // 32, 64, 8)
  for (f, s_, lane, j) in [(0, 0, 3, 1), (1, 1, 9 + 16 * 2, 4)]:
    row, l4 = lane & 15, lane >> 4
    full = wes[f, row & 7, pc[32 * s_ + 8 * l4 + j]]
    hi = full.half()
    want = hi if row < 8 else (full - hi.float()).half()
    assert esv[f, s_, lane, j] == want
  # plain row blocks (dgrad GEMMs)
  mat = (torch.arange(Cc, dtype=torch.float32)[:, None] * 0.01 + torch.arange(128, dtype=torch.float32)[None, :] * 1e-4).expand(FL, -1, -1).half()
  pf = plain_fragments(mat, NW).view(FL, 2, 2, NW, MB, 2, 64, 8)
  for (f, ks, u1, w, mb, k2, lane, j) in [(0, 0, 0, 0, 0, 0, 0, 0), (1, 1, 1, 1, 0, 1, 50, 3)]:
    r, hh = lane & 31, lane >> 5
    assert pf[f, ks, u1, w, mb, k2, lane, j] == mat[f, 32 * (w * MB + mb) + r, 64 * ks + 32 * u1 + 16 * k2 + 8 * hh + j]


def test_batched_log_det_w_equals_per_flow_logdet():
  """waveglow_amd/train.py:_log_det_w pads every flow's 1x1 weight into an 8x8 identity and takes ONE batched logdet;
  values and gradients must equal the reference's per-flow ``B * L * torch.logdet(W)`` (model.py:63)."""
  import torch
  from waveglow_amd.hparams import HParams
  from waveglow_amd.model import WaveGlow
  from waveglow_amd.train import _log_det_w
  torch.manual_seed(3)
  model = WaveGlow(HParams(n_channels=64, n_layers=2))
  n = 7 * 125
  got = _log_det_w(model, n)
  assert len(got) == model.n_flows and all(t.dim() == 0 for t in got)
  want = [n * torch.logdet(model.convinv[k].conv.weight.squeeze()) for k in range(model.n_flows)]
  for k in range(model.n_flows):
    assert torch.allclose(got[k], want[k], rtol=1e-6, atol=1e-4), k
  coef = torch.linspace(0.5, 1.5, model.n_flows)
  g_got = torch.autograd.grad(sum(c * t for c, t in zip(coef, got)), [m.conv.weight for m in model.convinv])
  g_want = torch.autograd.grad(sum(c * t for c, t in zip(coef, want)), [m.conv.weight for m in model.convinv])
  for a, b in zip(g_got, g_want):
    assert a.shape == b.shape and torch.allclose(a, b, rtol=1e-5, atol=1e-5 * float(b.abs().max()))


def test_shape_runs_keep_flow_order():
  """tests/_packing.py: _shape_runs -- the per-flow small tensors (end, start, 1x1; model.py:165-176: c_k drops at
  the early outputs) are stacked per run of equal shape; concatenating the runs must give back flow order."""
  from _packing import _shape_runs
  assert _shape_runs([8, 8, 8, 8, 6, 6, 6, 6, 4, 4, 4, 4]) == [(8, [0, 1, 2, 3]), (6, [4, 5, 6, 7]), (4, [8, 9, 10, 11])]
  assert _shape_runs([4]) == [(4, [0])]
  runs = _shape_runs([8, 6, 8, 8])                  # a shape that comes back starts a new run: order is never permuted
  assert runs == [(8, [0]), (6, [1]), (8, [2, 3])]
  assert [k for _, ks in runs for k in ks] == [0, 1, 2, 3]


def test_console_script_entry_point_resolves():
  """pyproject.toml declares the reference's console script name (reference pyproject.toml:59-60) and it points at a
  callable that parses the reference's sub-commands."""
  import importlib
  import tomli
  with open(os.path.join(ROOT, "pyproject.toml"), "rb") as f:
    proj = tomli.load(f)
  target = proj["project"]["scripts"]["waveglow-cli"]
  mod_name, fn_name = target.split(":")
  fn = getattr(importlib.import_module(mod_name), fn_name)
  assert callable(fn)
  from waveglow_amd.cli import build_parser
  sub = build_parser()
  for cmd in ("synthesize", "synthesize-wav", "train", "continue-train"):
    with pytest.raises(SystemExit) as e:
      sub.parse_args([cmd, "--help"])
    assert e.value.code == 0


def test_stft_oracle_against_torch_stft():
  """oracle/stft_oracle.py (the checker of the HIP conv-STFT / denoiser / mel front-end) against torch.stft / torch.istft --
  an implementation that shares NOTHING with it (FFT, not the windowed Fourier-basis matrices that both the oracle and
  waveglow_amd.denoiser.stft_bases construct).  Same parameters as the reference's STFT (stft.py:98-132: hann, periodic,
  n_fft 1024, hop 256, reflect padding).  What is specific to the reference (window_sumsquare, crop, clamp, bias frame,
  compression) is pinned by its own outputs in tests/test_stft_ref_cpu.py."""
  from oracle import stft_oracle as S
  rng = np.random.default_rng(3)
  x = rng.standard_normal((2, 256 * 13)).astype(np.float64) * 0.3
  fwd, inv, win_sq = S.bases()
  re, im = S.transform(x, fwd)
  win = torch.hann_window(1024, periodic=True, dtype=torch.float64)
  X = torch.stft(torch.from_numpy(x), n_fft=1024, hop_length=256, win_length=1024, window=win, center=True,
                 pad_mode="reflect", return_complex=True)
  assert X.shape == (2, 513, 14) == re.shape
  assert np.abs(re - X.real.numpy()).max() < 1e-9 and np.abs(im - X.imag.numpy()).max() < 1e-9
  # inverse of a MODIFIED spectrum (what the denoiser feeds it): magnitudes reduced, phases kept
  mag = np.sqrt(re ** 2 + im ** 2)
  g = np.clip(mag - 0.2 * mag.mean(), 0.0, None) / np.maximum(mag, 1e-30)
  y = S.inverse(re * g, im * g, inv, win_sq)
  Y = torch.istft(torch.complex(torch.from_numpy(re * g), torch.from_numpy(im * g)), n_fft=1024, hop_length=256,
                  win_length=1024, window=win, center=True)
  assert y.shape == tuple(Y.shape) and np.abs(y - Y.numpy()).max() < 1e-9
  # and the product's own basis construction gives the same transform
  from waveglow_amd.denoiser import stft_bases
  pf = stft_bases()[0]
  pf = pf.double().numpy() if torch.is_tensor(pf) else np.asarray(pf, dtype=np.float64)
  ft = np.einsum("kn,bnf->bkf", pf.reshape(1026, 1024), np.stack(
      [np.pad(x, ((0, 0), (512, 512)), mode="reflect")[:, f * 256:f * 256 + 1024] for f in range(14)], axis=2))
  assert np.abs(ft[:, :513] - X.real.numpy()).max() < 1e-4 and np.abs(ft[:, 513:] - X.imag.numpy()).max() < 1e-4


def test_build_lists_every_header():
  """waveglow_amd/build.py keeps HEADERS by hand, and needs_build() compares only the listed files with the library: a
  header of csrc/ that is not listed could be edited without a rebuild."""
  from waveglow_amd import build
  on_disk = sorted(f for f in os.listdir(build.CSRC) if f.endswith(".h"))
  listed = sorted(h for h in build.HEADERS if os.sep not in h and "/" not in h)
  assert listed == on_disk
  assert all(os.path.isfile(os.path.join(build.CSRC, h)) for h in build.HEADERS)
