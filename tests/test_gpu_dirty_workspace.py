"""GPU: no result depends on what a workspace, a saved-state buffer or an output buffer held before the call
(tests/_dirty.py).

Every case runs one whole call -- on objects of its own, so that every buffer is allocated inside the run -- with the
allocations of ``torch.empty`` starting from 0x00, from 0xFF and from 0x47, and once more with no hook at all; every output
must have the same bytes in all four runs.  The cached inference workspaces (``_Engine._ws`` and the workspace a captured
graph writes to) are dirtied between two calls on one engine as well.  Nothing here has a tolerance.

Parts of an output left out of the comparison, with the line of include/waveglow_amd.h each rests on: none.  (``dw2`` /
``db2`` of the last layer of each flow, header lines 595 and 724, are packed gradients the Python layer clears itself;
the per-parameter gradients compared here are written entirely.)
"""
import ctypes as C

import numpy as np
import pytest
import torch

import _batch_independence as BI
import _corners as K
import _dirty as D
import _pitch_cases
import _ragged_infer_grads as R
import _stoi_cases
import _stoi_loss_cases
from waveglow_amd import STOILoss, _lib, likelihood, metrics, pcm, resample, synthetic
from waveglow_amd.denoiser import Denoiser
from waveglow_amd.hparams import HParams
from waveglow_amd.model import WaveGlow, WaveGlowLoss
from waveglow_amd.stft_loss import MultiResolutionSTFTLoss
from waveglow_amd.taco_stft import TacotronSTFT, TSTFTHParams

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
SIGMA = BI.SIGMA
NAN = float("nan")

# id: (case of tests/_batch_independence.py or corner of tests/_corners.py, environment)
INFER = {
  "c64_l8": ("c64_l8", {}),
  "c64_l10": ("c64_l10", {}),
  "c256_l8-bn64": ("c256_l8", {"WG_FORCE_BN": "64"}),
  "c256_l8-bn128": ("c256_l8", {"WG_FORCE_BN": "128"}),
  "l1_c128": ("l1_c128", {}),
  "l1_c512": ("l1_c512", {}),
}
TRAIN = {"c64_l8": ("c64_l8", {}), "c256_l8-bn128": ("c256_l8", {"WG_FORCE_BN": "128"})}
CORNER_FRAMES = [6, 3]
MEL_LENS = [256 * t for t in (9, 40, 4, 31, 32)]          # test_mel_ragged_device_equals_single


@pytest.fixture(autouse=True)
def _poisoned_gradient_buffers(monkeypatch):
  monkeypatch.setenv("WG_TRAIN_POISON_GRADS", "1")


class Inputs:
  """Weights and inputs of one inference case, on the CPU, made once."""

  def __init__(self, name):
    self.name = name
    if name in BI.CASES:
      c = BI.case(name)
      self.hp, self.sd, self.B, self.T = c.hp, c.sd, c.B, c.T
      self.mel, self.z_init, self.z_early, self.wav = c.mel, c.z_init, c.z_early_list(slice(None)), c.wav
      self.frames = list(R.FRAMES[name])
    else:
      self.hp = HParams(**K.LAYOUTS[name])
      self.sd = synthetic.to_weightnorm_form(synthetic.make_state_dict(self.hp, seed=K.FIRST_SEED[name]))
      self.B, self.T = 2, 6
      self.mel = synthetic.make_mel(self.B, self.T, self.hp.n_mel_channels, seed=77)
      zi, ze = synthetic.make_noise(self.hp, self.B, 32 * self.T)
      self.z_init, self.z_early = zi, [ze[k] for k in sorted(ze, reverse=True)]
      g = torch.Generator().manual_seed(78)
      self.wav = torch.rand(self.B, 256 * self.T - 24, generator=g) * 1.2 - 0.6
      self.frames = list(CORNER_FRAMES)
    g = torch.Generator().manual_seed(79)
    self.full = torch.rand(self.B, 256 * self.T, generator=g) * 1.2 - 0.6       # audio of the ragged forward

  def model(self, train=False):
    m = WaveGlow(self.hp)
    m.load_state_dict(self.sd)
    m = m.to(DEV)
    return m.train() if train else m.eval()


_inputs = {}


def inputs(name):
  if name not in _inputs:
    _inputs[name] = Inputs(name)
  return _inputs[name]


def _env(monkeypatch, env):
  for k, v in env.items():
    monkeypatch.setenv(k, v)


def _nan_behind(t, frames, unit):
  t = t.clone()
  for b, f in enumerate(frames):
    t[b, ..., unit * f:] = NAN
  return t


def _dirty(model, pattern):
  """Between two calls on one engine: what the engine cached now holds ``pattern`` (0xFF in the run without a hook)."""
  assert D.dirty_cached(model._engine, D.ONES if pattern is None else pattern) >= 1


# ---------------------------------------------------------------------------------------------------------- inference
@pytest.mark.parametrize("ragged", [False, True], ids=["dense", "ragged"])
@pytest.mark.parametrize("dtype", [torch.float32, torch.float16], ids=["fp32", "fp16"])
@pytest.mark.parametrize("mode", list(INFER))
def test_inference(mode, dtype, ragged, monkeypatch):
  name, env = INFER[mode]
  _env(monkeypatch, env)
  x = inputs(name)
  frames = x.frames if ragged else None
  mel, zi, ze = x.mel, x.z_init, x.z_early
  if ragged:                                              # nothing behind a count is read
    mel, zi, ze = _nan_behind(mel, frames, 1), _nan_behind(zi, frames, 32), [_nan_behind(z, frames, 32) for z in ze]
  mel, zi, ze = mel.to(DEV, dtype), zi.to(DEV, dtype), [z.to(DEV, dtype) for z in ze]
  fr = torch.tensor(frames, dtype=torch.int32) if ragged else None

  def call(pattern):
    model = x.model()
    with torch.no_grad():
      first = model.infer_with_noise(mel, zi, ze, SIGMA, frames=fr)
      _dirty(model, pattern)
      second = model.infer_with_noise(mel, zi, ze, SIGMA, frames=fr)
    return {"audio": first, "audio after the cached workspace was dirtied": second}

  out = D.four_runs(monkeypatch, call, f"{mode} {dtype} {'ragged' if ragged else 'dense'}")
  a = out["audio"]
  D.same_bytes(a, out["audio after the cached workspace was dirtied"], "second call on the engine")
  assert bool(torch.isfinite(a).all()) and a.dtype == dtype
  for b in range(x.B):
    f = frames[b] if ragged else x.T
    assert a[b, :256 * f].any() and not a[b, 256 * f:].any(), b


@pytest.mark.parametrize("ragged", [False, True], ids=["dense", "ragged"])
@pytest.mark.parametrize("dtype", [torch.float32, torch.float16], ids=["fp32", "fp16"])
@pytest.mark.parametrize("mode", list(INFER))
def test_inference_graph_replays(mode, dtype, ragged, monkeypatch):
  """``graph=True``: the captured graph writes to the workspace of its warm-up call; three replays with that workspace
  dirtied in between, against the direct launch."""
  name, env = INFER[mode]
  _env(monkeypatch, env)
  x = inputs(name)
  frames = x.frames if ragged else None
  mel, zi, ze = x.mel.to(DEV, dtype), x.z_init.to(DEV, dtype), [z.to(DEV, dtype) for z in x.z_early]
  fr = torch.tensor(frames, dtype=torch.int32, device=DEV) if ragged else None

  def call(pattern):
    model = x.model()
    out = {}
    with torch.no_grad():
      for i in range(3):
        out[f"replay {i}"] = model.infer_with_noise(mel, zi, ze, SIGMA, frames=fr, graph=True)
        assert len(model._engine._graphs) == 1
        _dirty(model, pattern)
      out["direct"] = model.infer_with_noise(mel, zi, ze, SIGMA, frames=fr)
    return out

  out = D.four_runs(monkeypatch, call, f"{mode} graph {dtype} {'ragged' if ragged else 'dense'}")
  for i in range(3):
    D.same_bytes(out[f"replay {i}"], out["direct"], f"replay {i} against the direct launch")
  assert bool(torch.isfinite(out["direct"]).all()) and out["direct"].any()


# ------------------------------------------------------------------------------------ no-grad forward and likelihood
def _wg_loss_host(z, log_s, log_det, sigma):
  """wg_loss (log_det_W as host floats) on a 16-byte workspace from ``torch.empty``."""
  lib = _lib.load()
  n = len(log_s)
  ptrs = (C.c_void_p * n)(*[t.data_ptr() for t in log_s])
  sizes = (C.c_int64 * n)(*[t.numel() for t in log_s])
  ld = (C.c_float * n)(*[float(v) for v in log_det])
  out = torch.empty((), dtype=torch.float32, device=z.device)
  ws = torch.empty(16, dtype=torch.uint8, device=z.device)
  stream = torch.cuda.current_stream(z.device).cuda_stream
  _lib.check(lib.wg_loss(z.data_ptr(), z.numel(), ptrs, sizes, n, ld, float(sigma), out.data_ptr(), ws.data_ptr(), ws.numel(),
                         C.c_void_p(stream)))
  return out


@pytest.mark.parametrize("dtype", [torch.float32, torch.float16], ids=["fp32", "fp16"])
@pytest.mark.parametrize("mode", list(INFER))
def test_no_grad_forward_and_likelihood(mode, dtype, monkeypatch):
  """``model.forward`` under no_grad with ``WaveGlowLoss`` (wg_loss_dev) and wg_loss on its outputs, ``forward_ragged``, and
  ``wg_nll`` with the per-frame track on the dense and on the ragged outputs."""
  name, env = INFER[mode]
  _env(monkeypatch, env)
  x = inputs(name)
  mel, wav = x.mel.to(DEV, dtype), x.wav.to(DEV, dtype)
  mel_r = _nan_behind(x.mel, x.frames, 1).to(DEV, dtype)
  full_r = _nan_behind(x.full, x.frames, 256).to(DEV, dtype)

  def call(pattern):
    model = x.model()
    out = {}
    with torch.no_grad():
      z, log_s, log_det = model((mel, wav))
      out["z"] = z
      out.update({f"log_s.{k}": t for k, t in enumerate(log_s)})
      out["WaveGlowLoss"] = WaveGlowLoss(SIGMA)((z, log_s, log_det))
      if dtype == torch.float32:
        out["wg_loss"] = _wg_loss_host(z, log_s, log_det, SIGMA)
      _dirty(model, pattern)
      zr, lsr = model.forward_ragged(mel_r, full_r, x.frames)
      out["ragged z"] = zr
      out.update({f"ragged log_s.{k}": t for k, t in enumerate(lsr)})
      _dirty(model, pattern)
      eng, z32, ls32, none = likelihood._forward(model, mel, wav, None)
      rows, track = likelihood.nll_enqueue(eng, z32, ls32, none, SIGMA, per_frame=True)
      out["nll rows"], out["nll track"] = rows, track
      _dirty(model, pattern)
      eng, z32, ls32, fr = likelihood._forward(model, mel_r, full_r, x.frames)
      rows, track = likelihood.nll_enqueue(eng, z32, ls32, fr, SIGMA, per_frame=True)
      out["ragged nll rows"], out["ragged nll track"] = rows, track
      out["ragged nll rows alone"] = likelihood.nll_enqueue(eng, z32, ls32, fr, SIGMA)[0]
    return out

  out = D.four_runs(monkeypatch, call, f"{mode} {dtype} forward")
  assert bool(torch.isfinite(out["z"]).all()) and bool(torch.isfinite(out["WaveGlowLoss"]))
  if dtype == torch.float32:
    assert abs(float(out["wg_loss"]) - float(out["WaveGlowLoss"])) <= 1e-5 * max(1.0, abs(float(out["wg_loss"])))
  assert bool(torch.isfinite(out["nll rows"]).all()) and bool(torch.isfinite(out["ragged nll rows"]).all())
  D.same_bytes(out["ragged nll rows"], out["ragged nll rows alone"], "wg_nll with and without the track")
  for b, f in enumerate(x.frames):
    assert out["ragged z"][b, :, :32 * f].any() and not out["ragged z"][b, :, 32 * f:].any(), b
    assert bool(torch.isfinite(out["ragged nll track"][b, :f]).all()) and bool(torch.isnan(out["ragged nll track"][b, f:]).all())


# ---------------------------------------------------------------------------------- training direction on a new slot
def _grads(model, out, what):
  assert bool(model.grad_finite), f"{what}: non-finite gradients, or an entry of a (NaN-poisoned) gradient buffer left unwritten"
  for n, p in model.named_parameters():
    if p.requires_grad:
      assert p.grad is not None, (what, n)
      out["p/" + n] = p.grad.detach().clone()
  return out


def train_step(model, c, scale=1.0, what="training step"):
  """forward under autograd + backward on the case's batch (inputs and cotangents times ``scale``): z, log_s, the loss of
  ``WaveGlowLoss``, d mel, d audio and every parameter gradient."""
  model.zero_grad(set_to_none=True)
  model.grad_scale = c.scale_fwd
  m = c.mel.to(DEV).requires_grad_(True)
  a = (scale * c.wav).to(DEV).requires_grad_(True)
  z, log_s, log_det = model((m, a))
  nll = WaveGlowLoss(SIGMA)((z, log_s, log_det))
  (scale * BI.train_loss(c, slice(None), z, log_s, log_det) + nll).backward()
  out = {"z": z.detach(), "WaveGlowLoss": nll.detach(), "d mel": m.grad, "d audio": a.grad}
  out.update({f"log_s.{k}": t.detach() for k, t in enumerate(log_s)})
  return _grads(model, out, what)


@pytest.mark.parametrize("recompute", [False, True], ids=["full-save", "recompute"])
@pytest.mark.parametrize("mode", list(TRAIN))
def test_training_step_on_a_new_slot(mode, recompute, monkeypatch):
  """The slot of the training pool, the packed weights, the ``aux`` buffer of wg_train_prepare and every gradient buffer
  are new allocations here."""
  name, env = TRAIN[mode]
  _env(monkeypatch, env)
  x, c = inputs(name), BI.case(name)

  def call():
    model = x.model(train=True)
    model.recompute_activations = recompute
    return train_step(model, c)

  out = D.four_runs(monkeypatch, call, f"{mode} training step")
  for q, t in out.items():
    assert bool(torch.isfinite(t).all()), q
  assert out["d mel"].any() and out["d audio"].any()


# ------------------------------------------------------------------------------------------------ infer_differentiable
def synth_step(model, c, weight_grads, frames=None, scale=1.0, what="infer_differentiable"):
  """``infer_differentiable`` + backward on the case's batch (noise and cotangent times ``scale``, NaN behind the counts):
  audio, d mel, d z_init, d z_early and, with ``weight_grads``, every parameter gradient."""
  model.zero_grad(set_to_none=True)
  model.grad_scale = c.scale_inv
  mel, zi, ze, r = c.mel, scale * c.z_init, [scale * z for z in c.z_early_list(slice(None))], scale * c.r_audio
  if frames is not None:
    mel, zi, r = _nan_behind(mel, frames, 1), _nan_behind(zi, frames, 32), _nan_behind(r, frames, 256)
    ze = [_nan_behind(z, frames, 32) for z in ze]
  m, zi = mel.to(DEV).requires_grad_(True), zi.to(DEV).requires_grad_(True)
  ze = [z.to(DEV).requires_grad_(True) for z in ze]
  kw = {} if frames is None else {"frames": list(frames)}
  audio = model.infer_differentiable(m, SIGMA, z_init=zi, z_early=ze, weight_grads=weight_grads, **kw)
  assert audio.grad_fn is not None
  audio.backward(r.to(DEV))
  out = {"audio": audio.detach(), "d mel": m.grad, "d z_init": zi.grad}
  out.update({f"d z_early.{i}": z.grad for i, z in enumerate(ze)})
  return _grads(model, out, what)


@pytest.mark.parametrize("recompute", [False, True], ids=["full-save", "recompute"])
@pytest.mark.parametrize("ragged", [False, True], ids=["dense", "ragged"])
@pytest.mark.parametrize("weight_grads", [False, True], ids=["frozen", "weight_grads"])
@pytest.mark.parametrize("mode", list(TRAIN))
def test_infer_differentiable(mode, weight_grads, ragged, recompute, monkeypatch):
  name, env = TRAIN[mode]
  _env(monkeypatch, env)
  x, c = inputs(name), BI.case(name)
  frames = x.frames if ragged else None

  def call():
    model = x.model(train=True).requires_grad_(weight_grads)
    model.recompute_activations = recompute
    return synth_step(model, c, weight_grads, frames)

  out = D.four_runs(monkeypatch, call, f"{mode} infer_differentiable")
  for q, t in out.items():
    assert bool(torch.isfinite(t).all()), q
  assert any(q.startswith("p/") for q in out) == weight_grads
  for b in range(x.B):
    f = frames[b] if ragged else x.T
    assert out["audio"][b, :256 * f].any() and not out["audio"][b, 256 * f:].any() and not out["d mel"][b, :, f:].any(), b


# ---------------------------------------------------------------------------------------------------------- STFT family
def _audio(B, N, seed, lens=None):
  x = torch.rand((B, N), generator=torch.Generator().manual_seed(seed)) * 1.6 - 0.8
  if lens is not None:
    for b, n in enumerate(lens):
      x[b, n:] = NAN
  return x


def test_denoiser(monkeypatch):
  """The bias spectrum (``mag0_out`` of a transform-only call on the model's own bias audio), the dense call and the ragged
  one."""
  hp = HParams(n_channels=64, n_layers=4, n_flows=4, n_early_every=2)
  sd = synthetic.to_weightnorm_form(synthetic.make_state_dict(hp, seed=8))
  N = max(MEL_LENS)
  audio = _audio(len(MEL_LENS), N, 5).to(DEV)
  # lengths of the ragged denoiser are at least 1024 samples: 256 * 4 is the smallest
  padded = _audio(len(MEL_LENS), N, 5, MEL_LENS).to(DEV)

  def call():
    model = WaveGlow(hp)
    model.load_state_dict(sd)
    model = model.to(DEV).eval()
    den = Denoiser(model, hp, "zeros", DEV)
    return {"bias_spec": den.bias_spec, "dense": den(audio, 0.1), "ragged": den(padded, 0.1, MEL_LENS),
            "ragged, strength 0": den(padded, 0.0, MEL_LENS)}

  out = D.four_runs(monkeypatch, call, "denoiser")
  assert all(bool(torch.isfinite(t).all()) for t in out.values()) and out["bias_spec"].any()
  for b, n in enumerate(MEL_LENS):
    assert out["ragged"][b, 0, :n].any() and not out["ragged"][b, 0, n:].any(), b


def test_mel_front_end(monkeypatch):
  N = max(MEL_LENS)
  audio = _audio(len(MEL_LENS), N, 5)
  padded = _audio(len(MEL_LENS), N, 5, MEL_LENS).to(DEV)

  def call():
    taco = TacotronSTFT(TSTFTHParams(), DEV)
    mel, frames, frames_dev = taco.mel_spectrogram_ragged_device(padded, MEL_LENS)
    return {"dense": taco.mel_spectrogram(audio), "odd length": taco.mel_spectrogram(audio[:2, :3000]), "ragged": mel,
            "frames": frames_dev, "differentiable, no graph": taco.mel_spectrogram_differentiable(padded.nan_to_num(0.0))}

  out = D.four_runs(monkeypatch, call, "mel front-end")
  assert all(bool(torch.isfinite(t).all()) for q, t in out.items() if q != "frames")
  for b, n in enumerate(MEL_LENS):
    assert out["ragged"][b, :, :n // 256 + 1].any() and not out["ragged"][b, :, n // 256 + 1:].any(), b


@pytest.mark.parametrize("ragged", [False, True], ids=["dense", "lengths"])
def test_mel_front_end_gradient(ragged, monkeypatch):
  """``mel_spectrogram_differentiable`` forward plus backward, twice under retain_graph (the backward must leave the saved
  state of its forward intact)."""
  N = max(MEL_LENS)
  lens = MEL_LENS if ragged else None
  audio = _audio(len(MEL_LENS), N, 5, lens).to(DEV)
  g = torch.randn((len(MEL_LENS), 80, N // 256 + 1), generator=torch.Generator().manual_seed(6)).to(DEV)
  if ragged:
    g = _nan_behind(g, [n // 256 + 1 for n in MEL_LENS], 1)

  def call():
    taco = TacotronSTFT(TSTFTHParams(), DEV)
    y = audio.clone().requires_grad_(True)
    mel = taco.mel_spectrogram_differentiable(y, lens) if ragged else taco.mel_spectrogram_differentiable(y)
    mel.backward(g, retain_graph=True)
    first = y.grad.clone()
    y.grad = None
    mel.backward(g)
    return {"mel": mel.detach(), "d audio": first, "d audio, second backward": y.grad}

  out = D.four_runs(monkeypatch, call, f"mel gradient {'lengths' if ragged else 'dense'}")
  D.same_bytes(out["d audio"], out["d audio, second backward"], "second backward")
  assert bool(torch.isfinite(out["d audio"]).all()) and bool(torch.isfinite(out["mel"]).all())
  for b, n in enumerate(MEL_LENS if ragged else [N] * len(MEL_LENS)):
    assert out["d audio"][b, :n].any() and not out["d audio"][b, n:].any(), b


# N = 256 * 13 = 3328 samples, smallest hop 50: the short utterances of the first set end inside the first 64-frame
# workgroup of every resolution; in the second set utterance 1 has 1550 / 50 + 1 = 32 frames and utterance 2
# 3150 / 50 + 1 = 64 frames of the smallest hop -- they end exactly on the 32-frame and the 64-frame boundary -- and
# utterance 3 one frame behind the first (33).  Every length is above max n_fft / 2 = 1024.
STFT_N = 256 * 13
STFT_LENS = {"dense": None, "lengths": [256 * t for t in (13, 5, 7, 9)], "boundaries": [STFT_N, 1550, 3150, 1600]}


@pytest.mark.parametrize("backward", [False, True], ids=["forward", "forward+backward"])
@pytest.mark.parametrize("lens_id", list(STFT_LENS))
def test_stft_loss(lens_id, backward, monkeypatch):
  lens = STFT_LENS[lens_id]
  assert lens is None or (len(lens) == 4 and all(1024 < n <= STFT_N for n in lens))
  x = (0.5 * _audio(4, STFT_N, 21, lens)).to(DEV)
  y = (0.5 * _audio(4, STFT_N, 22, lens)).to(DEV)
  kw = {} if lens is None else {"lengths": lens}

  def call():
    crit = MultiResolutionSTFTLoss(device=DEV)
    if not backward:
      with torch.no_grad():
        sc, mag = crit.terms(x, y, **kw)
        return {"sc": sc, "mag": mag, "loss": crit(x, y, **kw)}
    xg = x.clone().requires_grad_(True)
    loss = crit(xg, y, **kw)
    loss.backward(retain_graph=True)
    first = xg.grad.clone()
    xg.grad = None
    loss.backward()
    return {"loss": loss.detach(), "d audio": first, "d audio, second backward": xg.grad}

  out = D.four_runs(monkeypatch, call, f"stft loss {lens_id}")
  assert all(bool(torch.isfinite(t).all()) for t in out.values()) and float(out["loss"]) > 0.0
  if backward:
    D.same_bytes(out["d audio"], out["d audio, second backward"], "second backward")
    for b, n in enumerate(lens or [STFT_N] * 4):
      assert out["d audio"][b, :n].any() and not out["d audio"][b, n:].any(), b


# --------------------------------------------------------------------------------------------------- validation metrics
def test_mel_metrics(monkeypatch):
  """``mfcc``, ``dtw_distance`` and ``mel_metrics`` on the pairs of tests/test_gpu_metrics.py, and one 2100 x 5 pair:
  ``dtw_kernel<3>`` (three rows per thread), which no other test instantiates, against the oracle as ``_check_dtw`` does."""
  import test_gpu_metrics as TM
  a, b, _ = TM.small_mels()
  ma, ta = TM._pad(a)
  mb, tb = TM._pad(b)
  big = TM.feature_case(500, 16, 2100, 5)
  assert (2100 + 1023) // 1024 == 3
  fa, fta = TM._pad([big[0]])
  fb, ftb = TM._pad([big[1]])

  def call():
    TM._check_dtw([big])
    feat_a, feat_b = metrics.mfcc(ma, ta), metrics.mfcc(mb, tb)
    cost, frames = metrics.dtw_distance(feat_a, ta, feat_b, tb)
    big_cost, big_frames = metrics.dtw_distance(fa, fta, fb, ftb)
    wide_cost, wide_frames = metrics.dtw_distance(fb, ftb, fa, fta)          # 5 x 2100: one row per thread, a long walk
    return {"mfcc a": feat_a, "mfcc b": feat_b, "dtw cost": cost, "dtw frames": frames, "2100 x 5 cost": big_cost,
            "2100 x 5 frames": big_frames, "5 x 2100 cost": wide_cost, "5 x 2100 frames": wide_frames,
            "mel_metrics rows": metrics.mel_metrics_enqueue(ma, ta, mb, tb)}

  out = D.four_runs(monkeypatch, call, "mel metrics")
  assert not torch.isnan(out["mel_metrics rows"]).any() and int(out["2100 x 5 frames"][0]) == big[2][1]


def test_pitch_metrics(monkeypatch):
  import test_gpu_pitch as TP
  a, b = _pitch_cases.signals()
  lens = list(_pitch_cases.RAGGED)
  xa, xb = TP._batch(a, lens, fill=np.nan), TP._batch(b, lens, fill=np.nan)

  def call():
    out = {"rows": metrics.pitch_metrics_enqueue(xa, lens, xb, lens)}
    for q, t in zip(("f0", "aperiodicity", "frames"), metrics.yin_f0(xb, lens)):
      out[f"ragged {q}"] = t
    for case, (params, n) in _pitch_cases.CASES.items():
      for q, t in zip(("f0", "aperiodicity", "frames"), metrics.yin_f0(TP._batch(a, [n]), **params)):
        out[f"{case} {q}"] = t
    return out

  out = D.four_runs(monkeypatch, call, "pitch metrics")
  assert out["ragged frames"].tolist() == [0, 1, 2, 19] and out["ragged f0"][3].any()
  assert not torch.isnan(out["ragged f0"]).any() and not torch.isnan(out["rows"][3]).any()


def test_stoi(monkeypatch):
  """``stoi`` / ``estoi`` on the three lengths of tests/_stoi_cases.py at 20 dB as one ragged batch (NaN behind the lengths),
  and every case's pair alone."""
  import test_gpu_stoi_loss as TS
  pairs = [_stoi_cases.pair(n, 20.0) for n in _stoi_cases.LENGTHS]
  xs, ys = [p[0] for p in pairs], [p[1] for p in pairs]
  xb, yb, lens = TS._batch(xs), TS._batch(ys), [len(x) for x in xs]
  clean = TS._batch([_stoi_cases.pair(_stoi_cases.LENGTHS[2], None)[0]])
  noisy = TS._batch([_stoi_cases.pair(_stoi_cases.LENGTHS[2], -5.0)[1]])

  def call():
    return {"rows": metrics.stoi_enqueue(xb, lens, yb, lens), "y is x": metrics.stoi_enqueue(clean, None, clean, None),
            "-5 dB": metrics.stoi_enqueue(clean, None, noisy, None)}

  out = D.four_runs(monkeypatch, call, "stoi")
  assert not torch.isnan(out["rows"][:, :2]).any() and float(out["y is x"][0, 0]) > 0.999


def test_stoi_loss(monkeypatch):
  """wg_stoi_forward + wg_stoi_backward on the cases of tests/_stoi_loss_cases.py, alone and as one ragged batch with an
  utterance without a segment, and ``STOILoss`` forward plus backward through the resampler."""
  import test_gpu_stoi_loss as TS
  names = _stoi_loss_cases.NAMES + ("short",)
  xs, ys = [_stoi_loss_cases.pair(n)[0] for n in names], [_stoi_loss_cases.pair(n)[1] for n in names]
  xb, yb, lens = TS._batch(xs, pitch=7000), TS._batch(ys, pitch=7000), [len(x) for x in xs]
  x22, y22 = (t.copy() for t in _stoi_loss_cases.pair_22k())
  lens22 = list(_stoi_loss_cases.LENGTHS_22K)
  for b, n in enumerate(lens22):
    x22[b, n:] = np.nan
    y22[b, n:] = np.nan
  target, audio = torch.from_numpy(x22).to(DEV), torch.from_numpy(y22).to(DEV)

  def call():
    out = {}
    rows, state = metrics.stoi_forward_saved(xb, lens, yb, lens)
    out["rows"] = rows
    out["d y"] = metrics.stoi_backward_enqueue(state, TS._g_rows(len(names)))
    out["d y, second backward"] = metrics.stoi_backward_enqueue(state, TS._g_rows(len(names)))
    for n, x, y in zip(names, xs, ys):
      r1, s1 = metrics.stoi_forward_saved(TS._batch([x]), None, TS._batch([y]), None)
      out[f"{n} rows"], out[f"{n} d y"] = r1, metrics.stoi_backward_enqueue(s1, TS._g_rows(1))
    crit = STOILoss(sampling_rate=_stoi_loss_cases.SR, factor_stoi=TS.G[0], factor_estoi=TS.G[1], device=DEV)
    leaf = audio.clone().requires_grad_(True)
    loss = crit(leaf, target, lens22)
    loss.backward()
    out["STOILoss"], out["STOILoss d audio"] = loss.detach(), leaf.grad
    return out

  out = D.four_runs(monkeypatch, call, "stoi loss")
  D.same_bytes(out["d y"], out["d y, second backward"], "second backward on one saved state")
  assert not torch.isnan(out["d y"]).any() and not torch.isnan(out["STOILoss d audio"]).any()
  for b, n in enumerate(names):
    D.same_bytes(out["d y"][b:b + 1, :lens[b]], out[f"{n} d y"], f"{n}: row of the batch against its own call")
    assert not out["d y"][b, lens[b]:].any()
    assert out["d y"][b].any() == (n not in ("silent", "short")), n


# ------------------------------------------------------------------------------------------ outputs only (no workspace)
def test_outputs_without_a_workspace(monkeypatch):
  """``pcm`` finishing (its workspace holds the per-chunk extrema), the ``device_data`` gather, ``resample`` and its
  backward: every entry of their outputs is written."""
  import test_gpu_device_data as TD
  N = 256 * 40
  lens = [N, 256 * 9 + 8, 8, 256 * 31 + 16, 1]
  raw = (2.5 * _audio(5, N, 31)).to(DEV)
  den = _audio(5, N, 32).to(DEV)
  lens_dev = torch.tensor(lens, dtype=torch.int32, device=DEV)
  pool, offsets = TD._pool(np.int16)
  picks = [p for pair in zip(TD.INVALID[520], TD.VALID[520]) for p in pair]
  d_pool, d_off = torch.from_numpy(pool).to(DEV), torch.from_numpy(offsets).to(DEV)
  d_picks = torch.tensor(picks, dtype=torch.int32).reshape(-1, 2).to(DEV)
  x22 = _audio(3, 3000, 33, [3000, 1777, 1]).to(DEV)
  lens22 = [3000, 1777, 1]
  lens22_dev = torch.tensor(lens22, dtype=torch.int32, device=DEV)

  def call():
    out = {"pcm and statistics": pcm.finish_enqueue(raw, den, lens_dev)}
    rows = torch.empty((len(picks), 520), dtype=torch.float32, device=DEV)
    status = torch.zeros(1, dtype=torch.int32, device=DEV)
    _lib.check(_lib.load().wg_data_gather(d_pool.data_ptr(), _lib.WG_PCM_I16, pool.size, d_off.data_ptr(), len(offsets) - 1,
                                          d_picks.data_ptr(), rows.data_ptr(), status.data_ptr(), len(picks), 520,
                                          C.c_void_p(torch.cuda.current_stream(DEV).cuda_stream)))
    out["gathered rows"], out["gather status"] = rows, status
    for sr_out in (10000, 44100, 22050):
      y = resample.resample_enqueue(x22, lens22_dev, 22050, sr_out)
      out[f"resample to {sr_out}"] = y
      g = torch.ones_like(y)
      out[f"resample backward from {sr_out}"] = resample.resample_backward_enqueue(g, lens22_dev, 22050, sr_out, 3000)
    leaf = x22.clone().requires_grad_(True)
    y, _ = resample.resample_differentiable(leaf, lens22, 22050, 10000)
    y.nan_to_num(0.0).sum().backward()
    out["resample_differentiable"], out["resample_differentiable d audio"] = y.detach(), leaf.grad
    return out

  out = D.four_runs(monkeypatch, call, "outputs without a workspace")
  assert int(out["gather status"]) == 1
  for q, t in out.items():
    if t.dtype.is_floating_point:
      assert not torch.isnan(t).any(), q
