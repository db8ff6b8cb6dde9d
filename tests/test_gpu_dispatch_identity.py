"""GPU: the bit-identity promises of the README at the DISPATCHER'S OWN kernel choices.

Ragged synthesis, the ragged no-grad forward and the likelihood, streaming and the gradient paths each promise an utterance
the bits of its own call whatever batch or window it is computed in.  The two sides of such a comparison are calls of
different workload size, and the library picks its WN-layer kernel by workload size (``wg_plan``): 64- or 128-column tiles,
single tiles / pairs / the resident walk, the deep-prefetch kernel, the 16x16x32 MFMA loop.  Every other test of these
promises pins the choice for both sides; here nothing is pinned.  Every test asks ``wg_plan`` (with the device's CU count)
for shapes whose two sides run DIFFERENT kernels, fails if there are none up to B * Fp = 8192 rows, prints the two plans and
then compares bytes.  No tolerances, except the parameter-gradient sum bound of tests/_batch_independence.py in (d).
"""
import numpy as np
import pytest
import torch

import _batch_independence as BI
import _dirty
import _dispatch as D
import _hot as H
import test_gpu_batch_independence as TBI
import test_gpu_stream as TS
from waveglow_amd import synthetic
from waveglow_amd.hparams import HParams
from waveglow_amd.model import WaveGlow

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
SIGMA = 0.8
SEED = 8                         # of the synthetic weights (the stream model's too)
_MODELS = {}


@pytest.fixture(autouse=True)
def _the_dispatcher_decides(monkeypatch):
  D.clean_environment(monkeypatch)


def _n_cu():
  return int(torch.cuda.get_device_properties(torch.device(DEV)).multi_processor_count)


def _hp(channels):
  return HParams(n_channels=channels, n_layers=8, n_flows=4, n_early_every=2)


def _fresh(hp, sd):
  """A new model, so a new engine: WG_FORCE_BN and WG_NO_START_FOLD are read when the engine is created."""
  m = WaveGlow.remove_weightnorm(WaveGlow(hp))
  m.load_state_dict(sd)
  return m.to(DEV).eval()


def _model(channels):
  """One model per width for the module, created (and its engine with it) inside a test: no switch is set."""
  if channels not in _MODELS:
    hp = _hp(channels)
    m = _fresh(hp, synthetic.make_state_dict(hp, seed=SEED))
    m._get_engine(torch.device(DEV))
    _MODELS[channels] = m
  return _MODELS[channels]


def _batch_shape(channels, cls, direction):
  found = D.find_batch(channels, cls, _n_cu(), direction)
  assert found is not None, f"{channels} channels: no batch with B * Fp <= {D.MAX_ROWS} runs in the {cls} class on {_n_cu()} CUs"
  return found


def _crossing(channels, direction, big, small, what):
  """Assert that the two sides run different kernels, and print them."""
  cfg, n_cu = D.config(channels), _n_cu()
  p, q = D.plan(cfg, direction, *big, n_cu), D.plan(cfg, direction, *small, n_cu)
  print(f"{what}: {big[0]} x {big[1]} frames -- {D.describe(p)}  |  {small[0]} x {small[1]} frames -- {D.describe(q)}")
  assert not D.same_kernel(p, q), f"{what}: both sides run the same kernel"
  return p, q


# ---------------------------------------------------------------------------------------------- (a) ragged inference
def _utterance(hp, T, seed, dtype):
  mel = synthetic.make_mel(1, T, seed=seed).to(dtype)
  zi, ze = synthetic.make_noise(hp, 1, 32 * T, seed=seed + 500)
  return mel, zi.to(dtype), [ze[k].to(dtype) for k in sorted(ze, reverse=True)]


def _padded(utts, T):
  """Utterances padded to T frames; what lies behind an utterance must not matter: loud mel and noise there."""
  mel = torch.cat([torch.nn.functional.pad(u[0], (0, T - u[0].shape[2]), value=3.0) for u in utts])
  zi = torch.cat([torch.nn.functional.pad(u[1], (0, 32 * T - u[1].shape[2]), value=7.0) for u in utts])
  ze = [torch.cat([torch.nn.functional.pad(u[2][i], (0, 32 * T - u[2][i].shape[2]), value=-5.0) for u in utts])
        for i in range(len(utts[0][2]))]
  return mel, zi, ze


def _infer(model, mel, zi, ze, frames=None):
  with torch.no_grad():
    out = model.infer_with_noise(mel.to(DEV), zi.to(DEV), [z.to(DEV) for z in ze], SIGMA,
                                 frames=None if frames is None else torch.tensor(frames, dtype=torch.int32))
  torch.cuda.synchronize()
  return out


def _ragged_infer(model, hp, B, T, dtype, seed, lens=None, own=None):
  """The ragged call on B utterances of ``lens`` frames (utterance ``own[0]`` replaced by ``own[1]``)."""
  lens = D.lengths(B, T) if lens is None else lens
  utts = [_utterance(hp, t, seed + b, dtype) for b, t in enumerate(lens)]
  if own is not None:
    utts[own[0]] = own[1]
  out = _infer(model, *_padded(utts, T), frames=lens)
  assert out.shape == (B, 256 * T) and out.dtype == dtype
  return out, utts, lens


CROSSINGS = [(ch, cls) for ch in (64, 128, 256, 512) for cls in D.CLASSES[ch] if cls != "small"]


@pytest.mark.parametrize("dtype", [torch.float32, torch.float16], ids=["fp32", "fp16"])
@pytest.mark.parametrize("channels,cls", CROSSINGS)
def test_ragged_inference_against_batch_of_one_calls(channels, cls, dtype):
  """The first, the last and the shortest utterance of a batch in the middle / large class against their own calls, which
  run in the small class; zeros behind every length."""
  B, T = _batch_shape(channels, cls, D.INFER)
  model, hp = _model(channels), _hp(channels)
  out, utts, lens = _ragged_infer(model, hp, B, T, dtype, 40)
  assert max(lens) == lens[1] == T and min(lens) == lens[2]
  for b in sorted({0, B - 1, 2}):
    what = f"{channels} channels {cls} {dtype}: utterance {b} ({lens[b]} frames)"
    p, q = _crossing(channels, D.INFER, (B, T), (1, lens[b]), what)
    assert D.class_of(channels, p) == cls and D.class_of(channels, q) == "small", what
    one = _infer(model, *utts[b])
    assert bool(torch.isfinite(one).all()) and float(one.abs().max()) > 0
    _dirty.same_bytes(out[b, :256 * lens[b]], one[0], what)
    assert not out[b, 256 * lens[b]:].any(), what


@pytest.mark.parametrize("channels", [64, 128, 256])
def test_ragged_inference_middle_against_large(channels):
  """The same utterance in a batch of the middle class and in one of the large class, other neighbours in each."""
  (Bm, Tm), (Bl, Tl) = _batch_shape(channels, "middle", D.INFER), _batch_shape(channels, "large", D.INFER)
  p, q = _crossing(channels, D.INFER, (Bl, Tl), (Bm, Tm), f"{channels} channels large | middle")
  assert (D.class_of(channels, p), D.class_of(channels, q)) == ("large", "middle")
  model, hp = _model(channels), _hp(channels)
  t = min(Tm, Tl) - 3
  own = _utterance(hp, t, 7, torch.float32)
  lm, ll = D.lengths(Bm, Tm), D.lengths(Bl, Tl)
  lm[0], ll[Bl - 1] = t, t
  mid, _, _ = _ragged_infer(model, hp, Bm, Tm, torch.float32, 100, lm, (0, own))
  big, _, _ = _ragged_infer(model, hp, Bl, Tl, torch.float32, 200, ll, (Bl - 1, own))
  assert float(mid[0].abs().max()) > 0
  _dirty.same_bytes(big[Bl - 1, :256 * t], mid[0, :256 * t], f"{channels} channels: one utterance, large against middle")
  assert not mid[0, 256 * t:].any() and not big[Bl - 1, 256 * t:].any()


# ---------------------------------------------------------------------------------------------- (b) forward, likelihood
def _recording(T, seed):
  g = torch.Generator().manual_seed(seed + 900)
  return synthetic.make_mel(1, T, seed=seed), torch.rand(1, 256 * T, generator=g) * 0.6 - 0.3


def _ragged_forward(model, B, T, seed, lens, own=None):
  """(z, log_s, likelihood rows) of the ragged no-grad forward on recordings of ``lens`` frames, NaN behind each."""
  recs = [_recording(t, seed + b) for b, t in enumerate(lens)]
  if own is not None:
    recs[own[0]] = own[1]
  mel = torch.cat([torch.nn.functional.pad(r[0], (0, T - r[0].shape[2]), value=float("nan")) for r in recs]).to(DEV)
  audio = torch.cat([torch.nn.functional.pad(r[1], (0, 256 * (T - r[0].shape[2])), value=float("nan")) for r in recs]).to(DEV)
  z, log_s = model.forward_ragged(mel, audio, lens)
  rows = model.log_likelihood_enqueue(mel, audio, frames=lens, sigma=SIGMA)
  torch.cuda.synchronize()
  return z, log_s, rows, recs


def _same_forward(z, log_s, rows, b, t, z1, ls1, rows1, what):
  _dirty.same_bytes(z[b, :, :32 * t], z1[0, :, :32 * t], f"{what}: z")
  assert not z[b, :, 32 * t:].any(), what
  for k, (x, y) in enumerate(zip(log_s, ls1)):
    _dirty.same_bytes(x[b, :, :32 * t], y[0, :, :32 * t], f"{what}: log_s {k}")
    assert not x[b, :, 32 * t:].any(), (what, k)
  _dirty.same_bytes(rows[b], rows1[0], f"{what}: likelihood row")
  assert bool(torch.isfinite(rows[b]).all())


@pytest.mark.parametrize("channels,cls", [(ch, cls) for ch in (64, 256) for cls in ("middle", "large")])
def test_ragged_forward_and_likelihood_against_batch_of_one_calls(channels, cls):
  B, T = _batch_shape(channels, cls, D.FORWARD)
  model = _model(channels)
  lens = D.lengths(B, T)
  z, log_s, rows, recs = _ragged_forward(model, B, T, 40, lens)
  assert z.shape == (B, 8, 32 * T) and len(log_s) == 4 and rows.dtype == torch.float64
  for b in sorted({0, B - 1, 2}):
    what = f"{channels} channels {cls} forward: utterance {b} ({lens[b]} frames)"
    p, q = _crossing(channels, D.FORWARD, (B, T), (1, lens[b]), what)
    assert D.class_of(channels, p) == cls and D.class_of(channels, q) == "small", what
    mel1, audio1 = recs[b][0].to(DEV), recs[b][1].to(DEV)
    with torch.no_grad():
      z1, ls1, _ = model((mel1, audio1))
    rows1 = model.log_likelihood_enqueue(mel1, audio1, sigma=SIGMA)
    assert bool(torch.isfinite(z1).all()) and float(z1.abs().max()) > 0
    _same_forward(z, log_s, rows, b, lens[b], z1, ls1, rows1, what)


@pytest.mark.parametrize("channels", [64, 256])
def test_ragged_forward_middle_against_large(channels):
  (Bm, Tm), (Bl, Tl) = _batch_shape(channels, "middle", D.FORWARD), _batch_shape(channels, "large", D.FORWARD)
  p, q = _crossing(channels, D.FORWARD, (Bl, Tl), (Bm, Tm), f"{channels} channels forward large | middle")
  assert (D.class_of(channels, p), D.class_of(channels, q)) == ("large", "middle")
  model = _model(channels)
  t = min(Tm, Tl) - 3
  own = _recording(t, 7)
  lm, ll = D.lengths(Bm, Tm), D.lengths(Bl, Tl)
  lm[0], ll[Bl - 1] = t, t
  zm, lsm, rm, _ = _ragged_forward(model, Bm, Tm, 100, lm, (0, own))
  zl, lsl, rl, _ = _ragged_forward(model, Bl, Tl, 200, ll, (Bl - 1, own))
  _same_forward(zl, lsl, rl, Bl - 1, t, zm[0:1], [x[0:1] for x in lsm], rm[0:1], f"{channels} channels forward: large against middle")


# ---------------------------------------------------------------------------------------------- (c) streaming
_SYNTH = []


def _synth():
  if not _SYNTH:
    from waveglow_amd.checkpoint import CheckpointWaveglow
    from waveglow_amd.synthesizer import Synthesizer
    hp = HParams(**TS.MODELS["C"][0])                      # 256 channels, 8 layers, 4 flows
    assert (hp.n_channels, hp.n_layers, hp.n_flows) == (256, 8, 4)
    m = WaveGlow(hp)
    m.load_state_dict(synthetic.to_weightnorm_form(synthetic.make_state_dict(hp, seed=8)))
    _SYNTH.append(Synthesizer(CheckpointWaveglow.from_instances(m, None, hp, 3), device=torch.device(DEV)))
  return _SYNTH[0]


def _stream_plans(synth, T, cls, chunk):
  """The whole-utterance call in class ``cls``, the stream's windows in the small class."""
  cfg, n_cu = D.config_of(synth.hparams), _n_cu()
  s = synth.open_stream(denoiser_strength=TS.STRENGTH, chunk_frames=chunk, seed=3)
  window = chunk + s.Hl + s.Hr
  whole, win = D.plan(cfg, D.INFER, 1, T, n_cu), D.plan(cfg, D.INFER, 1, window, n_cu)
  print(f"stream of {T} frames: whole -- {D.describe(whole)}  |  windows of {window} frames -- {D.describe(win)}")
  assert D.class_of(256, whole) == cls and D.class_of(256, win) == "small" and not D.same_kernel(whole, win)
  return s


def _stream_length(cls):
  T = D.find_single(256, cls, _n_cu())
  assert T is not None, f"no utterance with Fp <= {D.MAX_ROWS} runs alone in the {cls} class on {_n_cu()} CUs"
  return T + 3                                             # not a multiple of the chunk: a short last chunk


@pytest.mark.parametrize("cls", ["middle", "large"])
def test_stream_against_the_whole_utterance(cls):
  synth, chunk = _synth(), 64
  T = _stream_length(cls)
  s = _stream_plans(synth, T, cls, chunk)
  mel = TS._mel(synth, T)
  s.push(mel)
  s.close()
  chunks = []
  TS._drain(synth, s, chunks)
  assert len(chunks) == -(-T // chunk) and chunks[-1].final
  raw, den = TS._whole(synth, mel, s.noise(), TS.STRENGTH)
  _dirty.same_bytes(torch.cat([c.raw for c in chunks]), raw, f"stream {cls}: raw audio")
  _dirty.same_bytes(torch.cat([c.denoised for c in chunks]), den, f"stream {cls}: denoised audio")
  assert bool(torch.isfinite(den).all()) and float(raw.abs().max()) > 0


def test_known_length_stream_against_infer():
  synth, chunk = _synth(), 64
  T = _stream_length("middle")
  _stream_plans(synth, T, "middle", chunk)
  mel = TS._mel(synth, T)
  ref = synth.infer(mel[None], denoiser_strength=TS.STRENGTH, seed=7)
  chunks = list(synth.infer_stream(mel[None], chunk_frames=chunk, pcm=False, denoiser_strength=TS.STRENGTH, seed=7))
  assert chunks[-1].final
  assert np.array_equal(torch.cat([c.raw for c in chunks]).cpu().numpy(), ref.wav)
  assert np.array_equal(torch.cat([c.denoised for c in chunks]).cpu().numpy(), ref.wav_denoised)
  assert not np.array_equal(ref.wav, ref.wav_denoised)


# ---------------------------------------------------------------------------------------------- (d) gradient paths
def _wide(name, frozen):
  """The wide case of tests/_batch_independence.py: its batch on 128-column tiles, an utterance alone on 64-column ones."""
  c = BI.case(name)
  cfg, n_cu = D.config_of(c.hp), _n_cu()
  batch, one = D.plan(cfg, D.TRAIN, c.B, c.T, n_cu), D.plan(cfg, D.TRAIN, 1, c.T, n_cu)
  print(f"{name}: batch {c.B} x {c.T} -- {D.describe(batch)}  |  alone -- {D.describe(one)}")
  assert (batch.block_n, one.block_n) == (128, 64), f"{name}: the batch and an utterance alone run the same tile width on {n_cu} CUs"
  model = WaveGlow(c.hp)
  model.load_state_dict(c.sd)
  model = model.to(DEV).train()
  if frozen:
    model.requires_grad_(False)
  return c, model


@pytest.mark.parametrize("name", ["c256_wide", "c64_wide"])
def test_training_direction_across_tile_widths(name):
  c, model = _wide(name, False)
  batch = TBI._train_call(model, c, None)
  singles = [TBI._train_call(model, c, b) for b in range(c.B)]
  BI.compare(batch, singles, c, "fwd", f"{name} training, unpinned")


@pytest.mark.parametrize("weight_grads", [False, True], ids=["frozen", "weight_grads"])
@pytest.mark.parametrize("name", ["c256_wide", "c64_wide"])
def test_synthesis_direction_across_tile_widths(name, weight_grads):
  c, model = _wide(name, not weight_grads)
  batch = TBI._synth_call(model, c, None, weight_grads)
  singles = [TBI._synth_call(model, c, b, weight_grads) for b in range(c.B)]
  BI.compare(batch, singles, c, "inv", f"{name} synthesis {'weight_grads' if weight_grads else 'frozen'}, unpinned")


# ---------------------------------------------------------------------------------------------- (e) both widths, trained range
SUBNORMAL = 2.0 ** -14           # below it an fp16 value is subnormal
LARGE = 1e4
SHARE = 0.01
# draw: (mel scale, noise scale of synthesis, audio scale of the forward)
DRAWS = {"trained": (1.0, 1.0, 1.0), "subnormal": (3.0, 1.0, 1.0), "large": (1.0, 1e4, 3e3)}


def _shares(direction, c, inputs):
  """Worst layer's share of subnormal and of large entries among the fp16 planes the layer GEMMs read (x and acts), in the
  emulation of tests/_hot.py."""
  trace = {}
  with torch.no_grad():
    w = H.compose({k: v.double() for k, v in c.sd.items()})
    P = H.Prec(True, trace=trace)
    if direction == "inv":
      out = H.infer(w, inputs[0].double(), inputs[1].double(), {k: v.double() for k, v in inputs[2].items()}, H.SIGMA, c.cfg, P)
    else:
      out = H.forward(w, inputs[0].double(), inputs[1].double(), c.cfg, P)[0]
  assert bool(torch.isfinite(out).all())
  planes = trace["x"] + trace["acts"]
  return (max(float(((t.abs() < SUBNORMAL) & (t != 0)).double().mean()) for t in planes),
          max(float((t.abs() > LARGE).double().mean()) for t in planes))


@pytest.mark.parametrize("draw", list(DRAWS))
def test_both_tile_widths_give_the_same_bits_at_trained_range(draw, monkeypatch):
  """hot_c256 (weights at the range of a trained vocoder) under WG_FORCE_BN = 128 (16x16x32 MFMAs) and 64 (32x32x16, deep
  prefetch): synthesis and the no-grad forward, byte for byte -- on the fixture's inputs, on a draw with at least 1 % of a
  layer's fp16 activations subnormal, and on one with at least 1 % above 1e4."""
  ms, ns, ws = DRAWS[draw]
  inv, fwd = H.Hot("hot_c256", "inv"), H.Hot("hot_c256", "fwd")
  syn = (inv.mel * ms, inv.z_init * ns, {k: v * ns for k, v in inv.z_early.items()})
  ana = (fwd.mel * ms, fwd.wav * ws)
  for direction, c, inputs in (("inv", inv, syn), ("fwd", fwd, ana)):
    sub, big = _shares(direction, c, inputs)
    print(f"hot_c256 {direction} {draw}: worst layer {100 * sub:.1f} % subnormal, {100 * big:.1f} % above {LARGE:g}")
    assert draw != "subnormal" or sub >= SHARE
    assert draw != "large" or big >= SHARE
  outs = {}
  for bn in ("128", "64"):
    monkeypatch.setenv("WG_FORCE_BN", bn)
    m_inv, m_fwd = _fresh(inv.hp, inv.sd), _fresh(fwd.hp, fwd.sd)
    audio = _infer_hot(m_inv, syn, inv.sigma)
    with torch.no_grad():
      z, log_s, _ = m_fwd((ana[0].to(DEV), ana[1].to(DEV)))
    torch.cuda.synchronize()
    outs[bn] = {"audio": audio, "z": z, **{f"log_s.{k}": t for k, t in enumerate(log_s)}}
    for q, t in outs[bn].items():
      assert bool(torch.isfinite(t).all()) and float(t.abs().max()) > 0, (bn, q)
  for q in outs["128"]:
    _dirty.same_bytes(outs["128"][q], outs["64"][q], f"hot_c256 {draw}: {q}, 128-column against 64-column tiles")


def _infer_hot(model, inputs, sigma):
  mel, zi, ze = inputs
  with torch.no_grad():
    return model.infer_with_noise(mel.to(DEV), zi.to(DEV), [ze[k].to(DEV) for k in sorted(ze, reverse=True)], sigma)


# ---------------------------------------------------------------------------------------------- (f) the helper can tell
def test_the_comparison_reports_two_paths_that_differ(monkeypatch):
  """One side of a crossing of (a) with WG_NO_START_FOLD=1 -- the first layer reads stored x_0 planes instead of rebuilding
  them, which tests/test_gpu_parity.py shows to differ in bits: the byte comparison of this file must say so."""
  channels = 256
  B, T = _batch_shape(channels, "middle", D.INFER)
  hp, sd = _hp(channels), synthetic.make_state_dict(_hp(channels), seed=SEED)
  out, utts, lens = _ragged_infer(_fresh(hp, sd), hp, B, T, torch.float32, 40)
  _crossing(channels, D.INFER, (B, T), (1, lens[0]), "fold against no fold")
  monkeypatch.setenv("WG_NO_START_FOLD", "1")
  one = _infer(_fresh(hp, sd), *utts[0])
  monkeypatch.delenv("WG_NO_START_FOLD")
  with pytest.raises(AssertionError, match="entries differ"):
    _dirty.same_bytes(out[0, :256 * lens[0]], one[0], "fold against no fold")
  _dirty.same_bytes(out[0, :256 * lens[0]], _infer(_fresh(hp, sd), *utts[0])[0], "fold against fold")
