"""Streaming synthesis on the GPU: the chunks of a stream, concatenated, are BIT FOR BIT the whole-utterance audio (raw
and denoised; no tolerance anywhere in this file), for every chunk size, push pattern and model depth, alone and with
other sessions in the step; the two kernels of a step against torch slicing and numpy's conversion; the refusals."""
import numpy as np
import pytest
import torch

from waveglow_amd import _lib, synthetic
from waveglow_amd import streaming as S
from waveglow_amd.audio import convert_wav
from waveglow_amd.hparams import HParams
from waveglow_amd.model import WaveGlow

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
STRENGTH = 0.1          # large enough that the subtraction changes samples (asserted in _whole)
# name: (hparams, T, chunk_frames)
MODELS = {
  "A": (dict(n_flows=4, n_early_every=2, n_layers=4, n_channels=64), 40, 8),
  "B": (dict(n_flows=12, n_layers=8, n_channels=64), 230, 32),        # the full-depth halo, windows across many tiles
  "C": (dict(n_flows=4, n_layers=8, n_channels=256), 100, 16),        # the production width
}
_SYNTHS = {}


def _synth(name):
  """One Synthesizer per model for the whole module (the denoiser's bias spectrum costs a synthesis)."""
  if name not in _SYNTHS:
    from waveglow_amd.checkpoint import CheckpointWaveglow
    from waveglow_amd.synthesizer import Synthesizer
    hp = HParams(**MODELS[name][0])
    m = WaveGlow(hp)
    m.load_state_dict(synthetic.to_weightnorm_form(synthetic.make_state_dict(hp, seed=8)))
    _SYNTHS[name] = Synthesizer(CheckpointWaveglow.from_instances(m, None, hp, 3), device=torch.device(DEV))
  return _SYNTHS[name]


def _mel(synth, T, dtype=torch.float32, seed=11):
  return synthetic.make_mel(1, T, synth.hparams.n_mel_channels, seed=seed)[0].to(dtype)


def _drain(synth, s, chunks):
  while s.ready:
    (c,) = synth.stream_step([s], pcm=False)
    assert c is not None and c.start_sample == sum(x.raw.numel() for x in chunks)
    chunks.append(c)
  assert synth.stream_step([s], pcm=False) == [None]


def _stream(synth, mel, pieces, **kw):
  """Push ``mel`` in ``pieces`` frames at a time and take every chunk as soon as it is ready; ``ready`` must follow the
  planner after every push: chunk j exactly when (j + 1) C + Hr frames are in.  Returns (session, chunks)."""
  s = synth.open_stream(dtype=mel.dtype, **kw)
  chunks, at = [], 0
  assert s.ready == 0
  for t in pieces:
    s.push(mel[:, at:at + t] if at % 2 else mel[None, :, at:at + t].to(DEV))       # both layouts, host and device
    at += t
    assert s.ready == max(0, (at - s.Hr) // s.chunk_frames) - len(chunks)
    assert s.ready == sum(1 for j in range(len(chunks), at) if (j + 1) * s.chunk_frames + s.Hr <= at)
    _drain(synth, s, chunks)
  assert at == mel.shape[1] and not any(c.final for c in chunks)
  s.close()
  assert s.ready == -(-at // s.chunk_frames) - len(chunks) > 0
  _drain(synth, s, chunks)
  assert [c.final for c in chunks] == [False] * (len(chunks) - 1) + [True]
  assert s.emitted_frames == at and s.finished
  return s, chunks


def _whole(synth, mel, noise, strength, sigma=1.0):
  """(raw, denoised) of the whole-utterance calls on the stream's own noise, fp32 [256 T]."""
  with torch.no_grad():
    audio = synth.model.infer_with_noise(mel[None].to(DEV), noise[0], noise[1], sigma)
    den = synth.denoiser(audio, strength)[:, 0] if strength > 0 else audio.float()
  if strength > 0:
    assert float((den - audio.float()).abs().max()) > 1e-4 * float(audio.float().abs().max())
  return audio.float()[0], den[0]


def _check(synth, s, chunks, mel, strength):
  raw, den = _whole(synth, mel, s.noise(), strength)
  got_raw, got_den = torch.cat([c.raw for c in chunks]), torch.cat([c.denoised for c in chunks])
  assert got_raw.dtype == torch.float32 and got_raw.shape == raw.shape
  assert torch.equal(got_raw, raw)
  assert torch.equal(got_den, den)
  assert bool(torch.isfinite(got_den).all()) and float(got_raw.abs().max()) > 0


def _pieces(T, pattern):
  if pattern == "all":
    return [T]
  if pattern == "single":
    return [1] * T
  out, k = [], 0
  while sum(out) < T:                                    # uneven: 0, 3, 1, 7, 2, 11, ... frames, an empty push among them
    out.append(min((0, 3, 1, 7, 2, 11, 5)[k % 7], T - sum(out)))
    k += 1
  return out


@pytest.mark.parametrize("name,dtype", [("A", torch.float32), ("B", torch.float32), ("C", torch.float32),
                                        ("A", torch.float16)])
def test_stream_is_bit_identical(name, dtype):
  synth, (_, T, C) = _synth(name), MODELS[name]
  mel = _mel(synth, T, dtype)
  s, chunks = _stream(synth, mel, _pieces(T, "uneven"), denoiser_strength=STRENGTH, chunk_frames=C, seed=3)
  assert len(chunks) == -(-T // C)
  _check(synth, s, chunks, mel, STRENGTH)


@pytest.mark.parametrize("C", [1, 8, 13, 40, 64])
@pytest.mark.parametrize("strength", [0.0, STRENGTH])
def test_chunk_sizes(C, strength):
  synth, T = _synth("A"), MODELS["A"][1]
  mel = _mel(synth, T)
  s, chunks = _stream(synth, mel, _pieces(T, "uneven"), denoiser_strength=strength, chunk_frames=C, seed=4)
  _check(synth, s, chunks, mel, strength)
  if strength == 0:
    assert all(c.denoised is c.raw for c in chunks)


@pytest.mark.parametrize("pattern", ["all", "single", "uneven"])
def test_push_patterns(pattern):
  synth, (_, T, C) = _synth("A"), MODELS["A"]
  mel = _mel(synth, T)
  s, chunks = _stream(synth, mel, _pieces(T, pattern), denoiser_strength=STRENGTH, chunk_frames=C, seed=5)
  _check(synth, s, chunks, mel, STRENGTH)


def test_known_length_equals_infer():
  """With total_frames the noise is drawn as Synthesizer.infer draws it: the stream IS infer(mel, seed=7)."""
  synth, (_, T, C) = _synth("A"), MODELS["A"]
  mel = _mel(synth, T)
  ref = synth.infer(mel[None], denoiser_strength=STRENGTH, seed=7)
  chunks = list(synth.infer_stream(mel[None], chunk_frames=C, pcm=False, denoiser_strength=STRENGTH, seed=7))
  assert len(chunks) == T // C and chunks[-1].final and chunks[0].sampling_rate == ref.sampling_rate
  assert np.array_equal(torch.cat([c.raw for c in chunks]).cpu().numpy(), ref.wav)
  assert np.array_equal(torch.cat([c.denoised for c in chunks]).cpu().numpy(), ref.wav_denoised)
  assert not np.array_equal(ref.wav, ref.wav_denoised)


def test_open_ended_noise_is_the_sessions_own():
  """Open-ended sessions draw from their own generator: the same seed and pushes give the same noise whatever the global
  generator did in between, another seed gives other noise, and the global generator is not advanced."""
  synth, T = _synth("A"), 12
  mel = _mel(synth, T)

  def noise(seed):
    s = synth.open_stream(seed=seed, denoiser_strength=0.0)
    s.push(mel[:, :5])
    s.push(mel[:, 5:])
    return s.noise()
  torch.manual_seed(1)
  a = noise(9)
  state = torch.cuda.get_rng_state(torch.device(DEV))
  b = noise(9)
  assert torch.equal(state, torch.cuda.get_rng_state(torch.device(DEV)))
  c = noise(10)
  assert a[0].shape == (1, synth.model.n_remaining_channels, 32 * T) and len(a[1]) == synth.model.n_early_flows()
  assert torch.equal(a[0], b[0]) and all(torch.equal(x, y) for x, y in zip(a[1], b[1]))
  assert not torch.equal(a[0], c[0])


def test_several_sessions_in_one_step():
  """Three sessions at different chunk indices in one step: 3 frames without the denoiser, exactly 4 frames, 40 frames.
  Each gets the stream it gets alone and its whole-utterance audio; a session with nothing ready is left alone."""
  synth, C = _synth("A"), 8
  mels = [_mel(synth, T, seed=20 + T) for T in (3, 4, 40)]
  strengths = [0.0, STRENGTH, STRENGTH]

  def open_(i):
    return synth.open_stream(denoiser_strength=strengths[i], chunk_frames=C, seed=30 + i, total_frames=mels[i].shape[1])

  alone = []
  for i in range(3):
    s = open_(i)
    s.push(mels[i])
    s.close()
    chunks = []
    _drain(synth, s, chunks)
    _check(synth, s, chunks, mels[i], strengths[i])
    alone.append(chunks)
  ss = [open_(i) for i in range(3)]
  got = [[], [], []]

  def step():
    before = [(s.next_chunk, s.emitted_frames, s.frames) for s in ss]
    res = synth.stream_step(ss, pcm=False)
    for i, (s, c) in enumerate(zip(ss, res)):
      if c is None:
        assert (s.next_chunk, s.emitted_frames, s.frames) == before[i]
      else:
        got[i].append(c)
    return res
  assert step() == [None, None, None]
  ss[2].push(mels[2])
  ss[2].close()
  for _ in range(2):                                       # the long session is two chunks ahead ...
    r = step()
    assert r[0] is None and r[1] is None and r[2] is not None
  ss[0].push(mels[0])
  ss[1].push(mels[1][:, :2])
  ss[0].close()
  r = step()                                               # ... when the 3-frame one joins it,
  assert r[0] is not None and r[0].final and r[1] is None and r[2].start_sample == 2 * 256 * C
  ss[1].push(mels[1][:, 2:])
  ss[1].close()
  r = step()                                               # and three when the 4-frame one does
  assert r[0] is None and r[1] is not None and r[1].final and r[2].start_sample == 3 * 256 * C
  while ss[2].ready:
    step()
  assert step() == [None, None, None]
  for i in range(3):
    assert len(got[i]) == len(alone[i])
    for x, y in zip(got[i], alone[i]):
      assert (x.start_sample, x.final) == (y.start_sample, y.final)
      assert torch.equal(x.raw, y.raw) and torch.equal(x.denoised, y.denoised)
  with pytest.raises(_lib.WgError):                        # one strength per step
    a, b = synth.open_stream(denoiser_strength=0.1, total_frames=4), synth.open_stream(denoiser_strength=0.2, total_frames=4)
    for s in (a, b):
      s.push(mels[1])
      s.close()
    synth.stream_step([a, b])
  with pytest.raises(_lib.WgError):
    synth.stream_step([a, a])


# ---------------------------------------------------------------------------------------------- the two kernels
def _ties():
  """float32 y with y * 32767 exactly on k + 0.5 in float32 arithmetic, both signs, even and odd k."""
  k = np.arange(0, 32767, dtype=np.float32)
  y = ((k + np.float32(0.5)) / np.float32(32767)).astype(np.float32)
  y = y[y * np.float32(32767) == k + np.float32(0.5)]
  assert y.size > 1000 and (np.floor(y * np.float32(32767)) % 2 == 0).any() and (np.floor(y * np.float32(32767)) % 2 == 1).any()
  return np.concatenate([y, -y])


def _emit_rows():
  rng = np.random.default_rng(6)
  over = np.array([1.0, np.nextafter(np.float32(1), np.float32(2)), 1.5, -1.0, np.nextafter(np.float32(-1), np.float32(-2)),
                   -2.0, 0.99999994, 3e38, -3e38], dtype=np.float32)
  loud = rng.uniform(-1.2, 1.2, 9001).astype(np.float32)
  nan = rng.uniform(-1, 1, 600).astype(np.float32)
  nan[77] = np.nan
  inf = rng.uniform(-1, 1, 600).astype(np.float32)
  inf[599] = np.inf
  # (denoised row, offset, count, gain): aligned and unaligned offsets, counts that are no multiple of 8
  return [(_ties(), 0, None, 1.0), (_ties() * np.float32(2), 8, None, 0.5), (_ties() * np.float32(0.5), 3, None, 2.0),
          (np.tile(over, 3), 0, None, 1.0), (np.zeros(512, np.float32), 0, None, 1.0), (loud, 8, 8192, 0.5),
          (loud, 5, 8193, 2.0), (loud, 0, 1, 1.0), (loud, 16, 0, 1.0), (nan, 0, None, 1.0), (inf, 8, None, 1.0)]


def test_emit_against_numpy():
  rows = _emit_rows()
  rng = np.random.default_rng(7)
  crops, refs = [], []
  for den, off, count, gain in rows:
    count = den.size - off if count is None else count
    raw = (den + rng.uniform(-0.1, 0.1, den.size).astype(np.float32)).astype(np.float32)
    crops.append((torch.from_numpy(raw).to(DEV), torch.from_numpy(den).to(DEV), off, count, gain))
    refs.append((raw[off:off + count], den[off:off + count], gain))
  n_max = (max(c[3] for c in crops) + 7) // 8 * 8
  out = S.emit_enqueue(crops, n_max)
  pcm, stats = S.emit_read(out.cpu(), len(crops), n_max)
  for b, (raw, den, gain) in enumerate(refs):
    n = den.size
    assert not pcm[b, n:].any(), b
    finite = bool(np.isfinite(raw).all() and np.isfinite(den).all())
    assert stats[b, S.NON_FINITE] == (0.0 if finite else 1.0), b
    assert stats[b, 6] == 0 and stats[b, 7] == 0
    if n == 0:
      assert not stats[b].any()
      continue
    if not finite:
      continue
    g = den * np.float32(gain)
    assert g.dtype == np.float32
    want = convert_wav(np.clip(g, np.float32(-1), np.float32(1)), np.int16)
    assert np.array_equal(pcm[b, :n], want), b
    assert stats[b, S.RAW_MIN] == raw.min() and stats[b, S.RAW_MAX] == raw.max(), b
    assert stats[b, S.DEN_MIN] == den.min() and stats[b, S.DEN_MAX] == den.max(), b
    assert stats[b, S.CLIPPED] == np.count_nonzero((g > 1) | (g < -1)), b
  assert stats[3, S.CLIPPED] == 3 * 6 and stats[0, S.CLIPPED] == 0 and stats[6, S.CLIPPED] > 100
  assert set(np.unique(pcm[3, :27])) == {-32767, 32767}
  # raw and denoised may be the same tensor
  same = S.emit_enqueue([(c[1], c[1], c[2], c[3], c[4]) for c in crops[:9]], n_max)
  pcm2, stats2 = S.emit_read(same.cpu(), 9, n_max)
  assert np.array_equal(pcm2, pcm[:9]) and np.array_equal(stats2[:, 2:], stats[:9, 2:])
  assert np.array_equal(stats2[:, :2], stats2[:, 2:4])
  for bad in ([(crops[0][0], crops[0][1], 0, crops[0][0].numel() + 1, 1.0)], [(crops[0][0], crops[0][1], -1, 4, 1.0)]):
    with pytest.raises(_lib.WgError):
      S.emit_enqueue(bad, n_max)
  with pytest.raises(_lib.WgError):
    S.emit_enqueue(crops[:1], n_max + 4)


def test_nan_chunk_raises_naming_the_session():
  synth = _synth("A")
  mel = _mel(synth, 12)
  good, bad = (synth.open_stream(denoiser_strength=0.0, chunk_frames=8, total_frames=12, seed=i) for i in (1, 2))
  good.push(mel)
  bad.push(mel)
  bad.noise()[0][0, 0, 100] = float("nan")                          # a view of the session's own noise: frame 3 of chunk 0
  good.close(), bad.close()
  with pytest.raises(_lib.WgError, match=bad.name):
    synth.stream_step([good, bad])
  assert good.next_chunk == 0 and bad.next_chunk == 0              # nobody advanced
  c = synth.stream_step([good])[0]
  assert c.pcm.dtype == np.int16 and c.pcm.shape == (2048,) and not c.final


@pytest.mark.parametrize("case", ["f32", "f16", "f32-padded-mel", "f16-unaligned-noise"])
def test_gather_against_slicing(case):
  dtype = torch.float16 if case.startswith("f16") else torch.float32
  n_mel, n_rem, n_es, n_early, cap, w_max = 80, 4, 2, 2, 64, 16
  n_mel_out = 96 if "padded" in case else n_mel
  g = torch.Generator().manual_seed(12)
  shift = 1 if "unaligned" in case else 0                                   # sources off the 16-byte grid: element loads

  def source(rows, cols, lead):
    t = torch.randn((rows * (cols + 4) + 8,), generator=g).to(dtype).to(DEV)
    v = t[shift:shift + rows * (cols + 4 * shift)].view(rows, cols + 4 * shift)[:, :cols]
    return v[None] if lead else v
  streams = [(source(n_mel, cap, False), source(n_rem, 32 * cap, True), [source(n_es, 32 * cap, True) for _ in range(n_early)])
             for _ in range(3)]
  spans = [(0, w_max), (1, 1), (37, w_max), (37, 1), (1, 7), (0, 0)]
  windows = [streams[b % 3] + span for b, span in enumerate(spans)]
  B = len(windows)
  out = (torch.full((B, n_mel_out, w_max), float("nan"), dtype=dtype, device=DEV),
         torch.full((B, n_rem, 32 * w_max), float("nan"), dtype=dtype, device=DEV),
         [torch.full((B, n_es, 32 * w_max), float("nan"), dtype=dtype, device=DEV) for _ in range(n_early)])
  mel, z_init, z_early = S.gather_enqueue(windows, w_max, n_mel_out=n_mel_out, out=out)
  fresh = S.gather_enqueue(windows, w_max, n_mel_out=n_mel_out)
  for b, (m, zi, ze, start, count) in enumerate(windows):
    want = torch.zeros((n_mel_out, w_max), dtype=dtype, device=DEV)
    want[:n_mel, :count] = m[:, start:start + count]
    assert torch.equal(mel[b], want), b
    for got, src in [(z_init, zi)] + list(zip(z_early, ze)):
      want = torch.zeros(got.shape[1:], dtype=dtype, device=DEV)
      want[:, :32 * count] = src[0, :, 32 * start:32 * (start + count)]
      assert torch.equal(got[b], want), b
  assert torch.equal(fresh[0], mel) and torch.equal(fresh[1], z_init)
  assert all(torch.equal(x, y) for x, y in zip(fresh[2], z_early))
  for bad in ((60, 5), (-1, 4)):
    with pytest.raises(_lib.WgError):
      S.gather_enqueue([streams[0] + bad], w_max)
  with pytest.raises(_lib.WgError):
    S.gather_enqueue([streams[0] + (0, w_max + 1)], w_max)


# ---------------------------------------------------------------------------------------------- PCM path, refusals
@pytest.mark.parametrize("side_stream", [False, True])
def test_pcm_chunks(side_stream):
  """pcm=True chunks are numpy's conversion of the pcm=False chunks of a second identical session, on the default and on
  a non-default current stream."""
  synth, (_, T, C) = _synth("A"), MODELS["A"]
  mel = _mel(synth, T)
  ref = list(synth.infer_stream(mel, chunk_frames=C, pcm=False, denoiser_strength=STRENGTH, seed=2))
  peak = max(float(r.denoised.abs().max()) for r in ref)
  gain = 1.5 / peak                                        # loud enough that some samples clip (asserted)
  kw = dict(denoiser_strength=STRENGTH, chunk_frames=C, seed=2, total_frames=T, gain=gain)
  torch.cuda.synchronize()
  stream = torch.cuda.Stream(torch.device(DEV)) if side_stream else torch.cuda.current_stream(torch.device(DEV))
  with torch.cuda.stream(stream):
    s = synth.open_stream(**kw)
    s.push(mel)
    s.close()
    got = []
    while s.ready:
      got.append(synth.stream_step([s])[0])
  torch.cuda.synchronize()
  assert len(got) == len(ref) and got[-1].final
  clipped = 0
  for c, r in zip(got, ref):
    assert c.raw is None and c.denoised is None and c.start_sample == r.start_sample and c.final == r.final
    den, raw = r.denoised.cpu().numpy(), r.raw.cpu().numpy()
    g = den * np.float32(gain)
    assert np.array_equal(c.pcm, convert_wav(np.clip(g, np.float32(-1), np.float32(1)), np.int16))
    assert c.raw_min == float(raw.min()) and c.raw_max == float(raw.max())
    assert c.clipped == np.count_nonzero((g > 1) | (g < -1))
    assert c.sampling_rate == synth.hparams.sampling_rate
    clipped += c.clipped
  assert clipped > 0


def test_refusals():
  synth = _synth("A")
  mel = _mel(synth, 8)
  with pytest.raises(_lib.WgError):
    synth.open_stream(chunk_frames=0)
  with pytest.raises(_lib.WgError):
    synth.open_stream(total_frames=3)                                        # denoiser on (the default strength)
  s = synth.open_stream()
  for bad in (mel[:79], mel.half(), mel.double(), torch.empty((80, 4), device="meta"), mel[None, None], mel[0]):
    with pytest.raises(_lib.WgError):
      s.push(bad)
  assert s.frames == 0
  s.push(mel[:, :3])
  with pytest.raises(_lib.WgError):
    s.close()                                                                # 3 frames with the denoiser on
  s.push(mel[:, 3:4])
  s.close()                                                                  # 4 frames: the limit of the offline path
  with pytest.raises(_lib.WgError):
    s.push(mel[:, :1])                                                       # after close()
  assert s.ready == 1
  s = synth.open_stream(total_frames=6)
  s.push(mel[:, :5])
  with pytest.raises(_lib.WgError):
    s.push(mel[:, :2])                                                       # past total_frames
  with pytest.raises(_lib.WgError):
    s.close()                                                                # short of total_frames
  with pytest.raises(_lib.WgError):
    synth.open_stream(denoiser_strength=0.0).close()                         # not a frame
  one = synth.open_stream(denoiser_strength=0.0, total_frames=1, seed=5)     # strength 0: one frame works
  one.push(mel[:, :1])
  one.close()
  (c,) = synth.stream_step([one], pcm=False)
  assert c.final and torch.equal(c.raw, _whole(synth, mel[:, :1], one.noise(), 0.0)[0])
  other = _synth("C").open_stream(denoiser_strength=0.0, total_frames=1)
  other.push(mel[:, :1])
  other.close()
  with pytest.raises(_lib.WgError):
    synth.stream_step([other])                                               # another Synthesizer's session
