"""GPU checks of the per-utterance likelihood: the ragged no-grad forward (wg_forward with frames) against batch-of-one calls of
the dense one, the fp64 reduction (wg_nll) against the numpy restatement tests/_likelihood_oracle.py on the device's own z
and log_s, the dense batch against WaveGlowLoss, the golden cases of the reference, and ``validate --likelihood``."""
import numpy as np
import pytest
import torch

import _likelihood_oracle as oracle
import _pitch_cases
from _cases import Case
from waveglow_amd import HParams, WaveGlow, WaveGlowLoss, likelihood, synthetic

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
LIKELIHOOD = ["NLL (nats/sample)", "Bits per sample", "z variance", "# Likelihood frames"]
# |device - oracle| of every figure of a row, relative to the magnitude (sum z^2 / (2 sigma^2) + sum |log_s| + |log_det|) / n_b
# of the terms: the order of an fp64 summation over at most 1e5 terms (2^-53 * 1e5 = 1.1e-11 at the very worst)
ORDER_TOL = 1e-10
# Per-utterance |nll - nll of the reference's own fwd_* arrays| over the golden cases c64, c256, c512 (no earlier figure covers
# it; the batch-weighted mean keeps the project's 2e-3).  The bar is twice the worst value measured:
# the arithmetic is deterministic, the margin is for toolchain changes only.
UTTERANCE_NLL_WORST = 1.009e-5  # measured: c64 2.523e-06, c256 1.009e-05, c512 4.264e-09 (one utterance)
UTTERANCE_NLL_TOL = 2 * UTTERANCE_NLL_WORST


def build_model(hp, sd, normed=False):
  m = WaveGlow(hp)
  if normed:
    m.load_state_dict(synthetic.to_weightnorm_form(sd))
  else:
    m = WaveGlow.remove_weightnorm(m)
    m.load_state_dict(sd)
  return m.to(DEV).eval()


def _audio(n, seed):
  g = torch.Generator().manual_seed(seed)
  return torch.rand(1, n, generator=g) * 0.6 - 0.3


def _ragged_batch(lens, dtype=torch.float32):
  """Padded (mel, audio) of utterances of ``lens`` frames with NaN behind each, and the single (mel_b, audio_b) pairs."""
  Tm, B = max(lens), len(lens)
  mel = torch.full((B, 80, Tm), float("nan"))
  audio = torch.full((B, 256 * Tm), float("nan"))
  singles = []
  for b, T in enumerate(lens):
    m1, a1 = synthetic.make_mel(1, T, seed=40 + b), _audio(256 * T, 90 + b)
    mel[b, :, :T] = m1[0]
    audio[b, :256 * T] = a1[0]
    singles.append((m1.to(DEV, dtype), a1.to(DEV, dtype)))
  return mel.to(DEV, dtype), audio.to(DEV, dtype), singles


def _logdets(model):
  """log|det W_k| per column, fp64."""
  return [float(np.linalg.slogdet(c.conv.weight.detach().double().cpu().numpy()[:, :, 0])[1]) for c in model.convinv]


# ------------------------------------------------------------------------------------------- ragged forward
# the 1-frame utterance: the dense forward takes a single frame (audio_len 256 under one mel frame), so 1 is the smallest count
@pytest.mark.parametrize("channels,force_bn,dtype,lens", [
  (64, None, torch.float32, [37, 5, 64, 21]),
  (256, "128", torch.float32, [37, 5, 64, 21]),
  (256, "64", torch.float32, [37, 5, 64, 21]),
  (512, None, torch.float32, [37, 5, 64, 21]),
  (64, None, torch.float16, [37, 5, 64, 21]),
  (64, None, torch.float32, [1, 9, 3]),
])
def test_ragged_forward_equals_batch_of_one_calls(channels, force_bn, dtype, lens, monkeypatch):
  """wg_forward with frames: every utterance of a padded batch gets, bit for bit, the z and log_s of the dense forward on its own
  crop, and exact zeros behind its columns; mel and audio behind an utterance hold NaN."""
  if force_bn:
    monkeypatch.setenv("WG_FORCE_BN", force_bn)
  hp = HParams(n_channels=channels, n_layers=8, n_flows=4, n_early_every=2)
  model = build_model(hp, synthetic.make_state_dict(hp, seed=6))
  mel, audio, singles = _ragged_batch(lens, dtype)
  z, log_s = model.forward_ragged(mel, audio, lens)
  assert z.dtype == dtype and z.shape == (len(lens), 8, 32 * max(lens)) and len(log_s) == hp.n_flows
  for b, T in enumerate(lens):
    with torch.no_grad():
      z1, ls1, _ = model(singles[b])
    assert torch.isfinite(z1).all()
    assert torch.equal(z[b, :, :32 * T], z1[0]), b
    assert not z[b, :, 32 * T:].any(), b
    for k in range(hp.n_flows):
      assert torch.equal(log_s[k][b, :, :32 * T], ls1[k][0]), (b, k)
      assert not log_s[k][b, :, 32 * T:].any(), (b, k)
  # counts on the device are trusted: the same bits; one outside [1, T] gives that utterance zeros and harms no other
  fr = torch.tensor(lens, dtype=torch.int32, device=DEV)
  z2, log_s2 = model.forward_ragged(mel, audio, fr)
  assert torch.equal(z2, z) and all(torch.equal(a, b) for a, b in zip(log_s2, log_s))
  bad = fr.clone()
  bad[0], bad[1] = max(lens) + 1, 0
  z3, log_s3 = model.forward_ragged(mel, audio, bad)
  assert not z3[:2].any() and not any(t[:2].any() for t in log_s3)
  assert torch.equal(z3[2:], z[2:]) and all(torch.equal(a[2:], b[2:]) for a, b in zip(log_s3, log_s))


def test_full_counts_give_the_bits_of_the_dense_batch():
  hp = HParams(n_channels=64, n_layers=8, n_flows=4, n_early_every=2)
  model = build_model(hp, synthetic.make_state_dict(hp, seed=6), normed=True)
  B, T = 3, 11
  mel = synthetic.make_mel(B, T, seed=3).to(DEV)
  audio = torch.cat([_audio(256 * T, 50 + b) for b in range(B)]).to(DEV)
  with torch.no_grad():
    z, log_s, _ = model((mel, audio))
  z2, log_s2 = model.forward_ragged(mel, audio, [T] * B)
  assert torch.equal(z2, z) and all(torch.equal(a, b) for a, b in zip(log_s2, log_s))
  dense, track = model.log_likelihood_enqueue(mel, audio, per_frame=True)
  full, track2 = model.log_likelihood_enqueue(mel, audio, frames=[T] * B, per_frame=True)
  assert dense.dtype == torch.float64 and dense.shape == (B, 8) and track.shape == (B, T)
  assert torch.equal(dense, full) and torch.equal(track, track2) and torch.isfinite(track).all()


# ------------------------------------------------------------------------------------------- wg_nll
def _check_rows(rows, track, z, log_s, logdets, frames, sigma, what):
  want, want_track, yard = oracle.likelihood_rows(z.cpu().numpy(), [t.cpu().numpy() for t in log_s], logdets, frames, sigma)
  rows, track = rows.cpu().numpy(), track.cpu().numpy()
  assert rows[:, 5].tolist() == want[:, 5].tolist()                       # the counts are exact
  n = want[:, 5]
  # per-sample figures against the yardstick; the sums against the yardstick times the samples they run over; the moments
  # of z against 1 + mean z^2 (mean |z| <= max(1, mean z^2), and mean z^2 <= 2 sigma^2 * yardstick)
  zz = 1.0 + 2 * sigma * sigma * yard
  scale = np.stack([yard, yard / np.log(2), yard * n, yard * n, yard * n, np.ones_like(n), zz, zz], axis=1)
  err = np.abs(rows - want) / scale
  err[:, 5] = 0
  print(f"{what}: worst |device - oracle| / yardstick {err.max():.3e} (bar {ORDER_TOL:.0e}); nll {rows[:, 0].tolist()}")
  assert err.max() <= ORDER_TOL
  assert (np.isnan(track) == np.isnan(want_track)).all()
  live = ~np.isnan(want_track)
  assert np.abs(track[live] - want_track[live]).max() <= ORDER_TOL * max(1.0, float(np.abs(want_track[live]).max()))


@pytest.mark.parametrize("sigma", [1.0, 0.7])
def test_nll_against_the_oracle_dense_and_ragged(sigma):
  """wg_nll on the device's own z and log_s.  Dense at L = 163 (scalar loads, a partial last frame) and L = 180 (16-byte
  loads, a partial last frame); ragged at the pitch of 64 frames.  Bit-identical between two calls, and between an utterance
  in the batch and its own call at another pitch."""
  hp = HParams(n_channels=64, n_layers=8, n_flows=4, n_early_every=2)
  model = build_model(hp, synthetic.make_state_dict(hp, seed=6))
  logdets = _logdets(model)
  for S in (8 * 163 + 5, 8 * 180):
    B, T = 2, 6
    mel = synthetic.make_mel(B, T, seed=S).to(DEV)
    audio = torch.cat([_audio(S, S + b) for b in range(B)]).to(DEV)
    eng, z, log_s, fr = likelihood._forward(model, mel, audio, None)
    assert fr is None and z.shape[2] == S // 8
    rows, track = likelihood.nll_enqueue(eng, z, log_s, None, sigma, per_frame=True)
    _check_rows(rows, track, z, log_s, logdets, None, sigma, f"dense L={S // 8} sigma={sigma}")
    again, track2 = likelihood.nll_enqueue(eng, z, log_s, None, sigma, per_frame=True)
    assert torch.equal(rows, again) and torch.equal(track.nan_to_num(7.0), track2.nan_to_num(7.0))
  lens = [37, 5, 64, 21]
  mel, audio, _ = _ragged_batch(lens)
  eng, z, log_s, fr = likelihood._forward(model, mel, audio, lens)
  rows, track = likelihood.nll_enqueue(eng, z, log_s, fr, sigma, per_frame=True)
  _check_rows(rows, track, z, log_s, logdets, lens, sigma, f"ragged sigma={sigma}")
  again, track2 = likelihood.nll_enqueue(eng, z, log_s, fr, sigma, per_frame=True)
  assert torch.equal(rows, again) and torch.equal(track.nan_to_num(7.0), track2.nan_to_num(7.0))
  assert torch.equal(likelihood.nll_enqueue(eng, z, log_s, fr, sigma)[0], rows)          # without the track
  for b, T in enumerate(lens):
    zb = z[b:b + 1, :, :32 * T].contiguous()
    lsb = [t[b:b + 1, :, :32 * T].contiguous() for t in log_s]
    own, own_track = likelihood.nll_enqueue(eng, zb, lsb, None, sigma, per_frame=True)
    assert torch.equal(own[0], rows[b]) and torch.equal(own_track[0], track[b, :T]), b
    own, _ = likelihood.nll_enqueue(eng, zb, lsb, torch.tensor([T], dtype=torch.int32, device=DEV), sigma)
    assert torch.equal(own[0], rows[b]), b
  # counts outside [1, L / 32]: nothing is scored, nothing else moves
  bad = torch.tensor([65, 0, 64, 21], dtype=torch.int32, device=DEV)
  r2, t2 = likelihood.nll_enqueue(eng, z, log_s, bad, sigma, per_frame=True)
  assert r2[:2, 5].tolist() == [0.0, 0.0] and torch.isnan(r2[:2, 0]).all() and torch.isnan(t2[:2]).all()
  assert torch.equal(r2[2:], rows[2:])


@pytest.mark.parametrize("sigma", [1.0, 0.7])
def test_dense_batch_mean_is_the_training_loss(sigma):
  hp = HParams(n_channels=64, n_layers=8, n_flows=4, n_early_every=2)
  model = build_model(hp, synthetic.make_state_dict(hp, seed=6), normed=True)
  B, T, S = 3, 9, 256 * 9 - 13
  mel = synthetic.make_mel(B, T, seed=12).to(DEV)
  audio = torch.cat([_audio(S, 60 + b) for b in range(B)]).to(DEV)
  with torch.no_grad():
    loss = float(WaveGlowLoss(sigma)(model((mel, audio))))
  res = model.log_likelihood(mel, audio, sigma=sigma)
  assert len(res) == B and all(r.samples == S - S % 8 for r in res)
  mean = sum(r.samples * r.nll for r in res) / sum(r.samples for r in res)
  print(f"sigma={sigma}: batch-weighted mean {mean:.9f}, WaveGlowLoss {loss:.9f}")
  assert abs(mean - loss) <= 2e-6 * max(1.0, abs(loss))
  for r in res:
    assert abs(r.bits_per_sample - (r.nll + 0.5 * np.log(2 * np.pi * sigma * sigma)) / np.log(2)) <= 1e-12
    assert abs(r.nll - (r.sum_z2 / (2 * sigma * sigma) - r.sum_log_s - r.log_det) / r.samples) <= 1e-12


@pytest.mark.parametrize("name", ["c64", "c256", "c512"])
def test_dense_likelihood_against_the_reference(name):
  """The device's dense log_likelihood on the golden inputs against the oracle on the reference's own fwd_* arrays."""
  c = Case(name)
  model = build_model(c.hp, c.sd)
  wav = torch.from_numpy(c.npz["fwd_audio_in"])
  z_ref = c.npz["fwd_z"]
  B, _, L = z_ref.shape
  want, _, _ = oracle.likelihood_rows(z_ref, [c.npz[f"fwd_log_s_{k}"] for k in range(c.hp.n_flows)],
                                      c.npz["fwd_log_det"].astype(np.float64) / (B * L), None, 1.0)
  res = model.log_likelihood(c.mel.to(DEV), wav.to(DEV))
  assert [r.samples for r in res] == want[:, 5].tolist()
  mean = sum(r.samples * r.nll for r in res) / sum(r.samples for r in res)
  worst = max(abs(r.nll - w) for r, w in zip(res, want[:, 0]))
  print(f"{name}: batch mean {mean:.7f} (reference loss {float(c.npz['fwd_loss']):.7f}), "
        f"worst per-utterance |nll - reference| {worst:.3e}")
  assert abs(mean - float(c.npz["fwd_loss"])) <= 2e-3
  assert worst <= UTTERANCE_NLL_TOL


# ------------------------------------------------------------------------------------------- end to end
def test_cli_validate_likelihood_batch_equals_one_by_one(tmp_path, monkeypatch):
  """The four columns are there; a batch of three gives every utterance the figures of one-by-one validation bit for bit;
  they are the likelihood of the file's whole frames under its own mel.  Without the flag the table has the columns of
  before and nothing of the likelihood is launched.  (Byte equality of a whole total.csv between two runs cannot be asked:
  the table carries the time of day and measured durations.)"""
  import pandas
  from waveglow_amd import cli
  from waveglow_amd.audio import float_to_wav
  from waveglow_amd.checkpoint import CheckpointWaveglow
  from waveglow_amd.taco_stft import TacotronSTFT
  hp = HParams(n_channels=16, n_layers=3, n_flows=4, n_early_every=2, sigma=0.9)
  m = WaveGlow(hp)
  m.load_state_dict(synthetic.to_weightnorm_form(synthetic.make_state_dict(hp, seed=8)))
  folder = tmp_path / "ckpt"
  folder.mkdir()
  CheckpointWaveglow.from_instances(m, None, hp, 3).save(folder / "3.pt")
  src = tmp_path / "wavs"
  src.mkdir()
  sizes = (9000, 14001, 5120)
  rng = np.random.default_rng(3)
  for i, n in enumerate(sizes):
    t = np.arange(n) / hp.sampling_rate
    wav = 0.3 * np.sin(2 * np.pi * (150 + 40 * i) * t) + 0.02 * rng.standard_normal(n)
    float_to_wav(wav.astype(np.float32), src / f"u{i}.wav", sample_rate=hp.sampling_rate)
  tables = []
  for bs in ("3", "1"):
    out = tmp_path / f"val{bs}"
    assert cli.main(["validate", str(folder), str(out), str(src), "--full-run", "--custom-seed", "7", "--batch-size", bs,
                     "--likelihood"]) == 0
    tables.append(pandas.read_csv(out / "total.csv", sep="\t", float_precision="round_trip"))
    assert "Bits per sample: " in (out / "log.txt").read_text()
  today = _pitch_cases.TODAY
  assert list(tables[0].columns) == today[:-1] + LIKELIHOOD + today[-1:]
  for col in LIKELIHOOD + ["MCD", "Cosine Similarity (Padded)"]:
    x, y = tables[0][col].to_numpy(), tables[1][col].to_numpy()
    print(col, x.tolist())
    assert x.tobytes() == y.tobytes(), col
  assert tables[0]["# Likelihood frames"].tolist() == [n // 256 for n in sizes]
  # the figures of the files themselves
  model = m.to(DEV).eval()
  taco = TacotronSTFT(hp, torch.device(DEV))
  for i, n in enumerate(sizes):
    mel, frames, wav, lens = taco.get_mel_and_wav_tensors_from_files([src / f"u{i}.wav"])
    r = model.log_likelihood(mel, wav, frames=[n // 256], sigma=hp.sigma)[0]
    row = tables[0].iloc[i]
    assert (row["NLL (nats/sample)"], row["Bits per sample"], row["z variance"]) == (r.nll, r.bits_per_sample, r.z_var)
    assert np.isfinite([r.nll, r.bits_per_sample, r.z_var]).all() and r.samples == 256 * (n // 256)
  # without the flag: the table and the log of before, and no likelihood call at all
  def refuse(*a, **k):
    raise AssertionError("the likelihood was launched without --likelihood")
  monkeypatch.setattr(likelihood, "log_likelihood_enqueue", refuse)
  out = tmp_path / "plain"
  assert cli.main(["validate", str(folder), str(out), str(src), "--full-run", "--custom-seed", "7", "--batch-size", "3"]) == 0
  assert (out / "total.csv").read_text().splitlines()[0] == "\t".join(today)
  assert "NLL" not in (out / "log.txt").read_text() and "Bits per sample" not in (out / "log.txt").read_text()
  plain = pandas.read_csv(out / "total.csv", sep="\t", float_precision="round_trip")
  for col in ("MCD", "MFCC DTW MCD", "Cosine Similarity (Padded)", "# Frames"):
    assert plain[col].to_numpy().tobytes() == tables[0][col].to_numpy().tobytes(), col
