"""The validation metrics on the device (``wg_metrics_*``, waveglow_amd/metrics.py), the device entry of the mel front-end
and ``waveglow-cli validate`` end to end.  The reference of every value is tests/_metrics_oracle.py, computed once per
input and shared; path lengths, frame counts and penalties are compared exactly, and every utterance of a ragged batch
must come out bit for bit as its own call gives it."""
import functools

import numpy as np
import pytest
import torch

import _metrics_oracle as oracle
from waveglow_amd import _lib, metrics, synthetic
from waveglow_amd.hparams import HParams
from waveglow_amd.model import WaveGlow

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
PAIRS = ((1, 1), (1, 7), (7, 1), (33, 70), (65, 64), (130, 97))
MARGIN = 1e-9          # the oracle's decision margin must exceed this for its path length to be THE path length


def _mel(rng, n_mel, T):
  return rng.uniform(-11.5, 2.0, (n_mel, T)).astype(np.float32)


def _pad(arrays):
  """list of [C, T_b] -> (fp32 [B, C, Tmax] on the device, frame counts)."""
  T = [a.shape[1] for a in arrays]
  out = np.zeros((len(arrays), arrays[0].shape[0], max(T)), np.float32)
  for b, a in enumerate(arrays):
    out[b, :, :T[b]] = a
  return torch.from_numpy(out).to(DEV), T


@functools.lru_cache(maxsize=None)
def small_mels():
  """The six pairs of 80-channel mels, channel 5 of pair 3's second mel all zero, and the oracle's values for them."""
  rng = np.random.default_rng(11)
  a = [_mel(rng, 80, ta) for ta, _ in PAIRS]
  b = [_mel(rng, 80, tb) for _, tb in PAIRS]
  b[3][5] = 0.0
  return a, b, [oracle.mel_metrics(x, y) for x, y in zip(a, b)]


@functools.lru_cache(maxsize=None)
def feature_case(seed, K, ta, tb):
  """(a [K, ta], b [K, tb], oracle (cost, frames, margin)).  K = 16: MFCCs of uniform log-mels, rounded to fp32;
  K = 80: such mels themselves."""
  rng = np.random.default_rng(seed)
  ma, mb = _mel(rng, 80, ta), _mel(rng, 80, tb)
  if K == 16:
    ma, mb = oracle.mfcc(ma).astype(np.float32), oracle.mfcc(mb).astype(np.float32)
  return ma, mb, oracle.dtw(ma, mb)


def _check_dtw(cases):
  a, ta = _pad([c[0] for c in cases])
  b, tb = _pad([c[1] for c in cases])
  cost, frames = metrics.dtw_distance(a, ta, b, tb)
  cost, frames = cost.cpu().numpy(), frames.cpu().numpy()
  for i, (_, _, (ref_cost, ref_frames, margin)) in enumerate(cases):
    print(f"pair {i} ({ta[i]}, {tb[i]}): cost {cost[i]!r} oracle {ref_cost!r} rel {abs(cost[i] - ref_cost) / ref_cost:.3e} "
          f"frames {frames[i]} oracle {ref_frames} margin {margin:.3e}")
    assert margin > MARGIN, f"pair {i}: the oracle's own decisions are not stable enough to pin a path length"
    assert frames[i] == ref_frames
    assert abs(cost[i] - ref_cost) <= 1e-10 * ref_cost


@pytest.mark.parametrize("n_mel,n_mfcc", [(80, 16), (16, 15)])
def test_mfcc_equals_oracle(n_mel, n_mfcc):
  rng = np.random.default_rng(3)
  mels = [_mel(rng, n_mel, t) for t in (1, 7, 64, 65, 130)]
  mel, T = _pad(mels)
  mel[0, :, 1:] = 7.0                                        # behind an utterance: must not reach its coefficients
  out = metrics.mfcc(mel, T, n_mfcc).cpu().numpy()
  assert out.shape == (5, n_mfcc, 130) and out.dtype == np.float32
  for b, m in enumerate(mels):
    ref = oracle.mfcc(m, n_mfcc)
    err = np.abs(out[b, :, :T[b]].astype(np.float64) - ref.astype(np.float32).astype(np.float64))
    print(f"utterance {b}: largest |delta| / (2^-22 |X| + 1e-12) = {np.max(err / (2.0 ** -22 * np.abs(ref) + 1e-12)):.3f}")
    assert np.all(err <= 2.0 ** -22 * np.abs(ref) + 1e-12)
    assert not out[b, :, T[b]:].any()
  full = metrics.mfcc(mel[4:5], None, n_mfcc).cpu().numpy()  # no frame counts: every column counts
  assert np.array_equal(full[0], out[4])


def test_dtw_ragged_batch_equals_oracle():
  _check_dtw([feature_case(100 + i, 16, ta, tb) for i, (ta, tb) in enumerate(PAIRS)])


def test_dtw_diagonal_longer_than_a_workgroup():
  _check_dtw([feature_case(203, 16, 1100, 1030)])


def test_dtw_at_the_frame_limit():
  _check_dtw([feature_case(300, 16, 4096, 3)])


def test_dtw_eighty_features():
  _check_dtw([feature_case(400, 80, 33, 70), feature_case(401, 80, 65, 64)])


@pytest.mark.parametrize("seed,cost,frames", [(1, 8.0, 17), (4, 6.0, 15)])
def test_dtw_tie_order_on_integer_features(seed, cost, frames):
  r = np.random.default_rng(seed)
  a, b = np.zeros((16, 9), np.float32), np.zeros((16, 12), np.float32)
  a[0] = r.integers(0, 3, 9)
  b[0] = r.integers(0, 3, 12)
  assert oracle.dtw(a, b)[:2] == (cost, frames)
  got_cost, got_frames = metrics.dtw_distance(torch.from_numpy(a[None]).to(DEV), None, torch.from_numpy(b[None]).to(DEV), None)
  assert float(got_cost[0]) == cost and int(got_frames[0]) == frames


def test_padded_mcd_and_cosine_equal_oracle():
  a, b, ref = small_mels()
  ma, ta = _pad(a)
  mb, tb = _pad(b)
  got = metrics.mel_metrics(ma, ta, mb, tb)
  assert any(x > y for x, y in zip(ta, tb)) and any(x < y for x, y in zip(ta, tb))
  for i, (g, r) in enumerate(zip(got, ref)):
    print(f"pair {i}: mcd {g.mcd!r} oracle {r['mcd']!r}; cosine {g.cosine!r} oracle {r['cosine']!r}; "
          f"mcd_dtw {g.mcd_dtw!r} oracle {r['mcd_dtw']!r}; frames_dtw {g.frames_dtw} oracle {r['frames_dtw']}")
    assert abs(g.mcd - r["mcd"]) <= 1e-12 * r["mcd"]
    assert abs(g.cosine - r["cosine"]) <= 1e-9
    assert g.frames == r["frames"] == max(ta[i], tb[i]) and g.penalty == r["penalty"]
  # a zero channel scores 1: pair 3 with every channel of one side zero has cosine similarity 0
  z = metrics.mel_metrics(ma[3:4], [ta[3]], torch.zeros_like(mb[3:4]), [tb[3]])[0]
  assert z.cosine == 0.0


def _rows(a, b, order):
  ma, ta = _pad([a[i] for i in order])
  mb, tb = _pad([b[i] for i in order])
  rows = metrics.mel_metrics_enqueue(ma, ta, mb, tb)
  return rows.cpu().numpy(), (ma, ta, mb, tb)


def test_ragged_batch_equals_single_calls_bit_for_bit():
  a, b, _ = small_mels()
  order = list(range(len(PAIRS)))
  rows, (ma, ta, mb, tb) = _rows(a, b, order)
  again, _ = _rows(a, b, order)
  assert not np.isnan(rows).any() and rows.tobytes() == again.tobytes()                 # the same bits twice
  back, _ = _rows(a, b, order[::-1])                                                    # the longest first
  assert back[::-1].tobytes() == rows.tobytes()
  for i in order:
    single, _ = _rows(a, b, [i])                                                        # B = 1, Tmax = T
    assert single[0].tobytes() == rows[i].tobytes(), f"pair {i} {PAIRS[i]}"
  # the fused call is the separate entries chained
  fa, fb = metrics.mfcc(ma, ta), metrics.mfcc(mb, tb)
  cost, frames = metrics.dtw_distance(fa, ta, fb, tb)
  cost, frames = cost.cpu().numpy(), frames.cpu().numpy().astype(np.float64)
  total = np.array(ta, np.float64) + np.array(tb, np.float64)
  assert np.array_equal(rows[:, metrics.MCD_DTW], cost / frames)
  assert np.array_equal(rows[:, metrics.FRAMES_DTW], frames)
  assert np.array_equal(rows[:, metrics.PENALTY_DTW], 2.0 - total / frames)
  # the large pair alone and beside a short one
  la, lb, (ref_cost, ref_frames, _) = feature_case(203, 16, 1100, 1030)
  sa, sb, _ = feature_case(100, 16, 1, 1)
  c1, f1 = metrics.dtw_distance(*_pad([la]), *_pad([lb]))
  c2, f2 = metrics.dtw_distance(*_pad([sa, la]), *_pad([sb, lb]))
  assert c1.cpu().numpy().tobytes() == c2[1:].cpu().numpy().tobytes() and int(f1[0]) == int(f2[1]) == ref_frames


def test_refusals_leave_the_device_usable():
  a, b, ref = small_mels()
  ma, ta = _pad(a)
  mb, tb = _pad(b)

  def good():
    g = metrics.mel_metrics(ma, ta, mb, tb)[4]
    assert g.frames_dtw == ref[4]["frames_dtw"] and abs(g.mcd - ref[4]["mcd"]) <= 1e-12 * ref[4]["mcd"]

  bad_calls = [
    lambda: metrics.mel_metrics(ma.cpu(), ta, mb, tb),                                   # a CPU tensor
    lambda: metrics.mel_metrics(ma.half(), ta, mb, tb),                                  # fp16
    lambda: metrics.mel_metrics(ma, [4097] + ta[1:], mb, tb),                            # a frame count of 4097
    lambda: metrics.mel_metrics(ma, ta, mb[:5], tb[:5]),                                 # mismatched B
    lambda: metrics.mel_metrics(ma, ta[:5], mb, tb),
    lambda: metrics.dtw_distance(torch.zeros((1, 16, 4097), device=DEV), None, torch.zeros((1, 16, 3), device=DEV), None),
    lambda: metrics.mfcc(ma, ta, 80),
  ]
  for call in bad_calls:
    with pytest.raises(_lib.WgError):
      call()
    good()


# ------------------------------------------------------------------------------------------ mel front-end, device entry
@pytest.fixture(scope="module")
def ckpt(tmp_path_factory):
  """(checkpoint folder, hparams): the 64-channel synthetic model of test_gpu_ragged_post.py saved as 3.pt."""
  from waveglow_amd.checkpoint import CheckpointWaveglow
  hp = HParams(n_channels=64, n_layers=4, n_flows=4, n_early_every=2)
  m = WaveGlow(hp)
  m.load_state_dict(synthetic.to_weightnorm_form(synthetic.make_state_dict(hp, seed=8)))
  folder = tmp_path_factory.mktemp("validate_ckpt")
  CheckpointWaveglow.from_instances(m, None, hp, 3).save(folder / "3.pt")
  return folder, hp


def test_mel_ragged_device_equals_single(ckpt):
  from waveglow_amd.taco_stft import TacotronSTFT
  taco = TacotronSTFT(ckpt[1], torch.device(DEV))
  lens = [256 * t for t in (9, 40, 4, 31, 32)]
  N = max(lens)
  audio = (torch.rand((len(lens), N), generator=torch.Generator().manual_seed(5)) * 2 - 1).to(DEV)
  mel, frames, frames_dev = taco.mel_spectrogram_ragged_device(audio, lens)
  assert frames == [n // 256 + 1 for n in lens] and frames_dev.tolist() == frames and frames_dev.dtype == torch.int32
  assert mel.shape == (len(lens), taco.n_mel_channels, N // 256 + 1)
  for b, n in enumerate(lens):
    single = taco.mel_spectrogram(audio[b:b + 1, :n].cpu())[0]
    assert torch.equal(mel[b, :, :frames[b]], single), f"utterance {b} ({n} samples)"
    assert not mel[b, :, frames[b]:].any()
  for bad in (lambda: taco.mel_spectrogram_ragged_device(audio.cpu(), lens),
              lambda: taco.mel_spectrogram_ragged_device(audio, lens[:-1]),
              lambda: taco.mel_spectrogram_ragged_device(audio, [512] + lens[1:]),
              lambda: taco.mel_spectrogram_ragged_device(audio, [N + 256] + lens[1:])):
    with pytest.raises(_lib.WgError):
      bad()


# -------------------------------------------------------------------------------------------------------- end to end
METRIC_COLUMNS = ["# Difference frames", "# MFCC Coefficients", "MFCC DTW MCD", "MFCC DTW PEN", "# MFCC DTW frames", "MCD",
                  "PEN", "# Frames", "Cosine Similarity (Padded)", "Overamplified?", "Inferred wav duration (s)",
                  "Sampling rate (Hz)", "Seed", "Iteration", "Sigma", "Denoiser strength", "Name"]
FILES = ("original.mel.npy", "inferred_denoised.mel.npy", "original.wav", "inferred_denoised.wav", "inferred.wav")


def test_cli_validate_batch_equals_one_by_one(ckpt, tmp_path):
  import pandas
  from waveglow_amd import cli
  from waveglow_amd.audio import float_to_wav
  folder, hp = ckpt
  src = tmp_path / "wavs"
  src.mkdir()
  rng = np.random.default_rng(7)
  sizes = (3000, 5121, 4096)
  for i, n in enumerate(sizes):
    float_to_wav(rng.uniform(-0.5, 0.5, n).astype(np.float32), src / f"u{i}.wav", sample_rate=hp.sampling_rate)
  tables = []
  for bs in ("3", "1"):
    out = tmp_path / f"val{bs}"
    assert cli.main(["validate", str(folder), str(out), str(src), "--full-run", "--custom-seed", "7", "--batch-size", bs]) == 0
    assert (out / "log.txt").stat().st_size > 0
    tables.append(pandas.read_csv(out / "total.csv", sep="\t", float_precision="round_trip"))
  assert len(tables[0]) == 3 and list(tables[0]["Name"]) == [f"u{i}.wav" for i in range(3)]
  for col in METRIC_COLUMNS:
    assert list(tables[0][col]) == list(tables[1][col]), col
  assert list(tables[0]["# Difference frames"]) == [1, 1, 1]
  assert list(tables[0]["# Frames"]) == [n // 256 + 2 for n in sizes]
  wav_out = tmp_path / "resynth"
  assert cli.main(["synthesize-wav", str(folder / "3.pt"), str(src), "--custom-seed", "7", "-out", str(wav_out)]) == 0
  for i in range(3):
    d3, d1 = (tmp_path / f"val{bs}" / f"it=3_name=u{i}.wav" for bs in ("3", "1"))
    for name in FILES:
      assert (d3 / name).read_bytes() == (d1 / name).read_bytes(), f"u{i}: {name} differs between the batch sizes"
    assert (d3 / "inferred_denoised.wav").read_bytes() == (wav_out / f"u{i}.wav").read_bytes()
    orig, inf = np.load(d3 / "original.mel.npy"), np.load(d3 / "inferred_denoised.mel.npy")
    assert inf.shape[1] == orig.shape[1] + 1 == sizes[i] // 256 + 2
    m = metrics.mel_metrics(torch.from_numpy(orig[None]).to(DEV), None, torch.from_numpy(inf[None]).to(DEV), None)[0]
    row = tables[0].iloc[i]
    assert (row["MCD"], row["PEN"], row["# Frames"]) == (m.mcd, m.penalty, m.frames)
    assert (row["MFCC DTW MCD"], row["MFCC DTW PEN"], row["# MFCC DTW frames"]) == (m.mcd_dtw, m.penalty_dtw, m.frames_dtw)
    assert row["Cosine Similarity (Padded)"] == m.cosine
  assert cli.main(["validate", str(folder), str(tmp_path / "none"), str(src), "--files", "nobody.wav", "--custom-seed", "7"]) == 1
