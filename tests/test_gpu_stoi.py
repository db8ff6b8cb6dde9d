"""The intelligibility metrics on the device (``wg_stoi``, waveglow_amd/metrics.py) and ``waveglow-cli validate
--intelligibility-metrics`` end to end.  The reference of every value is tests/_stoi_oracle.py, computed once per case and
shared (tests/_stoi_cases.py).  The three counts are compared exactly, which the oracle's margin to the energy gate
(> 1e-6 dB, asserted first) makes a fair demand; STOI and ESTOI to 1e-10 absolute, at least 100 times the oracle's own
rounding against a longdouble restatement (tests/test_stoi_cpu.py: at most 1e-12) and five orders below any difference the
metric is read for.  Every row of a ragged batch must come out bit for bit as its own call gives it."""
import numpy as np
import pytest
import torch

import _pitch_cases
import _stoi_cases as cases
import _stoi_oracle as oracle
from waveglow_amd import _lib, metrics, resample, synthetic
from waveglow_amd.hparams import HParams
from waveglow_amd.model import WaveGlow

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
BAR = 1e-10
MARGIN = 1e-6


def _batch(signals, fill=np.nan):
  """fp32 [B, max(len)] on the device (at least one column), row b holding signals[b] and `fill` behind it."""
  out = np.full((len(signals), max(1, max(len(s) for s in signals))), fill, np.float32)
  for b, s in enumerate(signals):
    out[b, :len(s)] = s
  return torch.from_numpy(out).to(DEV)


def _rows(xs, ys):
  return metrics.stoi_enqueue(_batch(xs), [len(x) for x in xs], _batch(ys), [len(y) for y in ys]).cpu().numpy()


def _check(label, row, ref):
  """one row of the device against the oracle's result; returns the largest distance of the two values"""
  print(f"{label}: device {row[:5].tolist()} oracle {ref}")
  assert ref["margin"] > MARGIN, f"{label}: the oracle's own mask is not stable enough to pin"
  assert (row[metrics.STOI_FRAMES], row[metrics.STOI_FRAMES_KEPT], row[metrics.STOI_SEGMENTS]) == \
      (ref["frames"], ref["frames_kept"], ref["segments"]), label
  assert not row[5:].any()
  worst = 0.0
  for key, col in (("stoi", metrics.STOI), ("estoi", metrics.ESTOI)):
    if np.isnan(ref[key]):
      assert np.isnan(row[col]), (label, key)
    else:
      dist = abs(row[col] - ref[key])
      print(f"{label}: {key} {row[col]!r} oracle {ref[key]!r} distance {dist:.3e}")
      assert dist <= BAR, (label, key, dist)
      worst = max(worst, dist)
  return worst


@pytest.mark.parametrize("n", cases.LENGTHS)
def test_shared_cases_equal_oracle(n):
  pairs = [cases.pair(n, snr) for snr in cases.SNRS]
  rows = _rows([p[0] for p in pairs], [p[1] for p in pairs])
  worst = max(_check(f"{n} samples, snr {snr}", rows[i], cases.reference(n, snr)) for i, snr in enumerate(cases.SNRS))
  print(f"{n}: largest distance to the oracle {worst:.3e}")
  m = metrics.stoi(_batch([pairs[1][0]]), None, _batch([pairs[1][1]]), None)[0]
  ref = cases.reference(n, cases.SNRS[1])
  assert (m.frames, m.frames_kept, m.segments) == (ref["frames"], ref["frames_kept"], ref["segments"])
  assert m.stoi == rows[1, metrics.STOI] and m.estoi == rows[1, metrics.ESTOI]


def test_frame_count_corners():
  """Stationary noise keeps every frame, so F0 sets K = F0, F = F0 - 1 and J = F0 - 30: the first segment (30 .. 33), the
  frame tile T of the band kernel (T - 1, T, T + 1, 2 T + 1 frames; F = K - 1 crosses the tile one frame later, which the
  same list covers) and the segment tile S (J = S - 1, S, S + 1, 2 S + 1).  Then the shortest signals and a click in
  silence with one and two kept frames."""
  T, S = metrics.STOI_FRAME_TILE, metrics.STOI_SEGMENT_TILE
  counts = sorted({30, 31, 32, 33, T - 1, T, T + 1, T + 2, 2 * T + 1, 2 * T + 2, 29 + S, 30 + S, 31 + S, 31 + 2 * S})
  xs = [cases.stationary(f) for f in counts]
  ys = [cases.add_noise(x, 5.0) for x in xs]
  base = cases.stationary(4)
  for n in (0, 256, 257, 385):
    xs.append(base[:n]), ys.append(cases.add_noise(base, 5.0)[:n])
  for kept in (1, 2):
    xs.append(cases.click(kept)), ys.append(cases.add_noise(cases.click(kept), 20.0))
  rows = _rows(xs, ys)
  worst = 0.0
  for i, (x, y) in enumerate(zip(xs, ys)):
    ref = oracle.stoi(x, y)
    if i < len(counts):
      assert (ref["frames"], ref["frames_kept"], ref["segments"]) == (counts[i], counts[i], max(counts[i] - 30, 0))
    worst = max(worst, _check(f"{len(x)} samples", rows[i], ref))
  tail = rows[len(counts):, 2:5].tolist()
  assert tail == [[0, 0, 0], [0, 0, 0], [1, 1, 0], [2, 2, 0], [155, 1, 0], [155, 2, 0]]
  print(f"corners: largest distance to the oracle {worst:.3e}")


def test_silence_gives_exactly_zero():
  z = np.zeros(20000, np.float32)
  row = _rows([z], [z])[0]
  assert row.tolist() == [0.0, 0.0, 155.0, 155.0, 125.0, 0.0, 0.0, 0.0]
  row = _rows([z], [cases.clean(cases.LENGTHS[0])])[0]                         # a silent clean side: every band of x is 0
  assert row[:2].tolist() == [0.0, 0.0] and row[2:5].tolist() == [155.0, 155.0, 125.0]


def test_ragged_batch_rows_are_their_own_calls():
  """B = 5 on the longest pitch with NaN behind every length: three speech-like rows, one of length 0, one of 257 samples.
  Every row has the bits of its own B = 1 call on its own pitch, and two identical calls give identical bits."""
  pairs = [cases.pair(n, 20.0) for n in cases.LENGTHS]
  xs = [pairs[0][0], np.zeros(0, np.float32), pairs[1][0], pairs[2][0][:257], pairs[2][0]]
  ys = [pairs[0][1], np.zeros(0, np.float32), pairs[1][1], pairs[2][1][:257], pairs[2][1]]
  xb, yb = _batch(xs), _batch(ys)
  assert xb.shape == (5, 30353) and torch.isnan(xb[4, 10000:]).all() and torch.isnan(yb[1]).all()
  lens = [len(x) for x in xs]
  rows = metrics.stoi_enqueue(xb, lens, yb, lens).cpu().numpy()
  again = metrics.stoi_enqueue(xb, lens, yb, lens).cpu().numpy()
  assert rows.tobytes() == again.tobytes()
  assert np.isfinite(rows[[0, 2, 4]]).all() and rows[[0, 2, 4], 4].tolist() == [56.0, 84.0, 16.0]
  assert np.isnan(rows[[1, 3], :2]).all() and rows[1, 2:].tolist() == [0] * 6 and rows[3, 2:5].tolist() == [1, 1, 0]
  for i in range(5):
    own = _rows([xs[i]], [ys[i]])
    assert own.tobytes() == rows[i:i + 1].tobytes(), i
  # the longer of two lengths is cropped to the shorter, on the device; lengths may live there
  ld = torch.tensor(lens, dtype=torch.int32, device=DEV)
  longer = torch.tensor([n + 7 if 0 < n < 30000 else n for n in lens], dtype=torch.int32, device=DEV)
  xz = torch.nan_to_num(xb, nan=0.25)
  assert metrics.stoi_enqueue(xz, longer, yb, ld).cpu().numpy().tobytes() == rows.tobytes()
  # a length outside [0, N] on the device counts as 0
  off = torch.tensor([30354, -1, 30353, 257, 10000], dtype=torch.int32, device=DEV)
  out = metrics.stoi_enqueue(xb, off, yb, ld).cpu().numpy()
  assert out[2:].tobytes() == rows[2:].tobytes() and np.isnan(out[:2, :2]).all() and not out[:2, 2:].any()


def test_intelligibility_metrics_at_22050_hz():
  """The 22 050 Hz entry is the resampler followed by wg_stoi: bit for bit ``stoi`` on the resampler's own output cropped to
  the common length, and within the bar of the oracle fed that output."""
  n_a, n_b = 44100, 43000
  a = cases.speech_22k()[:n_a]
  b = cases.add_noise(cases.speech_22k()[:n_a], 10.0)[:n_b]
  xa, xb = _batch([a, a[:30000]]), _batch([b, b[:30000]])
  la, lb = [n_a, 30000], [n_b, 29000]
  rows = metrics.intelligibility_metrics_enqueue(xa, la, xb, lb, sampling_rate=22050).cpu().numpy()
  got = metrics.intelligibility_metrics(xa, la, xb, lb)
  from scipy.signal import resample_poly
  for i in range(2):
    n = min(la[i], lb[i])
    n10 = resample.out_len(n, 200, 441)
    ra, _ = resample.resample(xa[i:i + 1, :n].contiguous(), None, 22050, 10000)
    rb, _ = resample.resample(xb[i:i + 1, :n].contiguous(), None, 22050, 10000)
    assert ra.shape == (1, n10)
    own = metrics.stoi_enqueue(ra, None, rb, None).cpu().numpy()
    assert own.tobytes() == rows[i:i + 1].tobytes(), i
    ha, hb = ra[0].cpu().numpy(), rb[0].cpu().numpy()
    _check(f"pair {i} on the device resampler's output", rows[i], oracle.stoi(ha, hb))
    assert (got[i].stoi, got[i].estoi, got[i].frames) == (rows[i, 0], rows[i, 1], oracle.frame_count(n10))
    ref = oracle.stoi(resample_poly(xa[i, :n].cpu().numpy().astype(np.float64), 200, 441).astype(np.float32),
                      resample_poly(xb[i, :n].cpu().numpy().astype(np.float64), 200, 441).astype(np.float32))
    print(f"pair {i}: distance to the oracle fed scipy's resampling (not asserted): stoi "
          f"{abs(rows[i, 0] - ref['stoi']):.3e} estoi {abs(rows[i, 1] - ref['estoi']):.3e}, counts "
          f"{rows[i, 2:5].tolist()} against {[ref['frames'], ref['frames_kept'], ref['segments']]}")
  # 10 000 Hz skips the resampler
  x, y = cases.pair(cases.LENGTHS[2], 20.0)
  direct = metrics.intelligibility_metrics_enqueue(_batch([x]), None, _batch([y]), None, sampling_rate=10000)
  assert direct.cpu().numpy().tobytes() == _rows([x], [y]).tobytes()


def test_refusals_leave_the_device_usable():
  x, y = cases.pair(cases.LENGTHS[2], 20.0)
  xd, yd = _batch([x]), _batch([y])
  ref = cases.reference(cases.LENGTHS[2], 20.0)

  def good():
    m = metrics.stoi(xd, None, yd, None)[0]
    assert (m.frames, m.frames_kept, m.segments) == (ref["frames"], ref["frames_kept"], ref["segments"])
    assert abs(m.stoi - ref["stoi"]) <= BAR

  bad_calls = [
    lambda: metrics.stoi(xd.cpu(), None, yd, None),                                        # a CPU tensor
    lambda: metrics.stoi(xd, None, yd.cpu(), None),
    lambda: metrics.stoi(xd.half(), None, yd, None),                                       # fp16
    lambda: metrics.stoi(xd, None, yd.double(), None),
    lambda: metrics.stoi(xd[0], None, yd, None),                                           # rank
    lambda: metrics.stoi(xd, [10001], yd, None),                                           # a length behind the row
    lambda: metrics.stoi(xd, None, yd, [-1]),
    lambda: metrics.stoi(xd, [10000, 10000], yd, None),                                    # two lengths for one row
    lambda: metrics.stoi(xd, None, torch.cat([yd, yd]), None),                             # mismatched B
    lambda: metrics.stoi(xd, torch.tensor([10000], device=DEV), yd, None),                 # int64 lengths on the device
    lambda: metrics.intelligibility_metrics(xd, None, yd, None, sampling_rate=10001),      # 10000 / 10001
    lambda: metrics.intelligibility_metrics(xd, [10001], yd, None),
    lambda: metrics.intelligibility_metrics(xd.cpu(), None, yd, None),
  ]
  for call in bad_calls:
    with pytest.raises(_lib.WgError):
      call()
    good()


# -------------------------------------------------------------------------------------------------------- end to end
@pytest.fixture(scope="module")
def ckpt(tmp_path_factory):
  """(checkpoint folder, hparams): the 16-channel model of the golden case "tiny" with synthetic weights, saved as 3.pt."""
  from waveglow_amd.checkpoint import CheckpointWaveglow
  hp = HParams(n_channels=16, n_layers=3, n_flows=4, n_early_every=2)
  m = WaveGlow(hp)
  m.load_state_dict(synthetic.to_weightnorm_form(synthetic.make_state_dict(hp, seed=8)))
  folder = tmp_path_factory.mktemp("validate_stoi_ckpt")
  CheckpointWaveglow.from_instances(m, None, hp, 3).save(folder / "3.pt")
  return folder, hp


def test_cli_validate_intelligibility_metrics_batch_equals_one_by_one(ckpt, tmp_path):
  """The four columns are there, a batch of three gives every utterance the figures of one-by-one validation bit for bit,
  and they are the metric of the files: the clean side is the wav as loaded, the processed side the written
  inferred_denoised.wav.  That file is the int16 rounding of the peak-normalised synthesis the columns were computed on: a
  rounding error 98 dB below full scale, 58 dB below a frame at the energy gate, so the values agree to well within 1e-3
  (the counts, which the clean side alone decides, exactly)."""
  import pandas
  from waveglow_amd import cli
  from waveglow_amd.audio import float_to_wav, wav_to_float32
  folder, hp = ckpt
  src = tmp_path / "wavs"
  src.mkdir()
  sizes = (22050, 30001, 26000)
  speech = cases.speech_22k()
  for i, n in enumerate(sizes):
    float_to_wav(speech[3000 * i:3000 * i + n].copy(), src / f"u{i}.wav", sample_rate=hp.sampling_rate)
  tables = []
  for bs in ("3", "1"):
    out = tmp_path / f"val{bs}"
    assert cli.main(["validate", str(folder), str(out), str(src), "--full-run", "--custom-seed", "7", "--batch-size", bs,
                     "--intelligibility-metrics"]) == 0
    tables.append(pandas.read_csv(out / "total.csv", sep="\t", float_precision="round_trip"))
    assert "ESTOI: " in (out / "log.txt").read_text()
  today = _pitch_cases.TODAY
  assert list(tables[0].columns) == today[:-1] + cases.STOI_COLUMNS + today[-1:]
  for col in cases.STOI_COLUMNS + ["MCD", "MFCC DTW MCD", "Cosine Similarity (Padded)"]:
    x, y = tables[0][col].to_numpy(), tables[1][col].to_numpy()
    print(col, x.tolist())
    assert x.tobytes() == y.tobytes(), col
  for i, n in enumerate(sizes):
    wav, _ = wav_to_float32(src / f"u{i}.wav")
    syn, sr = wav_to_float32(tmp_path / "val3" / f"it=3_name=u{i}.wav" / "inferred_denoised.wav")
    assert sr == hp.sampling_rate and len(syn) == 256 * (n // 256 + 1)
    m = metrics.intelligibility_metrics(_batch([np.ascontiguousarray(wav, np.float32)]), None,
                                        _batch([np.ascontiguousarray(syn, np.float32)]), None, sampling_rate=sr)[0]
    row = tables[0].iloc[i]
    print(f"u{i}: table {[row[c] for c in cases.STOI_COLUMNS]} files {m}")
    assert row["# STOI frames"] == m.frames == metrics.stoi_frames(resample.out_len(n, 200, 441))
    assert row["# STOI frames kept"] == m.frames_kept > 30
    assert abs(row["STOI"] - m.stoi) <= 1e-3 and abs(row["ESTOI"] - m.estoi) <= 1e-3
    assert -1 <= row["ESTOI"] <= 1 and -1 <= row["STOI"] <= 1
  # both flags: the pitch columns first
  out = tmp_path / "both"
  assert cli.main(["validate", str(folder), str(out), str(src), "--full-run", "--custom-seed", "7", "--batch-size", "3",
                   "--pitch-metrics", "--intelligibility-metrics"]) == 0
  both = pandas.read_csv(out / "total.csv", sep="\t", float_precision="round_trip")
  assert list(both.columns) == today[:-1] + _pitch_cases.PITCH + cases.STOI_COLUMNS + today[-1:]
  for col in cases.STOI_COLUMNS:
    assert both[col].to_numpy().tobytes() == tables[0][col].to_numpy().tobytes(), col
  # without the flag: the table and the log of before
  out = tmp_path / "plain"
  assert cli.main(["validate", str(folder), str(out), str(src), "--full-run", "--custom-seed", "7", "--batch-size", "3"]) == 0
  assert (out / "total.csv").read_text().splitlines()[0] == "\t".join(today)
  assert "STOI" not in (out / "log.txt").read_text()
  plain = pandas.read_csv(out / "total.csv", sep="\t", float_precision="round_trip")
  for col in ("MCD", "MFCC DTW MCD", "Cosine Similarity (Padded)", "# Frames"):
    assert plain[col].to_numpy().tobytes() == tables[0][col].to_numpy().tobytes(), col
