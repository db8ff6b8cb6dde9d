"""The pitch metrics on the device (``wg_pitch_*``, waveglow_amd/metrics.py) and ``waveglow-cli validate --pitch-metrics``
end to end.  The reference of every value is tests/_pitch_oracle.py, computed once per parameter set and shared (tests/
_pitch_cases.py).  Frame counts, voicing decisions and the counts and shares of the pair row are compared exactly, f0 and
aperiodicity to 1e-9 and the two RMSEs to 1e-8 relative: a different summation order moves d' by at most W 2^-53 ~ 1e-13,
which at den > 1e-4 is at most 2e-9 in the parabola's shift, 6e-11 of a lag >= 36.  Every decision the comparison pins
must be stable in the oracle itself first (margin > 1e-7, den > 1e-4).  Every utterance of a ragged batch must come out
bit for bit as its own call gives it."""
import numpy as np
import pytest
import torch

import _pitch_cases as cases
import _pitch_oracle as oracle
from waveglow_amd import _lib, metrics, synthetic
from waveglow_amd.hparams import HParams
from waveglow_amd.model import WaveGlow

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
MARGIN, DEN = 1e-7, 1e-4
ROW_EXACT = (("gpe", metrics.GPE), ("vuv_error", metrics.VUV_ERROR), ("frames", metrics.PITCH_FRAMES),
             ("voiced_a", metrics.VOICED_A), ("voiced_b", metrics.VOICED_B), ("voiced_both", metrics.VOICED_BOTH))


def _batch(x, lens, fill=0.0):
  """fp32 [B, max(lens)] on the device, row b the first lens[b] samples of x and `fill` behind them."""
  out = np.full((len(lens), max(lens)), fill, np.float32)
  for b, n in enumerate(lens):
    out[b, :n] = x[:n]
  return torch.from_numpy(out).to(DEV)


def _host(tracks):
  return tuple(t.cpu().numpy() for t in tracks)


def _check_tracks(label, got, ref):
  """one utterance's device tracks (f0, aperiodicity, frame count) against the oracle's"""
  f0, ap, frames = got
  print(f"{label}: frames {frames} oracle {ref['frames']} margin {ref['margin']:.3e} den {ref['den']:.3e}")
  assert ref["margin"] > MARGIN and ref["den"] > DEN, f"{label}: the oracle's own decisions are not stable enough to pin"
  assert frames == ref["frames"]
  F = ref["frames"]
  assert not f0[F:].any() and not ap[F:].any()
  if F == 0:
    return
  assert np.array_equal(f0[:F] > 0, ref["f0"] > 0)
  v = ref["f0"] > 0
  rel_f0 = np.max(np.abs(f0[:F][v] / ref["f0"][v] - 1)) if v.any() else 0.0
  rel_ap = np.max(np.abs(ap[:F] / ref["aperiodicity"] - 1))
  print(f"{label}: voiced {int(v.sum())} of {F}; largest relative distance f0 {rel_f0:.3e} aperiodicity {rel_ap:.3e}")
  assert rel_f0 <= 1e-9 and rel_ap <= 1e-9


def _check_row(label, got, ref):
  print(f"{label}: row {got.tolist()} oracle {[ref[k] for k in oracle.ROW]} gpe margin {ref['gpe_margin']:.3e}")
  assert ref["gpe_margin"] > MARGIN
  for key, col in ROW_EXACT:
    assert got[col] == ref[key] or (np.isnan(got[col]) and np.isnan(ref[key])), key
  for key, col in (("f0_rmse_cents", metrics.F0_RMSE_CENTS), ("f0_rmse_hz", metrics.F0_RMSE_HZ)):
    if np.isnan(ref[key]):
      assert np.isnan(got[col]), key
    else:
      print(f"{label}: {key} {got[col]!r} oracle {ref[key]!r} rel {abs(got[col] / ref[key] - 1):.3e}")
      assert abs(got[col] - ref[key]) <= 1e-8 * ref[key]


def test_ragged_batch_with_defaults_equals_oracle():
  """0, 1, 2 and 19 frames: the utterance without a frame gives an all-zero track and a NaN row and disturbs nobody."""
  a, b = cases.signals()
  lens = list(cases.RAGGED)
  xa, xb = _batch(a, lens), _batch(b, lens)
  ta, tb = _host(metrics.yin_f0(xa, lens)), _host(metrics.yin_f0(xb, lens))
  assert ta[0].shape == (4, 19) and ta[0].dtype == np.float64 and ta[2].dtype == np.int32
  assert ta[2].tolist() == tb[2].tolist() == [0, 1, 2, 19]
  rows = metrics.pitch_metrics_enqueue(xa, lens, xb, lens).cpu().numpy()
  for i, n in enumerate(lens):
    _check_tracks(f"a[:{n}]", (ta[0][i], ta[1][i], int(ta[2][i])), cases.tracks("defaults", 0, n))
    _check_tracks(f"b[:{n}]", (tb[0][i], tb[1][i], int(tb[2][i])), cases.tracks("defaults", 1, n))
    _check_row(f"pair [:{n}]", rows[i], cases.row("defaults", n))
  assert np.isnan(rows[0, :4]).all() and not rows[0, 4:].any()
  full = cases.row("defaults")
  assert (full["frames"], full["voiced_both"], round(full["vuv_error"] * 19), round(full["gpe"] * 8)) == (19, 8, 4, 6)
  m = metrics.pitch_metrics(xa, lens, xb, lens)
  assert (m[3].frames, m[3].voiced_a, m[3].voiced_b, m[3].voiced_both) == (19, 12, 8, 8) and m[3].gross_pitch_error == 0.75
  assert m[3].vuv_error == 4 / 19 and m[0].frames == 0 and np.isnan(m[0].vuv_error)


@pytest.mark.parametrize("case", ["tau255", "tau256", "limits", "hop1"])
def test_corner_parameters_equal_oracle(case):
  """tau_max = 255 and 256 (the lag count crosses a pass of 256 threads), both upper limits (the largest LDS stage) and a
  hop of one sample, on side a."""
  params, n = cases.CASES[case]
  x = _batch(cases.signals()[0], [n])
  f0, ap, frames = _host(metrics.yin_f0(x, **params))
  ref = cases.tracks(case, 0)
  assert f0.shape == (1, ref["frames"])
  _check_tracks(case, (f0[0], ap[0], int(frames[0])), ref)


def test_sine_of_period_100_at_the_last_lag():
  """fmin = 220.5 makes lag 100 the last lag: no interpolation, f0 = 22050 / 100 on every frame, as in the oracle."""
  x = np.sin(2 * np.pi * np.arange(4000) / 100).astype(np.float32)
  f0, ap, frames = _host(metrics.yin_f0(_batch(x, [4000]), fmin=220.5))
  ref = oracle.yin(x, fmin=220.5)
  assert ref["margin"] > MARGIN and int(frames[0]) == ref["frames"] == 12
  assert np.all(f0[0] == 220.5) and np.all(ref["f0"] == 220.5) and np.all(ap[0] < 1e-6)


def test_pair_rows_of_hand_made_tracks():
  f0_a = np.zeros((4, 300))
  f0_b = np.zeros((4, 6))
  f0_a[0, :6] = [100.0, 0.0, 200.0, 0.0, 100.0, 150.0]
  f0_b[0, :5] = [110.0, 120.0, 0.0, 0.0, 200.0]
  f0_a[1, :2] = [100.0, 0.0]                                                   # no frame voiced on both sides
  f0_a[3] = 100.0 + np.arange(300)                                             # more frames than one pass of 256 threads
  f0_b[3, :6] = 150.0
  fa, fb = [6, 2, 0, 300], [5, 2, 1, 6]
  dev = lambda x, dt: torch.from_numpy(np.asarray(x, dt)).to(DEV)
  rows = metrics.pitch_compare(dev(f0_a, np.float64), dev(fa, np.int32), dev(f0_b, np.float64), dev(fb, np.int32))
  rows = rows.cpu().numpy()
  for i in range(4):
    _check_row(f"pair {i}", rows[i], oracle.compare(f0_a[i, :fa[i]], f0_b[i, :fb[i]]))
  assert rows[0, 4:].tolist() == [5, 3, 3, 2] and rows[0, 2] == 0.5 and rows[0, 3] == 0.4
  assert np.isnan(rows[1, :3]).all() and rows[1, 3] == 0.5 and np.isnan(rows[2, :4]).all() and rows[2, 4] == 0
  long = np.zeros((1, 300))
  long[0] = 100.0 + np.arange(300)
  both = metrics.pitch_compare(dev(long, np.float64), dev([300], np.int32), dev(long * 1.25, np.float64),
                               dev([300], np.int32)).cpu().numpy()[0]
  _check_row("300 frames", both, oracle.compare(long[0], long[0] * 1.25))
  assert both[metrics.GPE] == 1.0 and both[metrics.VOICED_BOTH] == 300
  # a frame count outside [0, fmax] on the device counts as 0 frames
  out = metrics.pitch_compare(dev(long, np.float64), dev([301], np.int32), dev(long, np.float64), dev([300], np.int32))
  assert np.isnan(out.cpu().numpy()[0, :4]).all()


def test_bit_for_bit_properties():
  a, b = cases.signals()
  lens = list(cases.RAGGED)
  xa, xb = _batch(a, lens), _batch(b, lens)
  ta, tb = metrics.yin_f0(xa, lens), metrics.yin_f0(xb, lens)
  ha, hb = _host(ta), _host(tb)
  assert ha[0][3].any() and hb[0][3].any()
  again = _host(metrics.yin_f0(xb, lens))                                               # the same bits twice
  assert all(x.tobytes() == y.tobytes() for x, y in zip(hb, again))
  for i, n in enumerate(lens):                                                          # B = 1, N = len
    f0, ap, fr = _host(metrics.yin_f0(xb[i:i + 1, :n].contiguous()))
    cols = f0.shape[1]
    assert cols == max(1, int(hb[2][i])) and int(fr[0]) == int(hb[2][i])
    assert f0[0].tobytes() == hb[0][i, :cols].tobytes() and ap[0].tobytes() == hb[1][i, :cols].tobytes(), n
  order = [3, 0, 2, 1]                                                                  # the longest first
  back = _host(metrics.yin_f0(xb[order].contiguous(), [lens[i] for i in order]))
  assert all(x.tobytes() == y[order].tobytes() for x, y in zip(back, hb))
  # the fused call is the two tracker calls chained with the compare call
  rows = metrics.pitch_metrics_enqueue(xa, lens, xb, lens).cpu().numpy()
  chained = metrics.pitch_compare(ta[0], ta[2], tb[0], tb[2]).cpu().numpy()
  assert rows.tobytes() == chained.tobytes()
  # a power-of-two scale changes no bit
  quarter = _host(metrics.yin_f0(xb * 0.25, lens))
  assert all(x.tobytes() == y.tobytes() for x, y in zip(hb, quarter))
  assert metrics.pitch_metrics_enqueue(xa, lens, xb * 0.25, lens).cpu().numpy().tobytes() == rows.tobytes()
  # nothing behind an utterance's end is read
  nan = _host(metrics.yin_f0(_batch(b, lens, fill=np.nan), lens))
  assert all(x.tobytes() == y.tobytes() for x, y in zip(hb, nan))
  # lengths on the device; one outside [0, N] counts as 0 frames
  ld = torch.tensor(lens, dtype=torch.int32, device=DEV)
  on_dev = _host(metrics.yin_f0(xb, ld))
  assert all(x.tobytes() == y.tobytes() for x, y in zip(hb, on_dev))
  assert metrics.pitch_metrics_enqueue(xa, ld, xb, ld).cpu().numpy().tobytes() == rows.tobytes()
  f0, ap, fr = _host(metrics.yin_f0(xb, torch.tensor([6001, -1, 1648, 6000], dtype=torch.int32, device=DEV)))
  assert fr.tolist() == [0, 0, 2, 19] and not f0[:2].any() and f0[2:].tobytes() == hb[0][2:].tobytes()


def test_refusals_leave_the_device_usable():
  a, b = cases.signals()
  xa, xb = _batch(a, [6000]), _batch(b, [6000])

  def good():
    m = metrics.pitch_metrics(xa, None, xb, None)[0]
    assert (m.frames, m.voiced_both, m.gross_pitch_error) == (19, 8, 0.75)

  bad_calls = [
    lambda: metrics.pitch_metrics(xa.cpu(), None, xb, None),                              # a CPU tensor
    lambda: metrics.pitch_metrics(xa.half(), None, xb, None),                             # fp16
    lambda: metrics.pitch_metrics(xa, [6001], xb, None),                                  # a length behind the row
    lambda: metrics.pitch_metrics(xa, [6000, 6000], xb, None),                            # two lengths for one row
    lambda: metrics.pitch_metrics(xa, None, torch.cat([xb, xb]), None),                   # mismatched B
    lambda: metrics.pitch_metrics(xa, torch.tensor([6000], device=DEV), xb, None),        # int64 lengths on the device
    lambda: metrics.yin_f0(xa[0]),
    lambda: metrics.yin_f0(xa, frame_length=4096),
    lambda: metrics.yin_f0(xa, fmin=20.0),
    lambda: metrics.yin_f0(xa, threshold=1.0),
  ]
  for call in bad_calls:
    with pytest.raises(_lib.WgError):
      call()
    good()


# -------------------------------------------------------------------------------------------------------- end to end
@pytest.fixture(scope="module")
def ckpt(tmp_path_factory):
  """(checkpoint folder, hparams): the 64-channel synthetic model of test_gpu_metrics.py saved as 3.pt."""
  from waveglow_amd.checkpoint import CheckpointWaveglow
  hp = HParams(n_channels=64, n_layers=4, n_flows=4, n_early_every=2)
  m = WaveGlow(hp)
  m.load_state_dict(synthetic.to_weightnorm_form(synthetic.make_state_dict(hp, seed=8)))
  folder = tmp_path_factory.mktemp("validate_pitch_ckpt")
  CheckpointWaveglow.from_instances(m, None, hp, 3).save(folder / "3.pt")
  return folder, hp


def test_cli_validate_pitch_metrics_batch_equals_one_by_one(ckpt, tmp_path):
  import pandas
  from waveglow_amd import cli
  from waveglow_amd.audio import float_to_wav, wav_to_float32
  folder, hp = ckpt
  src = tmp_path / "wavs"
  src.mkdir()
  sizes = (3000, 5121, 4096)
  a, b = cases.signals()
  for i, n in enumerate(sizes):
    float_to_wav((a if i != 1 else b)[:n].copy(), src / f"u{i}.wav", sample_rate=hp.sampling_rate)
  tables = []
  for bs in ("3", "1"):
    out = tmp_path / f"val{bs}"
    assert cli.main(["validate", str(folder), str(out), str(src), "--full-run", "--custom-seed", "7", "--batch-size", bs,
                     "--pitch-metrics"]) == 0
    tables.append(pandas.read_csv(out / "total.csv", sep="\t", float_precision="round_trip"))
    assert "F0 RMSE (cents)" in (out / "log.txt").read_text()
  assert list(tables[0].columns) == cases.TODAY[:-1] + cases.PITCH + cases.TODAY[-1:]
  for col in cases.PITCH + ["MCD", "MFCC DTW MCD", "Cosine Similarity (Padded)"]:
    x, y = tables[0][col].to_numpy(), tables[1][col].to_numpy()
    print(col, x.tolist())
    assert x.tobytes() == y.tobytes(), col
  # the original's side of the row is the tracker on the original wav; the synthesis has 256 * mel frames samples
  p = metrics.pitch_params(sampling_rate=hp.sampling_rate)
  for i, n in enumerate(sizes):
    wav, _ = wav_to_float32(src / f"u{i}.wav")
    F = min(metrics.pitch_frames(n, p), metrics.pitch_frames(256 * (n // 256 + 1), p))
    f0 = metrics.yin_f0(torch.from_numpy(np.ascontiguousarray(wav, np.float32))[None].to(DEV))[0].cpu().numpy()[0]
    row = tables[0].iloc[i]
    assert row["# Pitch frames"] == F > 0 and row["# Voiced frames original"] == int((f0[:F] > 0).sum()) > 0
    assert 0 <= row["V/UV error"] <= 1 and 0 <= row["# Voiced frames inferred"] <= F
  out = tmp_path / "plain"
  assert cli.main(["validate", str(folder), str(out), str(src), "--full-run", "--custom-seed", "7", "--batch-size", "3"]) == 0
  assert (out / "total.csv").read_text().splitlines()[0] == "\t".join(cases.TODAY)
  assert "F0 RMSE" not in (out / "log.txt").read_text()
  plain = pandas.read_csv(out / "total.csv", sep="\t", float_precision="round_trip")
  for col in ("MCD", "MFCC DTW MCD", "Cosine Similarity (Padded)", "# Frames"):
    assert plain[col].to_numpy().tobytes() == tables[0][col].to_numpy().tobytes(), col
