"""CPU-side checks of the intelligibility metrics: the numpy restatement the GPU tests compare against (tests/
_stoi_oracle.py) on hand cases, its rounding yardstick, the ``validate`` flag, the table's columns, and the argument
refusals of ``wg_stoi`` and of the Python layer that need no device."""
import ctypes as C
import datetime
from pathlib import Path

import numpy as np
import pytest

import _pitch_cases
import _stoi_cases as cases
import _stoi_oracle as oracle

TODAY, PITCH, STOI = _pitch_cases.TODAY, _pitch_cases.PITCH, cases.STOI_COLUMNS
BAND_TABLE = [(7, 9), (9, 11), (11, 14), (14, 17), (17, 22), (22, 27), (27, 34), (34, 43), (43, 55), (55, 69), (69, 87),
              (87, 109), (109, 138), (138, 174), (174, 219)]


def test_band_table_and_window():
  assert [tuple(r) for r in oracle.band_table().tolist()] == BAND_TABLE
  i = np.arange(256)
  assert np.max(np.abs(oracle.window() - (0.5 - 0.5 * np.cos(2 * np.pi * (i + 1) / 257)))) <= 1e-15
  from waveglow_amd import metrics
  assert [tuple(r) for r in metrics.stoi_band_table().tolist()] == BAND_TABLE and metrics.stoi_band_table().dtype == np.int32
  assert metrics.stoi_window().tobytes() == oracle.window().tobytes()          # device and oracle share the window's bits


def test_frame_count_formula():
  """The exclusive end of range(0, n - 256, 128): 256 + 128 k samples have k frames, not k + 1."""
  from waveglow_amd import metrics
  for count in (oracle.frame_count, metrics.stoi_frames):
    assert [count(n) for n in (0, 256, 257, 384, 385)] == [0, 0, 1, 1, 2]
    assert [count(256 + 128 * k) for k in (1, 2, 30)] == [1, 2, 30]
  x = cases.stationary(4)
  assert [oracle.stoi(x[:n], x[:n])["frames"] for n in (0, 256, 257, 384, 385)] == [0, 0, 1, 1, 2]


def test_identical_signals_give_one():
  for n in cases.LENGTHS:
    r = cases.reference(n, None)
    assert abs(r["stoi"] - 1) <= 1e-12 and abs(r["estoi"] - 1) <= 1e-12, r
    assert r["segments"] == r["frames_kept"] - 30 > 0


def test_silence_gives_exactly_zero_with_every_frame_kept():
  z = np.zeros(20000, np.float32)
  r = oracle.stoi(z, z)
  assert r["stoi"] == 0.0 and r["estoi"] == 0.0
  assert (r["frames"], r["frames_kept"], r["segments"]) == (155, 155, 125)


def test_stationary_noise_keeps_every_frame_and_needs_thirty_one():
  for frames, segments in ((30, 0), (31, 1)):
    x = cases.stationary(frames)
    assert len(x) == 256 + 128 * frames
    r = oracle.stoi(x, cases.add_noise(x, 5.0))
    assert (r["frames"], r["frames_kept"], r["segments"]) == (frames, frames, segments)
    if segments:
      assert 0 < r["estoi"] < 1 and 0 < r["stoi"] < 1
    else:
      assert np.isnan(r["stoi"]) and np.isnan(r["estoi"])


def test_values_fall_with_the_noise():
  x = cases.clean(cases.LENGTHS[0])
  got = [oracle.stoi(x, cases.add_noise(x, snr)) for snr in (20.0, 5.0, -5.0)]
  print([(r["stoi"], r["estoi"]) for r in got])
  for key in ("stoi", "estoi"):
    assert 1 > got[0][key] > got[1][key] > got[2][key] > 0


def test_the_metric_is_not_symmetric():
  x, y = cases.pair(cases.LENGTHS[0], -5.0)
  a, b = oracle.stoi(x, y), oracle.stoi(y, x)
  assert a["frames_kept"] != b["frames_kept"]                  # the gate runs on the first argument
  assert abs(a["stoi"] - b["stoi"]) > 1e-3 and abs(a["estoi"] - b["estoi"]) > 1e-3


def test_a_click_in_silence_keeps_one_or_two_frames():
  for kept in (1, 2):
    x = cases.click(kept)
    r = oracle.stoi(x, x)
    assert (r["frames"], r["frames_kept"], r["segments"]) == (155, kept, 0) and r["margin"] > 1.0


def test_shared_cases_are_pinned_and_their_lengths_are_the_stated_ones():
  """margin > 1e-6 dB is the condition under which the mask, and with it every count, is pinned."""
  assert [len(cases.clean(n)) for n in cases.LENGTHS] == list(cases.LENGTHS_10K) == [20000, 30353, 10000]
  assert cases.clean(cases.LENGTHS[0]).dtype == np.float32
  assert abs(float(np.max(np.abs(cases.speech_22k()))) - 0.5) < 1e-3
  for n, snr in cases.CASES:
    r = cases.reference(n, snr)
    print(n, snr, r)
    assert r["margin"] > 1e-6
    assert r["frames"] == oracle.frame_count(len(cases.clean(n))) and r["segments"] > 0
    assert 0.25 * r["frames"] < r["frames_kept"] < 0.75 * r["frames"]            # real pauses exist


def test_rounding_yardstick():
  """The largest |fp64 oracle - longdouble restatement| over the shared cases is at most 1e-12 (4.8e-15 when this was
  written), so the device bar of 1e-10 is at least 100 times the oracle's own rounding."""
  if np.finfo(np.longdouble).eps >= np.finfo(np.float64).eps:
    pytest.fail("np.longdouble is no wider than fp64 here: the yardstick cannot be taken")
  worst = 0.0
  for n, snr in cases.CASES:
    r, l = cases.reference(n, snr), oracle.stoi_longdouble(*cases.pair(n, snr))
    assert (r["frames"], r["frames_kept"], r["segments"]) == (l["frames"], l["frames_kept"], l["segments"])
    worst = max(worst, abs(r["stoi"] - l["stoi"]), abs(r["estoi"] - l["estoi"]))
  print(f"largest |fp64 - longdouble| over the shared cases: {worst:.3e}")
  assert worst <= 1e-12


def test_validate_parser_takes_intelligibility_metrics():
  from waveglow_amd import cli
  ns = cli.build_parser().parse_args(["validate", "c", "o", "d"])
  assert ns.intelligibility_metrics is False and ns.pitch_metrics is False
  ns = cli.build_parser().parse_args(["validate", "c", "o", "d", "--intelligibility-metrics", "--batch-size", "3"])
  assert ns.intelligibility_metrics is True and ns.pitch_metrics is False and ns.batch_size == 3
  assert "--intelligibility-metrics" in cli.__doc__


def test_get_df_columns_with_and_without_intelligibility_fields():
  from waveglow_amd.synthesizer import PcmResult
  from waveglow_amd.training import Entry
  from waveglow_amd.validation import ValidationEntries, ValidationEntry, get_df
  now = datetime.datetime(2024, 1, 2, 3, 4, 5)
  res = PcmResult(pcm=np.zeros(4, np.int16), sampling_rate=22050, was_overamplified=False, peak=0.5,
                  inference_duration_s=0.1, denoising_duration_s=0.01, timepoint=now)

  def entry(**more):
    return ValidationEntry(entry=Entry("u0", "u0.wav", Path("/d/u0.wav")), inference_result=res, seed=7, iteration=3,
                           timepoint=now, inferred_duration_s=1.5, diff_frames=1, mfcc_no_coeffs=16, mfcc_dtw_mcd=2.0,
                           mfcc_dtw_penalty=0.1, mfcc_dtw_frames=12, mcd=3.0, mcd_penalty=0.2, mcd_frames=11,
                           cosine_similarity=0.9, denoiser_strength=0.0005, sigma=1.0, **more)

  plain = entry()
  assert plain.stoi is None and plain.estoi is None and plain.stoi_frames is None and plain.stoi_frames_kept is None
  assert list(get_df(ValidationEntries([plain])).columns) == TODAY
  pitch = dict(f0_rmse_cents=35.5, f0_rmse_hz=4.25, gross_pitch_error=0.125, vuv_error=0.0625, pitch_frames=16,
               voiced_frames_orig=9, voiced_frames_inferred=8)
  intel = dict(stoi=0.875, estoi=0.75, stoi_frames=155, stoi_frames_kept=77)
  assert list(get_df(ValidationEntries([entry(**pitch)])).columns) == TODAY[:-1] + PITCH + TODAY[-1:]
  df = get_df(ValidationEntries([entry(**intel)]))
  assert list(df.columns) == TODAY[:-1] + STOI + TODAY[-1:] and len(df.columns) == 26
  assert [df.iloc[0][c] for c in STOI] == [0.875, 0.75, 155, 77]
  df = get_df(ValidationEntries([entry(**pitch, **intel)]))
  assert list(df.columns) == TODAY[:-1] + PITCH + STOI + TODAY[-1:] and len(df.columns) == 33
  assert [df.iloc[0][c] for c in STOI] == [0.875, 0.75, 155, 77] and df.iloc[0]["Wav path"] == "/d/u0.wav"


def test_stoi_entry_points_validate_arguments_without_a_gpu():
  """wg_stoi's argument checks run before any device work."""
  from waveglow_amd import _lib, build
  build.build_library()
  lib = _lib.load()
  # energies and kept lists of 155 frames, band spectra of 154, sums of 125 segments
  assert lib.wg_stoi_workspace_bytes(1, 20000) >= 155 * 12 + 2 * 15 * 154 * 8 + 125 * 16
  assert lib.wg_stoi_workspace_bytes(16, 100000) >= 16 * lib.wg_stoi_workspace_bytes(1, 100000) // 2
  assert lib.wg_stoi_workspace_bytes(1, 1) > 0 and lib.wg_stoi_workspace_bytes(65535, 1 << 21) > 0
  for B, n in ((0, 20000), (-1, 20000), (65536, 20000), (1, 0), (1, -5), (1, (1 << 21) + 1)):
    assert lib.wg_stoi_workspace_bytes(B, n) == 0, (B, n)
  dummy = (C.c_char * 128)()
  p = (C.addressof(dummy) + 15) & ~15                                          # the cos/sin table is read as 16-byte pairs
  big = 1 << 40
  ok = _lib.WgStoiParams(p, p, p)
  assert lib.wg_stoi(p, p, p, p, 1, 20000, C.byref(ok), p, p, 64, None) == -4           # the workspace is too small
  for args in ((None, p, p, p), (p, None, p, p), (p, p, None, p), (p, p, p, None)):
    assert lib.wg_stoi(*args, 1, 20000, C.byref(ok), p, p, big, None) == -1 and b"null" in lib.wg_last_error()
  assert lib.wg_stoi(p, p, p, p, 1, 20000, None, p, p, big, None) == -1 and b"null" in lib.wg_last_error()
  assert lib.wg_stoi(p, p, p, p, 1, 20000, C.byref(ok), None, p, big, None) == -1
  assert lib.wg_stoi(p, p, p, p, 1, 20000, C.byref(ok), p, None, big, None) == -1
  for bad in (_lib.WgStoiParams(None, p, p), _lib.WgStoiParams(p, None, p), _lib.WgStoiParams(p, p, None)):
    assert lib.wg_stoi(p, p, p, p, 1, 20000, C.byref(bad), p, p, big, None) == -1 and b"table" in lib.wg_last_error()
  assert lib.wg_stoi(p, p, p, p, 1, 20000, C.byref(_lib.WgStoiParams(p, p, p + 8)), p, p, big, None) == -1
  assert b"aligned" in lib.wg_last_error()
  for B, n in ((0, 20000), (65536, 20000), (1, 0), (1, (1 << 21) + 1)):
    assert lib.wg_stoi(p, p, p, p, B, n, C.byref(ok), p, p, big, None) == -1 and b"stoi" in lib.wg_last_error()


def test_python_layer_refuses_bad_arguments_before_any_launch():
  import torch
  import waveglow_amd
  from waveglow_amd import _lib, metrics
  assert waveglow_amd.intelligibility_metrics is metrics.intelligibility_metrics
  assert waveglow_amd.IntelligibilityMetrics is metrics.IntelligibilityMetrics and waveglow_amd.stoi is metrics.stoi
  assert (metrics.STOI_FRAME_TILE, metrics.STOI_SEGMENT_TILE, metrics.STOI_RATE) == (8, 4, 10000)
  x = torch.zeros((1, 4000))
  for call in (lambda: metrics.stoi(x, None, x, None), lambda: metrics.stoi_enqueue(x, [4000], x, [4000]),     # CPU tensors
               lambda: metrics.intelligibility_metrics(x, None, x, None),
               lambda: metrics.intelligibility_metrics_enqueue(x, None, x, None, sampling_rate=10000),
               lambda: metrics.stoi([0.0] * 4000, None, x, None),
               lambda: metrics.stoi(x.double(), None, x, None), lambda: metrics.stoi(x[0], None, x, None),
               lambda: metrics.intelligibility_metrics(x.half(), None, x, None),
               # a rate the resampler refuses is reported before the tensors are looked at
               lambda: metrics.intelligibility_metrics(x, None, x, None, sampling_rate=10001),
               lambda: metrics.intelligibility_metrics(x, None, x, None, sampling_rate=22050.5),
               lambda: metrics.intelligibility_metrics(x, None, x, None, sampling_rate=0)):
    with pytest.raises(_lib.WgError):
      call()
  with pytest.raises(_lib.WgError, match="max\\(up, down\\)"):
    metrics.intelligibility_metrics(x, None, x, None, sampling_rate=10001)
  m = metrics.rows_to_intelligibility_metrics(torch.tensor([[0.5, 0.25, 155.0, 77.0, 47.0, 0.0, 0.0, 0.0],
                                                            [float("nan"), float("nan"), 2.0, 2.0, 0.0, 0.0, 0.0, 0.0]]))
  assert m[0] == metrics.IntelligibilityMetrics(stoi=0.5, estoi=0.25, frames=155, frames_kept=77, segments=47)
  assert np.isnan(m[1].stoi) and np.isnan(m[1].estoi) and (m[1].frames, m[1].frames_kept, m[1].segments) == (2, 2, 0)
