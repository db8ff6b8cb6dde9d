"""CPU-side checks of the pitch metrics: the numpy restatement the GPU tests compare against (tests/_pitch_oracle.py) on
hand cases, the pair row of hand-made tracks, the ``validate`` flag, the table's columns, and the argument refusals of
``wg_pitch_*`` and of the Python layer that need no device."""
import ctypes as C
import datetime
from pathlib import Path

import numpy as np
import pytest

import _pitch_cases as cases
import _pitch_oracle as oracle

TODAY, PITCH = cases.TODAY, cases.PITCH


def _sine100(**params):
  return oracle.yin(np.sin(2 * np.pi * np.arange(4000) / 100).astype(np.float32), **params)


def test_oracle_sine_of_period_100_with_the_defaults_reads_high():
  """Every frame picks lag 100 with d'(100) ~ 0.  The interpolated f0 lies 1 / (2 tau^2) = 5e-5 above sr / tau: d'(tau) =
  d(tau) tau / sum d carries the factor tau, so d'(99) / d'(101) = 99 / 101 where d(99) = d(101), and the parabola's vertex
  sits at -1 / (2 tau).  Measured 4.5e-5 .. 5.5e-5 on the 11 frames, f0 = 220.5100 .. 220.5121."""
  t = _sine100()
  assert t["frames"] == (4000 - 1024 - 368) // 256 + 1 == 11
  assert np.all(t["tau"] == 100) and np.all(t["aperiodicity"] < 1e-6)
  rel = t["f0"] / 220.5 - 1
  print("f0 / 220.5 - 1:", rel)
  assert np.all(np.abs(rel - 1 / (2 * 100.0 ** 2)) <= 1e-5)


def test_oracle_sine_of_period_100():
  """f0 = 220.5 on every frame to 1e-6 relative.  With lags up to 368 the interpolation of d' misses that by 5e-5 (the test
  above), so the case runs where the definition takes no interpolation: fmin = 220.5 makes lag 100 the last lag
  (tau_max = ceil(22050 / 220.5) = 100), the search enters below the threshold before it, the walk ends at tau_max and
  f0 = sr / 100."""
  assert oracle.lags(22050, 220.5, 600.0) == (36, 100)
  t = _sine100(fmin=220.5)
  assert t["frames"] == (4000 - 1024 - 100) // 256 + 1 == 12 and np.all(t["tau"] == 100)
  assert np.max(np.abs(t["f0"] / 220.5 - 1)) <= 1e-6
  assert np.all(t["aperiodicity"] < 1e-6) and t["margin"] > 1e-7


def test_oracle_silence_and_noise_are_unvoiced():
  z = oracle.yin(np.zeros(3000, np.float32))
  assert z["frames"] == 7 and not z["f0"].any() and np.all(z["aperiodicity"] == 1.0)
  w = oracle.yin(np.random.default_rng(0).standard_normal(4000).astype(np.float32))
  assert w["frames"] == 11 and not w["f0"].any() and np.all(w["aperiodicity"] >= 0.1)


def test_oracle_frame_counts_at_the_edges():
  tau_min, tau_max = oracle.lags()
  assert (tau_min, tau_max) == (36, 368)
  need = 1024 + tau_max
  x = cases.signals()[0]
  assert [oracle.yin(x[:n])["frames"] for n in (need - 1, need, need + 255, need + 256)] == [0, 1, 1, 2]
  assert [oracle.frame_count(n, 1024, 256, tau_max) for n in (0, need - 1, need, need + 255, need + 256)] == [0, 0, 1, 1, 2]
  assert oracle.lags(22050, 86.5, 2000.0) == (11, 255) and oracle.lags(22050, 86.2, 2000.0) == (11, 256)
  assert oracle.lags(22050, 21.54, 600.0) == (36, 1024)


def test_oracle_power_of_two_scale_changes_no_bit():
  x = cases.signals()[1][:2500]
  t1, t2 = oracle.yin(x), oracle.yin(x * np.float32(0.25))
  assert t1["frames"] == 5 and t1["f0"].any()
  assert t1["f0"].tobytes() == t2["f0"].tobytes() and t1["aperiodicity"].tobytes() == t2["aperiodicity"].tobytes()


def test_oracle_fast_difference_is_the_plain_loop():
  x = cases.signals()[1][:300].astype(np.float64)
  assert oracle.difference(x[:64 + 200], 64, 200).tobytes() == oracle._difference_fast(x[:64 + 200], 64, 200).tobytes()
  d = oracle.difference(x[:64 + 200], 64, 200)
  assert d[0] == 0 and abs(d[7] - np.sum((x[:64] - x[7:71]) ** 2)) <= 1e-12 * d[7]


def test_oracle_reproduces_the_prototype_on_the_test_signals():
  """The counts and stability figures recorded with the definition (tests/test_gpu_pitch.py relies on them)."""
  row, a, b = cases.row("defaults"), cases.tracks("defaults", 0), cases.tracks("defaults", 1)
  assert (a["frames"], b["frames"], row["frames"]) == (19, 19, 19)
  assert row["voiced_both"] == 8 and round(row["vuv_error"] * 19) == 4 and round(row["gpe"] * 8) == 6
  assert min(a["margin"], b["margin"]) >= 2.3e-5 and row["gpe_margin"] >= 4.9e-2 and min(a["den"], b["den"]) >= 3.0e-3
  for name in ("tau255", "tau256", "limits", "hop1"):
    t = cases.tracks(name, 0)
    assert t["margin"] >= 1.0e-4 and t["den"] >= 1.4e-3, (name, t["margin"], t["den"])
    assert t["frames"] > 0 and t["f0"].any()


def test_pair_rows_of_hand_made_tracks():
  a = np.array([100.0, 0.0, 200.0, 0.0, 100.0, 150.0])
  b = np.array([110.0, 120.0, 0.0, 0.0, 200.0])
  r = oracle.compare(a, b)
  assert (r["frames"], r["voiced_a"], r["voiced_b"], r["voiced_both"]) == (5, 3, 3, 2)
  assert r["vuv_error"] == 2 / 5 and r["gpe"] == 1 / 2
  assert abs(r["f0_rmse_hz"] - np.sqrt((10.0 ** 2 + 100.0 ** 2) / 2)) <= 1e-12
  assert abs(r["f0_rmse_cents"] - np.sqrt(((1200 * np.log2(1.1)) ** 2 + 1200.0 ** 2) / 2)) <= 1e-9
  assert abs(r["gpe_margin"] - 0.1) <= 1e-12
  none = oracle.compare(np.array([100.0, 0.0]), np.array([0.0, 0.0]))          # no frame voiced on both sides
  assert np.isnan([none["f0_rmse_cents"], none["f0_rmse_hz"], none["gpe"]]).all() and none["vuv_error"] == 0.5
  assert (none["frames"], none["voiced_a"], none["voiced_b"], none["voiced_both"]) == (2, 1, 0, 0)
  empty = oracle.compare(np.zeros(0), np.array([100.0]))                        # no frame at all
  assert np.isnan([empty["f0_rmse_cents"], empty["f0_rmse_hz"], empty["gpe"], empty["vuv_error"]]).all()
  assert (empty["frames"], empty["voiced_a"], empty["voiced_b"], empty["voiced_both"]) == (0, 0, 0, 0)


def test_validate_parser_takes_pitch_metrics():
  from waveglow_amd import cli
  assert cli.build_parser().parse_args(["validate", "c", "o", "d"]).pitch_metrics is False
  ns = cli.build_parser().parse_args(["validate", "c", "o", "d", "--pitch-metrics", "--batch-size", "3"])
  assert ns.pitch_metrics is True and ns.batch_size == 3


def test_get_df_columns_with_and_without_pitch_fields():
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
  assert plain.f0_rmse_cents is None and plain.pitch_frames is None and plain.voiced_frames_inferred is None
  df = get_df(ValidationEntries([plain]))
  assert len(TODAY) == 22 and list(df.columns) == TODAY
  full = entry(f0_rmse_cents=35.5, f0_rmse_hz=4.25, gross_pitch_error=0.125, vuv_error=0.0625, pitch_frames=16,
               voiced_frames_orig=9, voiced_frames_inferred=8)
  df = get_df(ValidationEntries([full]))
  assert list(df.columns) == TODAY[:-1] + PITCH + TODAY[-1:] and len(df.columns) == 29
  row = df.iloc[0]
  assert [row[c] for c in PITCH] == [35.5, 4.25, 0.125, 0.0625, 16, 9, 8]
  assert row["Cosine Similarity (Padded)"] == 0.9 and row["Wav path"] == "/d/u0.wav"


def _params(lib_mod, **kw):
  base = dict(sampling_rate=22050.0, threshold=0.1, frame_length=1024, hop_length=256, tau_min=36, tau_max=368)
  base.update(kw)
  return lib_mod.WgPitchParams(**base)


def test_pitch_entry_points_validate_arguments_without_a_gpu():
  """wg_pitch_* argument checks run before any device work."""
  from waveglow_amd import _lib, build
  build.build_library()
  lib = _lib.load()
  ok = _params(_lib)
  need = 1024 + 368
  assert [lib.wg_pitch_frames(C.byref(ok), n) for n in (0, need - 1, need, need + 255, need + 256, 221184)] == \
      [0, 0, 1, 1, 2, 859]
  assert lib.wg_pitch_workspace_bytes(C.byref(ok), 16, 221184, 221184) >= 16 * 859 * 8 * 4 + 2 * 16 * 4
  assert lib.wg_pitch_workspace_bytes(C.byref(ok), 1, 10, 10) > 0                  # too short for a frame: NaN rows, no error
  bad_params = [_params(_lib, frame_length=15), _params(_lib, frame_length=2049), _params(_lib, hop_length=0),
                _params(_lib, tau_min=1), _params(_lib, tau_min=368), _params(_lib, tau_max=1025),
                _params(_lib, threshold=0.0), _params(_lib, threshold=1.0), _params(_lib, threshold=float("nan")),
                _params(_lib, sampling_rate=0.0)]
  dummy = (C.c_char * 64)()
  p = C.addressof(dummy)
  big = 1 << 40
  for bad in bad_params:
    assert lib.wg_pitch_frames(C.byref(bad), 4000) == -1 and b"pitch" in lib.wg_last_error()
    assert lib.wg_pitch_workspace_bytes(C.byref(bad), 1, 4000, 4000) == 0
    assert lib.wg_pitch_yin(p, p, C.byref(bad), p, p, p, 1, 4000, 11, None) == -1 and b"pitch" in lib.wg_last_error()
    assert lib.wg_pitch_metrics(p, p, 4000, p, p, 4000, C.byref(bad), p, 1, p, big, None) == -1
  for limit in (_params(_lib, frame_length=16), _params(_lib, frame_length=2048, tau_max=1024), _params(_lib, tau_min=2)):
    assert lib.wg_pitch_frames(C.byref(limit), 100000) > 0
  assert lib.wg_pitch_frames(C.byref(ok), -1) == -1
  assert lib.wg_pitch_frames(None, 10) == -1 and b"null" in lib.wg_last_error()
  assert lib.wg_pitch_workspace_bytes(C.byref(ok), 0, 4000, 4000) == 0
  assert lib.wg_pitch_workspace_bytes(C.byref(ok), 1, 0, 4000) == 0
  assert lib.wg_pitch_workspace_bytes(None, 1, 4000, 4000) == 0
  assert lib.wg_pitch_yin(None, p, C.byref(ok), p, p, p, 1, 4000, 11, None) == -1 and b"null" in lib.wg_last_error()
  assert lib.wg_pitch_yin(p, p, None, p, p, p, 1, 4000, 11, None) == -1 and b"null" in lib.wg_last_error()
  assert lib.wg_pitch_yin(p, p, C.byref(ok), p, p, None, 1, 4000, 11, None) == -1
  assert lib.wg_pitch_yin(p, p, C.byref(ok), p, p, p, 0, 4000, 11, None) == -1
  assert lib.wg_pitch_yin(p, p, C.byref(ok), p, p, p, 1, 0, 11, None) == -1
  assert lib.wg_pitch_yin(p, p, C.byref(ok), p, p, p, 1, 4000, 10, None) == -1 and b"fmax" in lib.wg_last_error()
  assert lib.wg_pitch_yin(p, p, C.byref(ok), p, p, p, 1, 100, 0, None) == -1           # a track has at least one column
  assert lib.wg_pitch_compare(p, p, p, p, None, 1, 11, 11, None) == -1 and b"null" in lib.wg_last_error()
  assert lib.wg_pitch_compare(p, p, p, p, p, 0, 11, 11, None) == -1
  assert lib.wg_pitch_compare(p, p, p, p, p, 1, 0, 11, None) == -1
  assert lib.wg_pitch_compare(p, p, p, p, p, 1, 11, 0, None) == -1
  assert lib.wg_pitch_metrics(p, p, 4000, p, None, 4000, C.byref(ok), p, 1, p, big, None) == -1
  assert lib.wg_pitch_metrics(p, p, 4000, p, p, 0, C.byref(ok), p, 1, p, big, None) == -1
  assert lib.wg_pitch_metrics(p, p, 4000, p, p, 4000, C.byref(ok), p, 65536, p, big, None) == -1
  assert lib.wg_pitch_metrics(p, p, 4000, p, p, 4000, C.byref(ok), p, 1, p, 64, None) == -4


def test_python_layer_refuses_bad_arguments_before_any_launch():
  import torch
  from waveglow_amd import _lib, metrics
  import waveglow_amd
  assert waveglow_amd.pitch_metrics is metrics.pitch_metrics and waveglow_amd.PitchMetrics is metrics.PitchMetrics
  p = metrics.pitch_params()
  assert (p.tau_min, p.tau_max, p.frame_length, p.hop_length, p.sampling_rate, p.threshold) == (36, 368, 1024, 256, 22050.0, 0.1)
  assert [metrics.pitch_frames(n, p) for n in (1391, 1392, 1647, 1648)] == [0, 1, 1, 2]
  q = metrics.pitch_params(frame_length=2048, fmin=21.54)
  assert (q.tau_min, q.tau_max) == (36, 1024)
  for bad in (dict(frame_length=15), dict(frame_length=2049), dict(frame_length=64.5), dict(hop_length=0), dict(fmin=21.5),
              dict(fmin=600.0, fmax=600.0), dict(fmin=700.0), dict(fmin=0.0), dict(threshold=0.0), dict(threshold=1.0),
              dict(threshold=float("nan")), dict(sampling_rate=0), dict(fmin="low")):
    with pytest.raises(_lib.WgError):
      metrics.pitch_params(**bad)
    with pytest.raises(_lib.WgError):                           # the parameters are checked before the tensors
      metrics.yin_f0(torch.zeros((1, 4000)), **bad)
  x = torch.zeros((1, 4000))
  f0 = torch.zeros((1, 11), dtype=torch.float64)
  fr = torch.zeros(1, dtype=torch.int32)
  for call in (lambda: metrics.yin_f0(x), lambda: metrics.yin_f0(x, [4000]), lambda: metrics.pitch_metrics(x, None, x, None),
               lambda: metrics.pitch_metrics_enqueue(x, [4000], x, [4000]), lambda: metrics.pitch_compare(f0, fr, f0, fr),
               lambda: metrics.yin_f0([0.0] * 4000),
               lambda: metrics.yin_f0(x.double()), lambda: metrics.yin_f0(x[0]), lambda: metrics.yin_f0(x[:0]),     # dtype, shape
               lambda: metrics.pitch_metrics_enqueue(x, None, x.half(), None),
               lambda: metrics.pitch_compare(f0.float(), fr, f0, fr), lambda: metrics.pitch_compare(f0, fr.long(), f0, fr),
               lambda: metrics._lengths("lengths", [4000, 4000], x), lambda: metrics._lengths("lengths", [4001], x),
               lambda: metrics._lengths("lengths", [-1], x), lambda: metrics._lengths("lengths", torch.tensor([1, 2]), x)):
    with pytest.raises(_lib.WgError):
      call()
