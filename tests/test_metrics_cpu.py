"""CPU-side checks of the validation metrics: the numpy restatement the GPU tests compare against (tests/
_metrics_oracle.py) pinned against scipy and hand cases, the tie order of the DTW, the ``validate`` parser, the table's
columns, and the argument refusals of ``wg_metrics_*`` that need no device."""
import ctypes as C
import datetime
from pathlib import Path

import numpy as np
import pytest

import _metrics_oracle as oracle


def _mel(rng, n_mel, T):
  return rng.uniform(-11.5, 2.0, (n_mel, T))


def test_oracle_dct_equals_scipy():
  import scipy.fft
  x = _mel(np.random.default_rng(0), 80, 37)
  ref = scipy.fft.dct(x, type=2, norm="ortho", axis=0)[1:17]
  got = oracle.mfcc(x, 16)
  assert got.shape == (16, 37) and np.max(np.abs(got - ref)) <= 1e-12
  y = _mel(np.random.default_rng(1), 16, 5)
  assert np.max(np.abs(oracle.mfcc(y, 15) - scipy.fft.dct(y, type=2, norm="ortho", axis=0)[1:16])) <= 1e-12


def test_oracle_hand_cases():
  x = _mel(np.random.default_rng(2), 80, 23).astype(np.float32)
  m = oracle.mel_metrics(x, x)
  assert m["mcd"] == 0 and m["penalty"] == 0 and m["frames"] == 23
  assert m["mcd_dtw"] == 0 and m["penalty_dtw"] == 0 and m["frames_dtw"] == 23
  assert abs(m["cosine"] - 1) <= 1e-15
  # one all-zero channel on one side scores 1: the similarity drops by exactly 1 / n_mel
  y = x.copy()
  y[5] = 0
  assert abs(oracle.cosine(x, y) - (1 - 1 / 80)) <= 1e-15
  assert oracle.cosine(np.zeros((4, 3)), np.ones((4, 5))) == 0.0
  # unequal lengths: F = max, penalty 2 - (Ta + Tb) / F; the shorter side's MFCCs are zero behind its end
  fa, fb = oracle.mfcc(x[:, :10]), oracle.mfcc(x)
  mcd, pen, F = oracle.padded_mcd(fa, fb)
  assert F == 23 and pen == 2 - 33 / 23
  assert abs(mcd - np.sum(np.linalg.norm(fb[:, 10:], axis=0)) / 23) <= 1e-12
  # a single frame against many: every cell lies on the only path
  cost, frames, margin = oracle.dtw(fa[:, :1], fb)
  assert frames == 23 and margin == np.inf
  assert abs(cost - np.sum(np.linalg.norm(fb - fa[:, :1], axis=0))) <= 1e-9


def test_oracle_cosine_equals_scipy():
  from scipy.spatial.distance import cosine
  rng = np.random.default_rng(3)
  a, b = _mel(rng, 80, 31), _mel(rng, 80, 40)
  a[7] = 0
  pa = np.zeros((80, 40))
  pa[:, :31] = a
  scores = []
  for u, v in zip(pa, b):
    with np.errstate(all="ignore"):
      s = cosine(u, v) if u.any() and v.any() else np.nan         # scipy: NaN (or an error) for a zero vector
    scores.append(1 if np.isnan(s) else s)
  assert abs(oracle.cosine(a, b) - (1 - np.mean(scores))) <= 1e-12
  assert abs(oracle.cosine(b, a) - (1 - np.mean(scores))) <= 1e-12


@pytest.mark.parametrize("seed,cost,frames", [(1, 8.0, 17), (4, 6.0, 15)])
def test_oracle_tie_order(seed, cost, frames):
  """Integer features: every operation is exact, so the path length depends on the tie order alone."""
  r = np.random.default_rng(seed)
  a, b = np.zeros((16, 9)), np.zeros((16, 12))
  a[0] = r.integers(0, 3, 9)
  b[0] = r.integers(0, 3, 12)
  assert oracle.dtw(a, b)[:2] == (cost, frames)
  others = [oracle.dtw(a, b, order)[:2] for order in oracle.OTHER_ORDERS]
  assert all(c == cost for c, _ in others)
  assert any(f != frames for _, f in others)                     # the case discriminates between tie orders


def test_validate_parser_has_the_reference_arguments():
  from waveglow_amd import cli
  ns = cli.build_parser().parse_args(["validate", "ckpts", "out", "data"])
  assert (ns.checkpoints_dir, ns.output_dir, ns.dataset_dir) == (Path("ckpts"), Path("out"), Path("data"))
  assert ns.sigma == 1.0 and ns.denoiser_strength == 0.0005 and ns.device == "cuda:0" and ns.custom_hparams is None
  assert ns.full_run is False and list(ns.files) == [] and list(ns.custom_checkpoints) == [] and ns.custom_seed is None
  assert ns.batch_size == 1
  ns = cli.build_parser().parse_args(["validate", "c", "o", "d", "--sigma", "0.9", "--denoiser-strength", "0.01", "--device",
                                      "cuda:1", "--custom-hparams", "a=1", "--full-run", "--files", "x.wav", "y.wav",
                                      "--custom-checkpoints", "10", "20", "--custom-seed", "7", "--batch-size", "4"])
  assert ns.sigma == 0.9 and ns.denoiser_strength == 0.01 and ns.device == "cuda:1" and ns.custom_hparams == "a=1"
  assert ns.full_run and ns.files == ["x.wav", "y.wav"] and ns.custom_checkpoints == [10, 20]
  assert ns.custom_seed == 7 and ns.batch_size == 4
  with pytest.raises(SystemExit):
    cli.build_parser().parse_args(["validate", "c", "o", "d", "--sigma", "1.5"])


def test_validate_refuses_a_distributed_run(monkeypatch, tmp_path):
  from waveglow_amd import cli
  monkeypatch.setenv("WORLD_SIZE", "2")
  assert cli.main(["validate", str(tmp_path), str(tmp_path / "out"), str(tmp_path)]) == 1
  assert not (tmp_path / "out").exists()


def test_entry_selection_follows_the_reference():
  import random
  from waveglow_amd.training import Entry
  from waveglow_amd.validation import select_entries
  data = [Entry(f"u{i}", f"u{i}.wav", Path(f"/d/u{i}.wav")) for i in range(5)]
  assert select_entries(data, set(), True, 1) == data
  assert select_entries(data, {"u3.wav", "u1.wav"}, False, 1) == [data[1], data[3]]
  with pytest.raises(AssertionError):
    select_entries(data, {"u3.wav", "nobody.wav"}, False, 1)
  random.seed(1234)
  expect = random.choice(data)
  assert select_entries(data, set(), False, 1234) == [expect]


def test_get_df_columns():
  from waveglow_amd.synthesizer import PcmResult
  from waveglow_amd.training import Entry
  from waveglow_amd.validation import ValidationEntries, ValidationEntry, get_df
  assert get_df(ValidationEntries()).empty
  now = datetime.datetime(2024, 1, 2, 3, 4, 5)
  res = PcmResult(pcm=np.zeros(4, np.int16), sampling_rate=22050, was_overamplified=False, peak=0.5,
                  inference_duration_s=0.1, denoising_duration_s=0.01, timepoint=now)
  e = ValidationEntry(entry=Entry("u0", "u0.wav", Path("/d/u0.wav")), inference_result=res, seed=7, iteration=3, timepoint=now,
                      inferred_duration_s=1.5, diff_frames=1, mfcc_no_coeffs=16, mfcc_dtw_mcd=2.0, mfcc_dtw_penalty=0.1,
                      mfcc_dtw_frames=12, mcd=3.0, mcd_penalty=0.2, mcd_frames=11, cosine_similarity=0.9,
                      denoiser_strength=0.0005, sigma=1.0)
  assert e.structural_similarity is None
  df = get_df(ValidationEntries([e]))
  assert list(df.columns) == [
    "Name", "Subpath", "Timepoint", "Iteration", "Seed", "Sigma", "Denoiser strength", "Inference duration (s)",
    "Denoising duration (s)", "Overamplified?", "Inferred wav duration (s)", "# Difference frames", "Sampling rate (Hz)",
    "# MFCC Coefficients", "MFCC DTW MCD", "MFCC DTW PEN", "# MFCC DTW frames", "MCD", "PEN", "# Frames",
    "Cosine Similarity (Padded)", "Wav path"]
  row = df.iloc[0]
  assert row["Name"] == "u0.wav" and row["Timepoint"] == "2024/01/02 03:04:05" and row["# MFCC DTW frames"] == 12
  assert row["MCD"] == 3.0 and row["PEN"] == 0.2 and row["# Frames"] == 11 and row["Wav path"] == "/d/u0.wav"


def test_metrics_entry_points_validate_arguments_without_a_gpu():
  """wg_metrics_* argument checks run before any device work."""
  from waveglow_amd import _lib, build
  build.build_library()
  lib = _lib.load()
  assert lib.wg_metrics_workspace_bytes(16, 80, 16, 864, 865) >= 16 * 80 * 8 + 16 * 16 * (864 + 865) * 4
  assert lib.wg_metrics_workspace_bytes(1, 80, 16, 4096, 4096) > 0
  for bad in ((0, 80, 16, 10, 10), (1, 80, 80, 10, 10), (1, 80, 0, 10, 10), (1, 129, 16, 10, 10), (1, 80, 16, 4097, 10),
              (1, 80, 16, 10, 4097), (1, 80, 16, 0, 10)):
    assert lib.wg_metrics_workspace_bytes(*bad) == 0, bad
  dummy = (C.c_char * 64)()
  p = C.addressof(dummy)
  big = 1 << 40
  assert lib.wg_metrics_mfcc(None, p, p, 1, 80, 16, 10, p, big, None) == -1 and b"null" in lib.wg_last_error()
  assert lib.wg_metrics_mfcc(p, p, p, 1, 80, 80, 10, p, big, None) == -1 and b"n_mfcc" in lib.wg_last_error()
  assert lib.wg_metrics_mfcc(p, p, p, 1, 80, 16, 4097, p, big, None) == -1 and b"4097" in lib.wg_last_error()
  assert lib.wg_metrics_mfcc(p, p, p, 1, 80, 16, 10, p, 64, None) == -4
  assert lib.wg_metrics_dtw(p, p, p, None, p, p, 1, 16, 10, 10, None) == -1 and b"null" in lib.wg_last_error()
  assert lib.wg_metrics_dtw(p, p, p, p, p, p, 1, 129, 10, 10, None) == -1 and b"K" in lib.wg_last_error()
  assert lib.wg_metrics_dtw(p, p, p, p, p, p, 1, 16, 4097, 10, None) == -1 and b"4097" in lib.wg_last_error()
  assert lib.wg_metrics_dtw(p, p, p, p, p, p, 1, 16, 10, 0, None) == -1
  assert lib.wg_metrics_dtw(p, p, p, p, p, p, 0, 16, 10, 10, None) == -1
  assert lib.wg_metrics_mel(p, p, p, p, None, 1, 80, 16, 10, 10, p, big, None) == -1 and b"null" in lib.wg_last_error()
  assert lib.wg_metrics_mel(p, p, p, p, p, 1, 80, 16, 10, 4097, p, big, None) == -1 and b"4097" in lib.wg_last_error()
  assert lib.wg_metrics_mel(p, p, p, p, p, 1, 16, 16, 10, 10, p, big, None) == -1
  assert lib.wg_metrics_mel(p, p, p, p, p, 1, 80, 16, 10, 10, p, 64, None) == -4


def test_python_layer_refuses_cpu_tensors_before_any_launch():
  import torch
  from waveglow_amd import _lib, metrics
  x = torch.zeros((1, 80, 5))
  for call in (lambda: metrics.mfcc(x), lambda: metrics.dtw_distance(x, None, x, None),
               lambda: metrics.mel_metrics(x, None, x, None), lambda: metrics.mel_metrics_enqueue(x, [5], x, [5])):
    with pytest.raises(_lib.WgError):
      call()
