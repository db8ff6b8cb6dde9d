"""CPU-side checks of the per-utterance likelihood: the numpy restatement the GPU tests compare against (tests/
_likelihood_oracle.py) pinned to the reference's own forward outputs and loss, hand cases, the ``validate`` flag, the
table's columns, and the argument refusals of ``wg_nll`` / ``wg_forward`` and of the Python layer that need no
device."""
import ctypes as C
import datetime
import math
from pathlib import Path

import numpy as np
import pytest

import _likelihood_oracle as oracle
import _pitch_cases
import _stoi_cases
from _cases import Case

TODAY, PITCH, STOI = _pitch_cases.TODAY, _pitch_cases.PITCH, _stoi_cases.STOI_COLUMNS
LIKELIHOOD = ["NLL (nats/sample)", "Bits per sample", "z variance", "# Likelihood frames"]


def _reference_forward(c):
  """The reference's fwd_* arrays of a golden case: z, [log_s_k], log|det W_k| per column."""
  z = c.npz["fwd_z"]
  B, _, L = z.shape
  log_s = [c.npz[f"fwd_log_s_{k}"] for k in range(c.hp.n_flows)]
  return z, log_s, c.npz["fwd_log_det"].astype(np.float64) / (B * L)


@pytest.mark.parametrize("name", ["tiny", "c64", "c256"])
def test_oracle_reproduces_the_reference_loss(name):
  """sum n_b nll_b / sum n_b over the dense batch is WaveGlowLoss (train.py:31-45) of the reference's own forward outputs:
  the bar test_forward_golden holds the device loss to on the same arrays."""
  c = Case(name)
  z, log_s, logdets = _reference_forward(c)
  rows, track, _ = oracle.likelihood_rows(z, log_s, logdets, None, 1.0)
  loss = float(c.npz["fwd_loss"])
  got = oracle.batch_mean(rows)
  print(f"{name}: oracle {got:.9f}, reference {loss:.9f}")
  assert abs(got - loss) <= 2e-6 * max(1.0, abs(loss))
  assert rows[:, 5].tolist() == [8.0 * z.shape[2]] * z.shape[0]
  # the frame track, times 256, sums to the row (the last frame of these cases is a partial one)
  assert z.shape[2] % 32 != 0 and track.shape == (z.shape[0], (z.shape[2] + 31) // 32)
  np.testing.assert_allclose(256.0 * track.sum(axis=1), rows[:, 0] * rows[:, 5], rtol=1e-12, atol=1e-12)


@pytest.mark.parametrize("sigma", [1.0, 0.7])
def test_all_zero_inputs(sigma):
  z = np.zeros((2, 8, 96))
  log_s = [np.zeros((2, h, 96)) for h in (4, 3)]
  rows, track, yard = oracle.likelihood_rows(z, log_s, [0.0, 0.0], [3, 2], sigma)
  assert rows[:, 0].tolist() == [0.0, 0.0]
  assert np.allclose(rows[:, 1], 0.5 * math.log2(2 * math.pi * sigma * sigma), rtol=0, atol=1e-15)
  assert rows[:, 5].tolist() == [768.0, 512.0] and rows[:, 6:].tolist() == [[0.0, 0.0]] * 2 and yard.tolist() == [0.0, 0.0]
  assert track[0].tolist() == [0.0] * 3 and track[1, :2].tolist() == [0.0] * 2 and math.isnan(track[1, 2])


def test_hand_case_terms_track_and_nan_behind_the_utterance():
  rng = np.random.default_rng(5)
  B, L, frames, sigma, logdets = 3, 128, [4, 1, 2], 0.8, [0.25, -0.5, 0.125]
  z = rng.standard_normal((B, 8, L))
  log_s = [rng.standard_normal((B, h, L)) * 0.1 for h in (4, 3, 2)]
  poisoned = [np.array(t) for t in (z, *log_s)]
  for b, f in enumerate(frames):
    for t in poisoned:
      t[b, :, 32 * f:] = np.nan                         # nothing behind an utterance is read
  rows, track, _ = oracle.likelihood_rows(poisoned[0], poisoned[1:], logdets, frames, sigma)
  assert np.isfinite(rows).all()
  for b, f in enumerate(frames):
    Lb = 32 * f
    z2 = float(np.sum(z[b, :, :Lb] ** 2))
    ls = float(sum(np.sum(t[b, :, :Lb]) for t in log_s))
    want = (z2 / (2 * sigma ** 2) - ls - Lb * sum(logdets)) / (8 * Lb)
    assert abs(rows[b, 0] - want) <= 1e-13 and rows[b, 5] == 8 * Lb and abs(rows[b, 4] - Lb * sum(logdets)) <= 1e-13
    assert abs(rows[b, 1] - (want + 0.5 * math.log(2 * math.pi * sigma ** 2)) / math.log(2)) <= 1e-13
    assert abs(rows[b, 6] - z[b, :, :Lb].mean()) <= 1e-13 and abs(rows[b, 7] - z[b, :, :Lb].var()) <= 1e-12
    assert np.isfinite(track[b, :f]).all() and np.isnan(track[b, f:]).all()
    assert abs(256.0 * track[b, :f].sum() - rows[b, 0] * rows[b, 5]) <= 1e-10
  # a count outside [1, L / 32] scores nothing
  rows, track, _ = oracle.likelihood_rows(z, log_s, logdets, [0, 5, 4], sigma)
  assert rows[:2, 5].tolist() == [0.0, 0.0] and np.isnan(rows[:2, 0]).all() and np.isnan(track[:2]).all()
  assert np.isfinite(rows[2]).all()


def test_validate_parser_takes_likelihood():
  from waveglow_amd import cli
  ns = cli.build_parser().parse_args(["validate", "c", "o", "d"])
  assert ns.likelihood is False and ns.pitch_metrics is False and ns.intelligibility_metrics is False
  assert ns.resample_inputs is False and ns.batch_size == 1 and ns.sigma == 1.0 and ns.denoiser_strength == 0.0005
  ns = cli.build_parser().parse_args(["validate", "c", "o", "d", "--likelihood", "--batch-size", "3"])
  assert ns.likelihood is True and ns.pitch_metrics is False and ns.intelligibility_metrics is False and ns.batch_size == 3
  assert "--likelihood" in cli.__doc__


def test_get_df_columns_with_and_without_likelihood_fields():
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
  assert plain.nll is None and plain.bits_per_sample is None and plain.z_variance is None
  assert plain.likelihood_frames is None
  assert list(get_df(ValidationEntries([plain])).columns) == TODAY
  pitch = dict(f0_rmse_cents=35.5, f0_rmse_hz=4.25, gross_pitch_error=0.125, vuv_error=0.0625, pitch_frames=16,
               voiced_frames_orig=9, voiced_frames_inferred=8)
  intel = dict(stoi=0.875, estoi=0.75, stoi_frames=155, stoi_frames_kept=77)
  like = dict(nll=-4.5, bits_per_sample=-5.25, z_variance=0.75, likelihood_frames=31)
  assert list(get_df(ValidationEntries([entry(**pitch)])).columns) == TODAY[:-1] + PITCH + TODAY[-1:]
  assert list(get_df(ValidationEntries([entry(**intel)])).columns) == TODAY[:-1] + STOI + TODAY[-1:]
  df = get_df(ValidationEntries([entry(**like)]))
  assert list(df.columns) == TODAY[:-1] + LIKELIHOOD + TODAY[-1:] and len(df.columns) == 26
  assert [df.iloc[0][c] for c in LIKELIHOOD] == [-4.5, -5.25, 0.75, 31]
  df = get_df(ValidationEntries([entry(**pitch, **intel, **like)]))
  assert list(df.columns) == TODAY[:-1] + PITCH + STOI + LIKELIHOOD + TODAY[-1:] and len(df.columns) == 37
  assert [df.iloc[0][c] for c in LIKELIHOOD] == [-4.5, -5.25, 0.75, 31] and df.iloc[0]["Wav path"] == "/d/u0.wav"


def test_entry_points_validate_arguments_without_a_gpu():
  """The argument checks of wg_nll and wg_forward run before any device work: -1 with a message."""
  from waveglow_amd import _lib, build
  build.build_library()
  lib = _lib.load()
  cfg = _lib.WgConfig(80, 12, 8, 4, 2, 8, 256, 3, 1024, 256)
  h = C.c_void_p()
  assert lib.wg_create(C.byref(cfg), 0, C.byref(h)) == 0
  # three fp64 partials per (utterance, frame)
  assert lib.wg_nll_workspace_bytes(h, 16, 32 * 864) >= 16 * 864 * 3 * 8
  assert lib.wg_nll_workspace_bytes(h, 1, 1) > 0
  for B, L in ((0, 64), (-1, 64), (65536, 64), (1, 0), (1, -32), (1, (1 << 26) + 1)):
    assert lib.wg_nll_workspace_bytes(h, B, L) == 0, (B, L)
  assert lib.wg_nll_workspace_bytes(None, 1, 64) == 0
  dummy = (C.c_char * 256)()
  p = (C.addressof(dummy) + 15) & ~15
  ls = (C.c_void_p * 12)(*[p] * 12)
  big = 1 << 40
  nll = lambda *a: lib.wg_nll(*a)     # noqa: E731
  assert nll(None, p, ls, None, 1.0, 1, 64, p, None, p, big, None) == -1 and b"null" in lib.wg_last_error()
  for z, lsp, rows, ws in ((None, ls, p, p), (p, None, p, p), (p, ls, None, p), (p, ls, p, None)):
    assert nll(h, z, lsp, None, 1.0, 1, 64, rows, None, ws, big, None) == -1 and b"null" in lib.wg_last_error()
  for sigma in (0.0, -1.0, float("nan"), float("inf")):
    assert nll(h, p, ls, None, sigma, 1, 64, p, None, p, big, None) == -1 and b"sigma" in lib.wg_last_error()
  for B, L in ((0, 64), (65536, 64), (1, 0), (1, (1 << 26) + 1)):
    assert nll(h, p, ls, None, 1.0, B, L, p, None, p, big, None) == -1 and b"nll" in lib.wg_last_error()
  assert nll(h, p, ls, p, 1.0, 1, 65, p, None, p, big, None) == -1 and b"32 columns" in lib.wg_last_error()
  assert nll(h, p, ls, None, 1.0, 1, 64, p, None, p, big, None) == -2        # nothing was finalised: refused, not run
  # wg_forward with frame counts: null arguments, then the geometry the counts fix, then the call order
  # (h, mel, frames, audio, z, log_s, log_det_W, B, n_frames, audio_len, io_dtype, workspace, workspace_bytes, stream)
  fwd = lambda *a: lib.wg_forward(*a)     # noqa: E731
  ld = (C.c_float * 12)()
  assert fwd(None, p, p, p, p, ls, None, 1, 8, 2048, 0, p, big, None) == -1 and b"null" in lib.wg_last_error()
  for mel, audio, z, lsp, ws in ((None, p, p, ls, p), (p, None, p, ls, p), (p, p, None, ls, p), (p, p, p, None, p),
                                 (p, p, p, ls, None)):
    assert fwd(h, mel, p, audio, z, lsp, None, 1, 8, 2048, 0, ws, big, None) == -1 and b"null" in lib.wg_last_error()
  assert fwd(h, p, p, p, p, ls, None, 1, 0, 0, 0, p, big, None) == -1
  for audio_len in (2040, 2056, 8):                      # with counts the batch is whole frames: 256 * n_frames samples
    assert fwd(h, p, p, p, p, ls, None, 1, 8, audio_len, 0, p, big, None) == -1 and b"256 * n_frames" in lib.wg_last_error()
  assert fwd(h, p, p, p, p, ls, None, 1, (1 << 23) + 1, 0, 0, p, big, None) == -1          # n_frames above INT32_MAX >> 8
  # log_det_W: required without counts, optional with them (a null one passes the null checks and reaches the call order)
  assert fwd(h, p, None, p, p, ls, None, 1, 8, 2048, 0, p, big, None) == -1 and b"null" in lib.wg_last_error()
  assert fwd(h, p, None, p, p, ls, ld, 1, 8, 2048, 0, p, big, None) == -2
  assert fwd(h, p, p, p, p, ls, None, 1, 8, 2048, 0, p, big, None) == -2
  assert fwd(h, p, p, p, p, ls, ld, 1, 8, 2048, 0, p, big, None) == -2
  assert lib.wg_destroy(h) == 0


def test_python_layer_refuses_bad_arguments_before_any_launch():
  import torch
  import waveglow_amd
  from waveglow_amd import HParams, WaveGlow, _lib, likelihood
  assert waveglow_amd.log_likelihood is likelihood.log_likelihood and waveglow_amd.Likelihood is likelihood.Likelihood
  assert waveglow_amd.log_likelihood_enqueue is likelihood.log_likelihood_enqueue
  assert likelihood.Likelihood._fields == ("nll", "bits_per_sample", "samples", "z_mean", "z_var", "sum_z2", "sum_log_s",
                                           "log_det")
  model = WaveGlow(HParams(n_channels=64, n_layers=2, n_flows=2, n_early_every=2))
  T = 6
  mel, audio = torch.zeros((2, 80, T)), torch.zeros((2, 256 * T))
  for call in (lambda: model.log_likelihood(mel, audio),                                     # CPU tensors
               lambda: model.log_likelihood(mel, audio, frames=[T, 2]),
               lambda: model.log_likelihood_enqueue(mel, audio, frames=[T, 2]),
               lambda: model.forward_ragged(mel, audio, [T, 2]),
               lambda: likelihood.log_likelihood(model, mel.numpy(), audio),
               lambda: model.log_likelihood(mel, audio, sigma=0.0),                        # sigma, before the tensors
               lambda: model.log_likelihood(mel, audio, sigma=-1.0),
               lambda: model.log_likelihood_enqueue(mel, audio, sigma=float("nan"))):
    with pytest.raises(_lib.WgError):
      call()
  # the frame counts of a host list / CPU tensor: each in [1, T] and 256 * f within the audio
  for frames in ([0, 2], [T + 1, 2], [T, -1], [T], [T, 2, 1], torch.tensor([T + 1, 1]), torch.tensor([1.0, 2.0])):
    with pytest.raises(_lib.WgError):
      likelihood._frames(frames, mel, audio)
  short = torch.zeros((2, 256 * T - 1))
  with pytest.raises(_lib.WgError, match="256"):
    likelihood._frames([T, 2], mel, short)                                                  # longer than the audio
  assert likelihood._frames((T - 1, 2), mel, short).tolist() == [T - 1, 2]
  assert likelihood._frames(torch.tensor([1, T]), mel, audio).dtype == torch.int32
  for bad_mel, bad_audio in ((mel.double(), audio.double()), (mel[0], audio), (mel, audio[:1]), (mel, audio.half()),
                             (mel.to(torch.int32), audio)):
    with pytest.raises(_lib.WgError):
      likelihood._inputs(model, bad_mel, bad_audio)
