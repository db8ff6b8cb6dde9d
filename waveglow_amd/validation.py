"""``validate`` with the reference's surface (src/waveglow/validation.py:23-108, :125-287): copy synthesis of validation
utterances from their own mels, and per utterance the mel-cepstral distortion with and without DTW alignment, the
alignment penalties and the cosine similarity between the original mel and the mel of the synthesised audio.

Behind the noise draws a batch of utterances is one launch sequence on the device: the flow and the denoiser
(``Synthesizer._infer_batch_device``), the int16 finishing (``wg_wav_finish``), the normalisation, the mel of the result
(``TacotronSTFT.mel_spectrogram_ragged_device``), the metrics (``wg_metrics_mel``) and, with ``pitch_metrics``, the F0 and
voicing errors between the original wavs, kept on the device, and that audio (``wg_pitch_metrics``), and with
``intelligibility_metrics`` STOI and ESTOI of the same two, both resampled to 10 kHz (``wg_resample``, ``wg_stoi``).  Not built: the PNG
plots and the structural similarity computed from them (``structural_similarity`` stays None).
"""
from __future__ import annotations

import datetime
import random
from dataclasses import dataclass
from logging import getLogger
from typing import Callable, Dict, List, Optional, Set

import numpy as np
import torch

from . import _lib, metrics, pcm
from . import likelihood as ll
from .audio import wav_to_float32
from .checkpoint import CheckpointWaveglow
from .synthesizer import PcmResult, Synthesizer
from .taco_stft import TacotronSTFT
from .training import Entry

MCD_NO_OF_COEFFS_PER_FRAME = 16          # src/waveglow/globals.py


@dataclass
class ValidationEntry:
  entry: Entry = None
  inference_result: PcmResult = None     # the durations, sampling rate and over-amplification flag of the reference's field
  seed: int = None
  diff_duration_s: float = None
  iteration: int = None
  inferred_duration_s: float = None
  timepoint: datetime.datetime = None
  diff_frames: int = None
  mfcc_no_coeffs: int = None
  mfcc_dtw_mcd: float = None
  mfcc_dtw_penalty: float = None
  mfcc_dtw_frames: int = None
  mcd: float = None
  mcd_penalty: float = None
  mcd_frames: int = None
  structural_similarity: float = None
  cosine_similarity: float = None
  denoiser_strength: float = None
  sigma: float = None
  # validate(pitch_metrics=True) only (waveglow_amd/metrics.py: PitchMetrics); None otherwise
  f0_rmse_cents: float = None
  f0_rmse_hz: float = None
  gross_pitch_error: float = None
  vuv_error: float = None
  pitch_frames: int = None
  voiced_frames_orig: int = None
  voiced_frames_inferred: int = None
  # validate(intelligibility_metrics=True) only (waveglow_amd/metrics.py: IntelligibilityMetrics); None otherwise
  stoi: float = None
  estoi: float = None
  stoi_frames: int = None
  stoi_frames_kept: int = None
  # validate(likelihood=True) only (waveglow_amd/likelihood.py: Likelihood of the ORIGINAL wav under the checkpoint); None otherwise
  nll: float = None
  bits_per_sample: float = None
  z_variance: float = None
  likelihood_frames: int = None


class ValidationEntries(List[ValidationEntry]):
  pass


@dataclass
class ValidationEntryOutput:
  mel_orig: np.ndarray = None
  orig_sr: int = None
  wav_orig: np.ndarray = None
  inferred_sr: int = None
  mel_inferred_denoised: np.ndarray = None
  wav_inferred_denoised: np.ndarray = None     # int16: convert_wav(normalize_wav(denoised audio), int16)
  wav_inferred: np.ndarray = None              # int16: convert_wav(normalize_wav(raw audio), int16)


def get_df(entries: ValidationEntries):
  """The reference's table (validation.py:52-108) without the "Structual Similarity (Padded)" column.  Entries validated
  with the pitch metrics get seven more columns behind "Cosine Similarity (Padded)", entries validated with the
  intelligibility metrics four more behind those, entries validated with the likelihood four more behind those."""
  from pandas import DataFrame
  if len(entries) == 0:
    return DataFrame()
  with_pitch = any(e.pitch_frames is not None for e in entries)
  with_stoi = any(e.stoi_frames is not None for e in entries)
  with_ll = any(e.likelihood_frames is not None for e in entries)
  data = [{
    "Name": e.entry.basename,
    "Subpath": e.entry.stem,
    "Timepoint": f"{e.timepoint:%Y/%m/%d %H:%M:%S}",
    "Iteration": e.iteration,
    "Seed": e.seed,
    "Sigma": e.sigma,
    "Denoiser strength": e.denoiser_strength,
    "Inference duration (s)": e.inference_result.inference_duration_s,
    "Denoising duration (s)": e.inference_result.denoising_duration_s,
    "Overamplified?": e.inference_result.was_overamplified,
    "Inferred wav duration (s)": e.inferred_duration_s,
    "# Difference frames": e.diff_frames,
    "Sampling rate (Hz)": e.inference_result.sampling_rate,
    "# MFCC Coefficients": e.mfcc_no_coeffs,
    "MFCC DTW MCD": e.mfcc_dtw_mcd,
    "MFCC DTW PEN": e.mfcc_dtw_penalty,
    "# MFCC DTW frames": e.mfcc_dtw_frames,
    "MCD": e.mcd,
    "PEN": e.mcd_penalty,
    "# Frames": e.mcd_frames,
    "Cosine Similarity (Padded)": e.cosine_similarity,
    **({
      "F0 RMSE (cents)": e.f0_rmse_cents,
      "F0 RMSE (Hz)": e.f0_rmse_hz,
      "Gross pitch error": e.gross_pitch_error,
      "V/UV error": e.vuv_error,
      "# Pitch frames": e.pitch_frames,
      "# Voiced frames original": e.voiced_frames_orig,
      "# Voiced frames inferred": e.voiced_frames_inferred,
    } if with_pitch else {}),
    **({
      "STOI": e.stoi,
      "ESTOI": e.estoi,
      "# STOI frames": e.stoi_frames,
      "# STOI frames kept": e.stoi_frames_kept,
    } if with_stoi else {}),
    **({
      "NLL (nats/sample)": e.nll,
      "Bits per sample": e.bits_per_sample,
      "z variance": e.z_variance,
      "# Likelihood frames": e.likelihood_frames,
    } if with_ll else {}),
    "Wav path": str(e.entry.wav_absolute_path),
  } for e in entries]
  return DataFrame(data=[list(x.values()) for x in data], columns=list(data[0].keys()))


def select_entries(data: List[Entry], entry_names: Set[str], full_run: bool, seed: int) -> List[Entry]:
  """validation.py:133-144: everything, the named entries (all of them must exist), or one random entry."""
  if full_run:
    return list(data)
  if len(entry_names) == 0:
    assert len(data) > 0
    random.seed(seed)
    return [random.choice(data)]
  entries = [x for x in data if x.basename in entry_names]
  if len(entries) != len(entry_names):
    getLogger(__name__).error("Not all entry name's were found!")
    raise AssertionError("Not all entry name's were found!")
  return entries


def _validate_batch(synth: Synthesizer, taco: TacotronSTFT, chunk: List[Entry], sigma, denoiser_strength, seed, iteration,
                    save_callback, out: ValidationEntries, pitch_metrics: bool = False,
                    intelligibility_metrics: bool = False, likelihood: bool = False) -> None:
  logger = getLogger(__name__)
  dev = synth.device
  timepoint = datetime.datetime.now()
  B = len(chunk)
  if pitch_metrics or intelligibility_metrics or likelihood:              # the wavs stay on the device: read once
    mel_orig, frames, wav_orig_dev, n_orig_dev = taco.get_mel_and_wav_tensors_from_files(
      [e.wav_absolute_path for e in chunk])
  else:
    mel_orig, frames = taco.get_mel_tensors_from_files([e.wav_absolute_path for e in chunk])
  if max(frames) + 1 > metrics.MAX_FRAMES:
    raise _lib.WgError(f"validate: an utterance of {max(frames)} frames is too long for the metrics "
                       f"(at most {metrics.MAX_FRAMES - 1})")
  audio, den, frames, samples_dev, ev = synth._infer_batch_device([mel_orig[b, :, :frames[b]] for b in range(B)], sigma,
                                                                 denoiser_strength, seed)
  N = audio.shape[1]
  fin = pcm.finish_enqueue(audio, den, samples_dev)                       # inferred_denoised.wav, as infer_batch_pcm
  fin_raw = pcm.finish_enqueue(audio, audio, samples_dev) if den is not audio else fin      # inferred.wav
  # normalize_wav (audio_utils.py:67-95) of the denoised audio on the device: x / peak unless the peak is 1 or 0
  peak = fin[2 * B * N:].view(torch.float32).view(B, pcm.N_STATS)[:, pcm.DEN_PEAK:pcm.DEN_PEAK + 1]
  normed = torch.where((peak != 1.0) & (peak != 0.0), den / peak, den)
  samples = [256 * t for t in frames]
  mel_inf, frames_inf, frames_inf_dev = taco.mel_spectrogram_ragged_device(normed, samples)
  frames_dev = torch.tensor(frames, dtype=torch.int32).to(dev)
  rows = metrics.mel_metrics_enqueue(mel_orig, frames_dev, mel_inf, frames_inf_dev, MCD_NO_OF_COEFFS_PER_FRAME)
  # one copy for the rows, with the peak of the normalised audio beside them (what normalize_wav asserts of its result)
  inside = torch.arange(N, device=dev)[None, :] < samples_dev[:, None]
  parts = [rows, torch.where(inside, normed.abs(), 0.0).amax(dim=1, keepdim=True).double()]
  if pitch_metrics:
    # d' is a ratio: the tracks do not depend on the level of either side (bit for bit under a power of two, to rounding
    # otherwise), so the original as loaded is compared with the peak-normalised synthesis
    parts.append(metrics.pitch_metrics_enqueue(wav_orig_dev, n_orig_dev, normed, samples_dev,
                                               sampling_rate=synth.hparams.sampling_rate))
  if intelligibility_metrics:
    # the clean side is the original as loaded, the processed side the peak-normalised synthesis
    parts.append(metrics.intelligibility_metrics_enqueue(wav_orig_dev, n_orig_dev, normed, samples_dev,
                                                         sampling_rate=synth.hparams.sampling_rate))
  if likelihood:
    # the original recording under the checkpoint: no sampling, so no seed noise; whole frames only (n // 256)
    parts.append(ll.log_likelihood_enqueue(synth.model, mel_orig, wav_orig_dev, n_orig_dev // ll.FRAME_SAMPLES,
                                           sigma=synth.hparams.sigma))
  rows = torch.cat(parts, dim=1).cpu()
  first = metrics.N_ROW + 1
  pitch = metrics.rows_to_pitch_metrics(rows[:, first:first + metrics.N_ROW]) if pitch_metrics else None
  first += metrics.N_ROW if pitch_metrics else 0
  intel = metrics.rows_to_intelligibility_metrics(rows[:, first:first + metrics.N_ROW]) if intelligibility_metrics else None
  first += metrics.N_ROW if intelligibility_metrics else 0
  like = ll.rows_to_likelihoods(rows[:, first:first + ll.N_ROW]) if likelihood else None
  fin_h = fin.cpu()
  fin_raw_h = fin_raw.cpu() if fin_raw is not fin else fin_h
  mel_orig_h, mel_inf_h = mel_orig.cpu().numpy(), mel_inf.cpu().numpy()
  den_pcm, stats = pcm.finish_read(fin_h, B, N)
  raw_pcm, _ = pcm.finish_read(fin_raw_h, B, N)
  inf_s = ev[0].elapsed_time(ev[1]) / 1e3
  den_s = ev[1].elapsed_time(ev[2]) / 1e3 if denoiser_strength > 0 else 0
  sr = synth.hparams.sampling_rate
  for b, (entry, m) in enumerate(zip(chunk, metrics.rows_to_metrics(rows[:, :metrics.N_ROW]))):
    norm_peak = float(rows[b, metrics.N_ROW])
    assert norm_peak == 1.0 or norm_peak == 0.0                                    # audio_utils.py:92-93
    n = samples[b]
    res = PcmResult(pcm=den_pcm[b, :n].copy(), sampling_rate=sr,
                    was_overamplified=bool(stats[b, pcm.RAW_MIN] < -1.0 or stats[b, pcm.RAW_MAX] > 1.0),
                    peak=float(stats[b, pcm.DEN_PEAK]), inference_duration_s=inf_s / B, denoising_duration_s=den_s / B,
                    timepoint=timepoint)
    val = ValidationEntry(entry=entry, inference_result=res, seed=seed, iteration=iteration, timepoint=timepoint,
                          inferred_duration_s=n / sr, denoiser_strength=denoiser_strength, sigma=sigma,
                          mfcc_no_coeffs=MCD_NO_OF_COEFFS_PER_FRAME, diff_frames=frames_inf[b] - frames[b],
                          mfcc_dtw_mcd=m.mcd_dtw, mfcc_dtw_penalty=m.penalty_dtw, mfcc_dtw_frames=m.frames_dtw, mcd=m.mcd,
                          mcd_penalty=m.penalty, mcd_frames=m.frames, cosine_similarity=m.cosine)
    if pitch:
      pm = pitch[b]
      val.f0_rmse_cents, val.f0_rmse_hz, val.gross_pitch_error, val.vuv_error = \
          pm.f0_rmse_cents, pm.f0_rmse_hz, pm.gross_pitch_error, pm.vuv_error
      val.pitch_frames, val.voiced_frames_orig, val.voiced_frames_inferred = pm.frames, pm.voiced_a, pm.voiced_b
    if intel:
      im = intel[b]
      val.stoi, val.estoi, val.stoi_frames, val.stoi_frames_kept = im.stoi, im.estoi, im.frames, im.frames_kept
    if like:
      lk = like[b]
      val.nll, val.bits_per_sample, val.z_variance = lk.nll, lk.bits_per_sample, lk.z_var
      val.likelihood_frames = lk.samples // ll.FRAME_SAMPLES
    wav_orig, orig_sr = wav_to_float32(entry.wav_absolute_path)
    output = ValidationEntryOutput(mel_orig=mel_orig_h[b, :, :frames[b]].copy(), orig_sr=orig_sr, wav_orig=wav_orig,
                                   inferred_sr=sr, mel_inferred_denoised=mel_inf_h[b, :, :frames_inf[b]].copy(),
                                   wav_inferred_denoised=res.pcm, wav_inferred=raw_pcm[b, :n].copy())
    logger.info(f"Current: {entry.stem}")
    logger.info(f"MCD DTW: {val.mfcc_dtw_mcd}")
    logger.info(f"MCD DTW penalty: {val.mfcc_dtw_penalty}")
    logger.info(f"MCD DTW frames: {val.mfcc_dtw_frames}")
    logger.info(f"MCD: {val.mcd}")
    logger.info(f"MCD penalty: {val.mcd_penalty}")
    logger.info(f"MCD frames: {val.mcd_frames}")
    logger.info(f"Cosine Similarity: {val.cosine_similarity}")
    if pitch:
      logger.info(f"F0 RMSE (cents): {val.f0_rmse_cents}")
      logger.info(f"F0 RMSE (Hz): {val.f0_rmse_hz}")
      logger.info(f"Gross pitch error: {val.gross_pitch_error}")
      logger.info(f"V/UV error: {val.vuv_error}")
      logger.info(f"Pitch frames: {val.pitch_frames} (voiced: original {val.voiced_frames_orig}, "
                  f"inferred {val.voiced_frames_inferred})")
    if intel:
      logger.info(f"STOI: {val.stoi}")
      logger.info(f"ESTOI: {val.estoi}")
      logger.info(f"STOI frames: {val.stoi_frames} (kept: {val.stoi_frames_kept})")
    if like:
      logger.info(f"NLL (nats/sample): {val.nll}")
      logger.info(f"Bits per sample: {val.bits_per_sample}")
      logger.info(f"z variance: {val.z_variance}")
      logger.info(f"Likelihood frames: {val.likelihood_frames}")
    save_callback(entry, output)
    out.append(val)


def validate(checkpoint: CheckpointWaveglow, data: List[Entry], custom_hparams: Optional[Dict[str, str]],
             denoiser_strength: float, sigma: float, entry_names: Set[str], full_run: bool,
             save_callback: Callable[[Entry, ValidationEntryOutput], None], seed: Optional[int], device: torch.device, *,
             batch_size: int = 1, pitch_metrics: bool = False, resample_inputs: bool = False,
             intelligibility_metrics: bool = False, likelihood: bool = False) -> ValidationEntries:
  """validation.py:125-287.  ``batch_size`` utterances share one launch sequence; every utterance gets the audio, the
  mels and the metrics it gets alone (its noise is drawn as ``Synthesizer.infer`` draws it, and every kernel of the
  sequence treats the padding behind an utterance as the end of the sequence).  ``pitch_metrics`` adds the F0 and
  voicing errors between the original wav and the synthesis (``metrics.pitch_metrics_enqueue`` with its defaults at the
  model's sampling rate); without it nothing of them is launched and their fields stay None.  ``intelligibility_metrics``
  adds STOI and ESTOI of the same two signals in the same way (``metrics.intelligibility_metrics_enqueue``: both resampled
  to 10 kHz on the device; the original is the clean side).  ``resample_inputs``: wavs at
  other rates are resampled to the model's on the device (``TacotronSTFT(..., resample_inputs=True)``) and the metrics
  compare the resampled original with the synthesis; ``wav_orig`` / ``orig_sr`` of the output stay the file's own.
  ``likelihood`` adds what the checkpoint assigns to the ORIGINAL wav (after ``resample_inputs``, the resampled one) under
  its own mel: the negative log-likelihood in nats per sample at ``hparams.sigma`` -- comparable with the training log --,
  bits per sample and the variance of z, over the ``n // 256`` whole frames of the file
  (``WaveGlow.log_likelihood_enqueue``); without it nothing of it is launched and its fields stay None."""
  logger = getLogger(__name__)
  result = ValidationEntries()
  if seed is None:
    seed = random.randint(1, 9999)
    logger.info(f"As no seed was given, using random seed: {seed}.")
  entries = select_entries(data, set(entry_names), full_run, seed)
  if len(entries) == 0:
    logger.info("Nothing to synthesize!")
    return result
  synth = Synthesizer(checkpoint=checkpoint, custom_hparams=custom_hparams, device=device)
  taco = TacotronSTFT(synth.hparams, synth.device, resample_inputs=resample_inputs)
  bs = max(1, int(batch_size))
  for i in range(0, len(entries), bs):
    _validate_batch(synth, taco, entries[i:i + bs], sigma, denoiser_strength, seed, checkpoint.iteration, save_callback,
                    result, pitch_metrics, intelligibility_metrics, likelihood)
  return result
