"""``Synthesizer`` facade with the reference's surface (src/waveglow/synthesizer.py:20-94)."""
from __future__ import annotations

import datetime
import os
import random
import time
from dataclasses import dataclass
from logging import getLogger
from typing import Dict, Optional

import numpy as np
import torch

from . import pcm
from .audio import is_overamp
from .checkpoint import CheckpointWaveglow
from .denoiser import Denoiser
from .hparams import overwrite_custom_hparams
from .model import WaveGlow


def get_default_device() -> torch.device:
  """src/waveglow/utils.py:112-118."""
  n = torch.cuda.device_count()
  if n == 1:
    return torch.device("cuda")
  if n > 1:
    return torch.device("cuda:0")
  return torch.device("cpu")


def init_global_seeds(seed: int) -> None:
  """src/waveglow/utils.py:221-229 -- called on EVERY Synthesizer.infer."""
  os.environ["PYTHONHASHSEED"] = str(seed)
  random.seed(seed)
  np.random.seed(seed)
  torch.random.manual_seed(seed)
  torch.manual_seed(seed)
  if torch.cuda.is_available():
    torch.cuda.manual_seed(seed)


@dataclass
class InferenceResult:
  wav: np.ndarray
  wav_denoised: np.ndarray
  sampling_rate: int
  inference_duration_s: float
  denoising_duration_s: float
  was_overamplified: bool
  timepoint: datetime.datetime


@dataclass
class PcmResult:
  """One utterance of ``Synthesizer.infer_batch_pcm``: the samples that go into the wav file."""
  pcm: np.ndarray               # int16, 256 * T samples: convert_wav(normalize_wav(denoised audio), int16)
  sampling_rate: int
  was_overamplified: bool       # of the raw audio, as InferenceResult.was_overamplified
  peak: float                   # max |x| of the denoised audio, the value the normalisation divided by
  inference_duration_s: float
  denoising_duration_s: float
  timepoint: datetime.datetime


def load_model(hparams, state_dict: Optional[dict], device: torch.device) -> WaveGlow:
  """src/waveglow/train.py:48-55 (without the silent CPU fallback of try_copy_to: the kernels need the GPU)."""
  model = WaveGlow(hparams).to(device)
  if state_dict is not None:
    model.load_state_dict(state_dict)
  return model


class Synthesizer:
  def __init__(self, checkpoint: CheckpointWaveglow, *, custom_hparams: Optional[Dict[str, str]] = None,
               device: Optional[torch.device] = None):
    device = torch.device(device) if device is not None else get_default_device()
    if device.type == "cuda" and device.index is None:
      device = torch.device("cuda", torch.cuda.current_device())
    hparams = overwrite_custom_hparams(checkpoint.get_hparams(), custom_hparams)
    model = load_model(hparams, checkpoint.state_dict, device)
    model = WaveGlow.remove_weightnorm(model).eval()
    self.device, self.hparams, self.model = device, hparams, model
    self.denoiser = Denoiser(waveglow=model, hparams=hparams, mode="zeros", device=device).to(device)
    self._pinned = None          # host staging buffer of infer_batch_pcm, grown on demand

  def infer(self, mel: torch.Tensor, *, sigma: float = 1.0, denoiser_strength: float = 0.0005,
            seed: int = 0) -> InferenceResult:
    timepoint = datetime.datetime.now()
    init_global_seeds(seed)
    denoising_duration = 0
    mel = mel.to(self.device)
    start = time.perf_counter()
    with torch.no_grad():
      audio = self.model.infer(mel, sigma=sigma)
      torch.cuda.synchronize(self.device)      # the reference's timer has no device sync (synthesizer.py:61)
      end = time.perf_counter()
      audio_denoised = audio
      if denoiser_strength > 0:
        t0 = time.perf_counter()
        audio_denoised = self.denoiser(audio, strength=denoiser_strength)
        torch.cuda.synchronize(self.device)
        denoising_duration = time.perf_counter() - t0
    audio_np = audio.squeeze().float().cpu().numpy()
    audio_denoised_np = audio_denoised.squeeze().float().cpu().numpy()
    over = bool(is_overamp(audio_np))
    if over:
      getLogger(__name__).debug("Waveglow output was overamplified.")
    return InferenceResult(wav=audio_np, wav_denoised=audio_denoised_np, sampling_rate=self.hparams.sampling_rate,
                           inference_duration_s=end - start, denoising_duration_s=denoising_duration,
                           was_overamplified=over, timepoint=timepoint)

  def _infer_batch_device(self, mels, sigma, denoiser_strength, seed):
    """The device work of a ragged batch, enqueued without a synchronise: noise drawn per utterance exactly as ``infer``
    draws it (seed reset, then the three tensors in the reference's order and shapes, model.py:234-271), one
    ragged ``wg_infer`` sequence and, for a strength above 0, one ragged denoiser call.  Returns the raw fp32 audio
    [B, 256 Tmax], the denoised audio (the raw tensor itself at strength 0), the frame counts, the sample counts as an
    int32 tensor on the device and three events: before the flow, behind it, behind the denoiser."""
    mels = [m.squeeze(0) if m.dim() == 3 else m for m in mels]
    B = len(mels)
    lens = [int(m.shape[1]) for m in mels]
    Tm = max(lens)
    model, dev = self.model, self.device
    n_mel, ng = mels[0].shape[0], model.n_group
    dtype = mels[0].dtype
    mel = torch.zeros((B, n_mel, Tm), dtype=dtype, device=dev)
    z_init = torch.zeros((B, model.n_remaining_channels, Tm * 256 // ng), dtype=dtype, device=dev)
    early = [k for k in reversed(range(model.n_flows)) if k % model.n_early_every == 0 and k > 0]
    z_early = [torch.zeros((B, model.n_early_size, Tm * 256 // ng), dtype=dtype, device=dev) for _ in early]
    samples_dev = torch.tensor([256 * t for t in lens], dtype=torch.int32).to(dev)
    for b, m in enumerate(mels):
      L = lens[b] * 256 // ng
      mel[b, :, :lens[b]] = m.to(dev)
      init_global_seeds(seed)                                                        # synthesizer.py:56
      z_init[b, :, :L] = torch.empty((1, model.n_remaining_channels, L), dtype=dtype, device=dev).normal_()[0]
      for j in range(len(early)):
        z_early[j][b, :, :L] = torch.empty((1, model.n_early_size, L), dtype=dtype, device=dev).normal_()[0]
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(3)]
    stream = torch.cuda.current_stream(dev)
    with torch.no_grad():
      ev[0].record(stream)
      audio = model.infer_with_noise(mel, z_init, z_early, sigma, frames=torch.tensor(lens, dtype=torch.int32)).float().contiguous()
      ev[1].record(stream)
      den = audio
      if denoiser_strength > 0:
        den = torch.empty_like(audio)
        self.denoiser.run_ragged(audio, [256 * t for t in lens], samples_dev, denoiser_strength, den)
      ev[2].record(stream)
    return audio, den, lens, samples_dev, ev

  def infer_batch(self, mels, *, sigma: float = 1.0, denoiser_strength: float = 0.0005, seed: int = 0):
    """Several mel-spectrograms ``[1 or -, n_mel, T_i]`` of different lengths in ONE ragged launch sequence (the
    reference's commented-out ``--batch-size``, inference_v2.py:64).  Every utterance gets the audio that ``infer`` on
    it alone would return with the same seed: its noise is drawn exactly as that call draws it, and the kernels treat the
    padding behind an utterance as the end of the sequence (``wg_infer``, ``wg_stft_denoise`` with counts).  Returns
    one InferenceResult per utterance; the durations are the batch's on the device, divided evenly."""
    timepoint = datetime.datetime.now()
    audio, den, lens, _, ev = self._infer_batch_device(mels, sigma, denoiser_strength, seed)
    B = len(lens)
    audio_np = audio.cpu().numpy()
    den_np = den.cpu().numpy() if den is not audio else audio_np
    inf_s = ev[0].elapsed_time(ev[1]) / 1e3
    den_s = ev[1].elapsed_time(ev[2]) / 1e3 if denoiser_strength > 0 else 0
    res = []
    for b in range(B):
      a_np, d_np = audio_np[b, :256 * lens[b]].copy(), den_np[b, :256 * lens[b]].copy()
      res.append(InferenceResult(wav=a_np, wav_denoised=d_np, sampling_rate=self.hparams.sampling_rate,
                                 inference_duration_s=inf_s / B, denoising_duration_s=den_s / B,
                                 was_overamplified=bool(is_overamp(a_np)), timepoint=timepoint))
    return res

  def infer_batch_pcm(self, mels, *, sigma: float = 1.0, denoiser_strength: float = 0.0005, seed: int = 0,
                      output_sampling_rate: Optional[int] = None):
    """``infer_batch`` finished to int16 on the device (``wg_wav_finish``): behind the noise draws the batch is one
    launch sequence, and ONE copy (the int16 samples and the statistics, through a pinned buffer) and one synchronise
    bring it to the host.  Returns one PcmResult per utterance; ``pcm`` equals
    ``convert_wav(normalize_wav(r.wav_denoised), np.int16)`` of the corresponding ``infer_batch`` result bit for bit.
    An utterance with NaN or infinite samples raises WgError.

    ``output_sampling_rate`` (not in the reference): the denoised audio is resampled to that rate on the device
    (waveglow_amd/resample.py, not clipped) between the denoiser and ``wg_wav_finish``, so the peak normalisation and the
    int16 conversion run on the resampled signal: ``pcm`` has ``out_len(256 T)`` samples and equals
    ``convert_wav(normalize_wav(x), np.int16)`` of ``x = resample(wav_denoised)``, ``sampling_rate`` is the output rate and
    ``peak`` the resampled signal's; ``was_overamplified`` stays the statement about the raw audio at the model's rate.
    Still one host copy and one synchronise.  Without it nothing changes and nothing more is launched."""
    if output_sampling_rate is not None:
      return self._infer_batch_pcm_resampled(mels, sigma, denoiser_strength, seed, output_sampling_rate)
    timepoint = datetime.datetime.now()
    audio, den, lens, samples_dev, ev = self._infer_batch_device(mels, sigma, denoiser_strength, seed)
    B, N = audio.shape
    out = pcm.finish_enqueue(audio, den, samples_dev)
    if self._pinned is None or self._pinned.numel() < out.numel():
      self._pinned = torch.empty(out.numel(), dtype=torch.uint8, pin_memory=True)
    host = self._pinned[:out.numel()]
    host.copy_(out, non_blocking=True)
    torch.cuda.current_stream(self.device).synchronize()
    samples, stats = pcm.finish_read(host, B, N)
    inf_s = ev[0].elapsed_time(ev[1]) / 1e3
    den_s = ev[1].elapsed_time(ev[2]) / 1e3 if denoiser_strength > 0 else 0
    return [PcmResult(pcm=samples[b, :256 * lens[b]].copy(), sampling_rate=self.hparams.sampling_rate,
                      was_overamplified=bool(stats[b, pcm.RAW_MIN] < -1.0 or stats[b, pcm.RAW_MAX] > 1.0),
                      peak=float(stats[b, pcm.DEN_PEAK]), inference_duration_s=inf_s / B,
                      denoising_duration_s=den_s / B, timepoint=timepoint) for b in range(B)]

  def _infer_batch_pcm_resampled(self, mels, sigma, denoiser_strength, seed, rate):
    """``infer_batch_pcm`` with an output rate.  ``wg_wav_finish`` runs on the resampled denoised audio (samples, peak);
    the raw audio at the model's rate only gives its extrema under the length mask, for ``was_overamplified``, and they
    ride behind the finished buffer in the one copy: [int16 samples | statistics of the resampled | raw min, max, flag]."""
    from . import _lib
    from .resample import out_len, resample_enqueue, resample_plan
    timepoint = datetime.datetime.now()
    up, down, _, _ = resample_plan(self.hparams.sampling_rate, rate)        # refuses the rate before any device work
    audio, den, lens, samples_dev, ev = self._infer_batch_device(mels, sigma, denoiser_strength, seed)
    B, N = audio.shape
    lens_r = [out_len(256 * t, up, down) for t in lens]
    Nr = (out_len(N, up, down) + 7) // 8 * 8                                 # wg_wav_finish: rows of a multiple of 8
    res = resample_enqueue(den, samples_dev, self.hparams.sampling_rate, rate, pitch=Nr)
    lens_r_dev = torch.tensor(lens_r, dtype=torch.int32).to(self.device)
    fin = pcm.finish_enqueue(res, res, lens_r_dev)
    inside = torch.arange(N, device=self.device)[None, :] < samples_dev[:, None]
    raw = torch.stack([torch.where(inside, audio, float("inf")).amin(dim=1),
                       torch.where(inside, audio, float("-inf")).amax(dim=1),
                       (inside & ~torch.isfinite(audio)).any(dim=1).float()], dim=1)        # fp32 [B, 3]
    out = torch.cat([fin, raw.contiguous().view(torch.uint8).view(-1)])
    if self._pinned is None or self._pinned.numel() < out.numel():
      self._pinned = torch.empty(out.numel(), dtype=torch.uint8, pin_memory=True)
    host = self._pinned[:out.numel()]
    host.copy_(out, non_blocking=True)
    torch.cuda.current_stream(self.device).synchronize()
    samples, stats = pcm.finish_read(host[:fin.numel()], B, Nr)
    raw = host[fin.numel():].numpy().view(np.float32).reshape(B, 3)
    bad = np.nonzero(raw[:, 2])[0]
    if bad.size:
      raise _lib.WgError(f"utterance {int(bad[0])} of the batch has NaN or infinite samples: it cannot be written as PCM")
    inf_s = ev[0].elapsed_time(ev[1]) / 1e3
    den_s = ev[1].elapsed_time(ev[2]) / 1e3 if denoiser_strength > 0 else 0
    return [PcmResult(pcm=samples[b, :lens_r[b]].copy(), sampling_rate=int(rate),
                      was_overamplified=bool(raw[b, 0] < -1.0 or raw[b, 1] > 1.0),
                      peak=float(stats[b, pcm.DEN_PEAK]), inference_duration_s=inf_s / B,
                      denoising_duration_s=den_s / B, timepoint=timepoint) for b in range(B)]

  # ------------------------------------------------------------------ streaming (waveglow_amd/streaming.py)
  def open_stream(self, *, sigma: float = 1.0, denoiser_strength: float = 0.0005, seed: int = 0, chunk_frames: int = 32,
                  total_frames: Optional[int] = None, gain: float = 1.0, dtype: Optional[torch.dtype] = None):
    """A ``StreamSession``: push mel frames as they arrive, take audio in chunks of ``chunk_frames`` frames through
    ``stream_step``.  The chunks, concatenated, have the bits of whole-utterance synthesis -- with ``total_frames`` given
    those of ``infer(mel, seed=seed)`` (the noise is drawn here, once, as that call draws it, which resets the global
    generators as that call does), open-ended those of ``model.infer_with_noise(mel, *session.noise())`` (a generator of
    the session's own, drawn from at every push).  A chunk leaves once ``Hr`` frames behind it have arrived
    (``streaming.halo_frames``: 99 for the default model with the denoiser on) or the stream is closed.  ``dtype``: the
    mel's (float32 or float16), by default the model's parameter dtype.  WgError before any device work for
    ``chunk_frames < 1`` and for a known length below 4 frames with the denoiser on (the whole-utterance path's limit)."""
    from .streaming import StreamSession
    if dtype is None:
      dtype = next(self.model.parameters()).dtype
    return StreamSession(self, sigma=sigma, denoiser_strength=denoiser_strength, seed=seed, chunk_frames=chunk_frames,
                         total_frames=total_frames, gain=gain, dtype=dtype)

  def stream_step(self, sessions, pcm: bool = True) -> list:
    """Advance every session that has a chunk ready by ONE chunk, all of them in one launch sequence (one table upload,
    one ``wg_stream_gather``, one ragged flow, one ragged denoiser call, one ``wg_stream_emit``, one pinned copy and one
    synchronise).  Returns one entry per session: None where nothing was ready (that session is not touched), else a
    ``StreamChunk``.  ``pcm=True``: int16 samples on the host, ``convert_wav(np.clip(denoised * gain, -1, 1), np.int16)``
    -- NOT peak-normalised: the utterance's peak is not known while it streams -- with the raw audio's extrema and the
    number of clipped samples; a chunk with NaN or infinite samples raises WgError naming the session, and no session
    advances.  ``pcm=False``: fp32 device tensors ``raw`` and ``denoised``; nothing is copied or synchronised.  The
    sessions of a step share dtype, sigma and -- those with the denoiser on -- its strength (WgError otherwise)."""
    from .streaming import stream_step
    return stream_step(self, list(sessions), pcm)

  def infer_stream(self, mel: torch.Tensor, *, chunk_frames: int = 32, pcm: bool = True, **kw):
    """Generator over one finished mel ``[1 or -, n_mel, T]``: ``open_stream(total_frames=T)``, ``push``, ``close``, then
    one ``StreamChunk`` per step until the final one.  The audio is that of ``infer(mel, ...)`` with the same keywords."""
    m = mel[0] if mel.dim() == 3 else mel
    s = self.open_stream(chunk_frames=chunk_frames, total_frames=int(m.shape[-1]), dtype=m.dtype, **kw)
    s.push(m)
    s.close()
    while True:
      chunk = self.stream_step([s], pcm=pcm)[0]
      yield chunk
      if chunk.final:
        return
