"""Mel front-end with the reference's surface (src/waveglow/taco_stft.py:53-125), computed by the HIP library
(``wg_stft_mel``: conv-STFT magnitudes on exact-fp32 MFMA, mel projection + log compression).

``librosa.filters.mel`` (taco_stft.py:66-73) is restated below (Slaney scale, Slaney area normalisation -- librosa's
defaults ``htk=False, norm='slaney'``); librosa is absent here.  The front-end is pinned against
``oracle/stft_oracle.py`` (numpy fp64 restatement) and against outputs of the reference's own
``TacotronSTFT.mel_spectrogram`` (tests/golden/stft_ref.npz, tests/test_gpu_stft_ref.py) -- made with THIS filter bank in
place of ``librosa.filters.mel``, so everything is pinned except the filter bank's values.

``TacotronSTFT.mel_spectrogram_differentiable`` is the same front-end with an autograd graph back to the audio (the
reference detaches at taco_stft.py:99): ``wg_stft_mel_forward_saved`` keeps the spectrum, and ``wg_stft_mel_backward``
runs the mel / magnitude chain rule in one row kernel and the transposed conv-STFT as an fp32 MFMA GEMM.
"""
from __future__ import annotations

import ctypes as C
from dataclasses import dataclass

import numpy as np
import torch

from . import _args, _lib
from .audio import convert_wav, wav_to_float32
from .denoiser import stft_handle

FLOAT32_64_MIN_WAV, FLOAT32_64_MAX_WAV = -1.0, 1.0   # audio_utils.py


@dataclass
class STFTHParams:
  filter_length: int = 1024
  hop_length: int = 256
  win_length: int = 1024
  window: str = "hann"


@dataclass
class TSTFTHParams(STFTHParams):
  n_mel_channels: int = 80
  sampling_rate: int = 22050
  mel_fmin: float = 0.0
  mel_fmax: float = 8000.0


def read_wav_raw(path):
  """(samples as stored -- int16 stays int16 --, sampling rate) of a PCM wav file."""
  from scipy.io.wavfile import read
  sampling_rate, wav = read(path)
  return wav, sampling_rate


def _float32_tensor(wav: np.ndarray) -> torch.Tensor:
  """what ``get_wav_tensor_from_file`` hands out for samples as stored: ``convert_wav`` to float32, on the host"""
  return torch.from_numpy(np.ascontiguousarray(convert_wav(wav, np.float32), dtype=np.float32))


def _hz_to_mel(f):
  f = np.asarray(f, dtype=np.float64)
  f_sp = 200.0 / 3
  mels = f / f_sp
  min_log_hz, logstep = 1000.0, np.log(6.4) / 27.0
  min_log_mel = min_log_hz / f_sp
  return np.where(f >= min_log_hz, min_log_mel + np.log(np.maximum(f, 1e-30) / min_log_hz) / logstep, mels)


def _mel_to_hz(m):
  m = np.asarray(m, dtype=np.float64)
  f_sp = 200.0 / 3
  min_log_hz, logstep = 1000.0, np.log(6.4) / 27.0
  min_log_mel = min_log_hz / f_sp
  return np.where(m >= min_log_mel, min_log_hz * np.exp(logstep * (m - min_log_mel)), f_sp * m)


def slaney_mel_filterbank(sr: int, n_fft: int, n_mels: int, fmin: float, fmax: float) -> np.ndarray:
  """librosa.filters.mel(sr=, n_fft=, n_mels=, fmin=, fmax=) with its defaults: triangular filters on the Slaney mel
  scale, each scaled to unit area (2 / bandwidth).  [n_mels, 1 + n_fft/2] float32."""
  fftfreqs = np.linspace(0.0, sr / 2.0, 1 + n_fft // 2)
  mel_f = _mel_to_hz(np.linspace(_hz_to_mel(fmin), _hz_to_mel(fmax), n_mels + 2))
  fdiff = np.diff(mel_f)
  ramps = mel_f[:, None] - fftfreqs[None, :]
  lower = -ramps[:-2] / fdiff[:-1, None]
  upper = ramps[2:] / fdiff[1:, None]
  weights = np.maximum(0.0, np.minimum(lower, upper))
  weights *= (2.0 / (mel_f[2:n_mels + 2] - mel_f[:n_mels]))[:, None]
  return weights.astype(np.float32)


def dynamic_range_compression(x, C_=1, clip_val=1e-5):
  return torch.log(torch.clamp(x, min=clip_val) * C_)


def dynamic_range_decompression(x, C_=1):
  return torch.exp(x) / C_


class _MelFn(torch.autograd.Function):
  """Inputs: the TacotronSTFT module, the audio [B, N] and the device copy of the lengths (int32 [B]) or None.  The
  forward keeps the library's workspace (spectrum, magnitudes, pre-log sums) and the lengths on ctx; the backward writes
  its d (re, im) to a separate part of that workspace, so the saved state survives and a second backward under
  retain_graph gives the same gradient."""

  @staticmethod
  def forward(ctx, taco, y, lens):
    y = y.contiguous()
    B, N = y.shape
    h = taco._h
    ws = _args.workspace(taco.lib.wg_stft_mel_grad_workspace_bytes(h, B, N), y.device,
                         f"mel front-end: audio of {N} samples is too short (reflect padding needs > 512)")
    mel = torch.empty((B, taco.n_mel_channels, N // 256 + 1), dtype=torch.float32, device=y.device)
    _lib.check(taco.lib.wg_stft_mel_forward_saved(h, _args.ptr(taco.mel_basis), taco.n_mel_channels, _args.ptr(y),
                                                  _args.ptr(lens), _args.ptr(mel), B, N, _args.ptr(ws), ws.numel(),
                                                  _args.stream(y.device)))
    ctx.taco, ctx.ws, ctx.dims, ctx.lens = taco, ws, (B, N), lens
    return mel

  @staticmethod
  def backward(ctx, g_mel):
    taco, ws = ctx.taco, ctx.ws
    B, N = ctx.dims
    g = g_mel.to(torch.float32).contiguous()
    gy = torch.empty((B, N), dtype=torch.float32, device=ws.device)
    _lib.check(taco.lib.wg_stft_mel_backward(taco._h, _args.ptr(taco.mel_basis), taco.n_mel_channels, _args.ptr(g),
                                             _args.ptr(ctx.lens), _args.ptr(gy), B, N, _args.ptr(ws), ws.numel(),
                                             _args.stream(ws.device)))
    return None, gy, None


class TacotronSTFT(torch.nn.Module):
  def __init__(self, hparams, device, resample_inputs: bool = False):
    """``resample_inputs`` (not in the reference): a wav file whose rate differs from ``hparams.sampling_rate`` is
    resampled to it on the device (waveglow_amd/resample.py, clipped to [-1, 1]) instead of being refused."""
    super().__init__()
    device = torch.device(device)
    if device.type != "cuda":
      raise _lib.WgError("the mel front-end runs on the GPU library only")
    self.resample_inputs = bool(resample_inputs)
    self.n_mel_channels = hparams.n_mel_channels
    self.sampling_rate = hparams.sampling_rate
    self.device = device
    self.lib = _lib.load()
    self._owner = stft_handle(self.lib, hparams, device, hparams.window)
    self._h = self._owner.value                # what every call takes; the owner releases it
    basis = slaney_mel_filterbank(hparams.sampling_rate, hparams.filter_length, hparams.n_mel_channels,
                                  hparams.mel_fmin, hparams.mel_fmax)
    self.register_buffer("mel_basis", torch.from_numpy(basis).to(device))

  def spectral_normalize(self, magnitudes):
    return dynamic_range_compression(magnitudes)

  def spectral_de_normalize(self, magnitudes):
    return dynamic_range_decompression(magnitudes)

  def mel_spectrogram(self, y: torch.Tensor) -> torch.Tensor:
    """(B, T) in [-1, 1] -> (B, n_mel_channels, T // hop + 1)   (taco_stft.py:84-104)"""
    assert float(y.min()) >= FLOAT32_64_MIN_WAV and float(y.max()) <= FLOAT32_64_MAX_WAV   # taco_stft.py:95-97
    y = y.to(self.device, torch.float32).contiguous()
    return self._mel(y)

  def _mel(self, y: torch.Tensor, lens_dev=None) -> torch.Tensor:
    """wg_stft_mel on contiguous fp32 audio [B, N] on the module's device, with the device copy of the lengths
    (int32 [B]) of a ragged batch or None; no graph."""
    B, N = y.shape
    ws = _args.workspace(self.lib.wg_stft_mel_workspace_bytes(self._h, B, N), y.device,
                         f"mel front-end: audio of {N} samples is too short (reflect padding needs > 512)")
    out = torch.empty((B, self.n_mel_channels, N // 256 + 1), dtype=torch.float32, device=y.device)
    _lib.check(self.lib.wg_stft_mel(self._h, _args.ptr(self.mel_basis), self.n_mel_channels, _args.ptr(y),
                                    _args.ptr(lens_dev), _args.ptr(out), B, N, _args.ptr(ws), ws.numel(),
                                    _args.stream(y.device)))
    return out

  def mel_spectrogram_ragged(self, wavs):
    """``mel_spectrogram`` of several utterances of different lengths in one upload and one ``wg_stft_mel`` call.

    ``wavs``: 1-D float32 CPU tensors in [-1, 1], each longer than 512 samples.  Returns ``(mel, frames)``: ``mel``
    [B, n_mel_channels, Tmax] on the module's device, ``frames[b] = len(wavs[b]) // 256 + 1``; ``mel[b, :, :frames[b]]``
    is bit for bit ``mel_spectrogram(wavs[b][None])[0]`` and the columns behind it are 0.  The reference's range assert
    (taco_stft.py:95-97) runs on the host before the upload, so nothing on the device is synchronised.  No graph."""
    mel, frames, _, _ = self.mel_spectrogram_ragged_keep(wavs)
    return mel, frames

  def mel_spectrogram_ragged_keep(self, wavs):
    """``mel_spectrogram_ragged`` that also returns what it uploaded: ``(mel, frames, audio, lens)`` with ``audio`` fp32
    [B, N] (zero behind an utterance) and ``lens`` int32 [B] on the module's device, for callers that go on working with
    the waveforms there (the pitch metrics of ``validate``)."""
    if len(wavs) == 0:
      raise _lib.WgError("mel_spectrogram_ragged: empty batch")
    lens = []
    for w in wavs:
      if not isinstance(w, torch.Tensor) or w.device.type != "cpu" or w.dtype != torch.float32 or w.dim() != 1:
        raise _lib.WgError("mel_spectrogram_ragged takes 1-D float32 CPU tensors")
      if w.numel() <= 512:
        raise _lib.WgError(f"mel front-end: audio of {w.numel()} samples is too short (reflect padding needs > 512)")
      assert float(w.min()) >= FLOAT32_64_MIN_WAV and float(w.max()) <= FLOAT32_64_MAX_WAV   # taco_stft.py:95-97
      lens.append(int(w.numel()))
    B, N = len(wavs), max(lens)
    host = torch.zeros(4 * (B * N + B), dtype=torch.uint8)           # padded audio, then the lengths: one upload
    audio = host[:4 * B * N].view(torch.float32).view(B, N)
    for b, w in enumerate(wavs):
      audio[b, :lens[b]] = w
    host[4 * B * N:].view(torch.int32).copy_(torch.tensor(lens, dtype=torch.int32))
    dev = host.to(self.device)
    y, lens_dev = dev[:4 * B * N].view(torch.float32).view(B, N), dev[4 * B * N:].view(torch.int32)
    return self._mel(y, lens_dev), [n // 256 + 1 for n in lens], y, lens_dev

  def mel_spectrogram_ragged_device(self, audio: torch.Tensor, lens):
    """``mel_spectrogram_ragged`` of audio that is on the device already (synthesised audio on its way to the metrics).

    ``audio``: fp32 [B, N] on the module's device, row b holding ``lens[b]`` samples; ``lens``: B integers as
    ``_args.counts`` takes them (a list, a tuple or a 1-D CPU tensor of an integer dtype; a float or a bool entry raises
    WgError), each in (512, N].  Returns ``(mel, frames, frames_dev)``: ``mel`` [B, n_mel_channels, N // 256 + 1],
    ``frames[b] = lens[b] // 256 + 1`` as a list and as an int32 tensor on the device; ``mel[b, :, :frames[b]]`` is bit
    for bit ``mel_spectrogram(audio[b:b+1, :lens[b]])[0]`` and the columns behind it are 0.  The device copy of ``lens``
    is uploaded here.  No range assert and no synchronise: the caller answers for the audio lying in [-1, 1].  No
    graph."""
    _args.tensor("mel_spectrogram_ragged_device: audio", audio, device=self.device, ndim=2)
    B, N = audio.shape
    if B < 1:
      raise _lib.WgError("mel_spectrogram_ragged_device: empty batch")
    # checked only (no device): the lengths go up together with the frame counts, in one tensor, below
    lens = _args.counts("mel_spectrogram_ragged_device: lengths", lens, B, 513, N, device=None)[1]
    audio = audio.contiguous()
    both = torch.tensor([lens, [n // 256 + 1 for n in lens]], dtype=torch.int32).to(audio.device)
    return self._mel(audio, both[0]), [n // 256 + 1 for n in lens], both[1]

  def mel_spectrogram_differentiable(self, y: torch.Tensor, lengths=None) -> torch.Tensor:
    """``mel_spectrogram(y)`` with an autograd graph back to ``y`` (taco_stft.py:84-104 without the detach at :99).

    ``lengths``: B integers as ``_args.counts`` takes them (a list, a tuple or a 1-D CPU tensor of an integer dtype; a
    float or a bool entry raises WgError), each in (512, N]: the sample counts of a padded batch.  The result is then
    what ``mel_spectrogram_ragged_device(y, lengths)`` returns as ``mel``, bit for bit: row b is the mel of the crop
    ``y[b, :lengths[b]]`` in its first ``lengths[b] // 256 + 1`` columns and 0 behind them.  Its backward ignores the
    gradient of those zero columns, gives ``y.grad[b, :lengths[b]]`` the bits of the crop's own backward (reflect
    padding about its own last sample) and ``y.grad[b, lengths[b]:] = 0``.

    ``y`` [B, N] fp32 on the module's device, any N > 512 -> [B, n_mel_channels, N // 256 + 1], bit-identical to
    ``mel_spectrogram``.  No range assert and no host synchronisation: generated audio may leave [-1, 1].  With grad
    mode on and ``y.requires_grad`` the result's graph leads to ``y``; otherwise it is the same tensor without one.
    ``mel_basis`` is a constant.  Other devices, CPU tensors and other dtypes raise WgError."""
    _args.tensor("mel_spectrogram_differentiable: audio", y, device=self.device, ndim=2)
    if lengths is not None:
      B, N = y.shape
      graph = torch.is_grad_enabled() and y.requires_grad
      lens_dev, lens = _args.counts("mel_spectrogram_differentiable: lengths", lengths, B, 513, N,
                                    device=y.device if graph else None)
      return _MelFn.apply(self, y, lens_dev) if graph else self.mel_spectrogram_ragged_device(y.detach(), lens)[0]
    if torch.is_grad_enabled() and y.requires_grad:
      return _MelFn.apply(self, y, None)
    return self._mel(y.detach().contiguous())

  def get_wav_tensor_from_file(self, wav_path) -> torch.Tensor:
    wav, sampling_rate = wav_to_float32(wav_path) if not self.resample_inputs else read_wav_raw(wav_path)
    if sampling_rate != self.sampling_rate:
      if not self.resample_inputs:
        raise ValueError(f"{wav_path}: The sampling rate of the file ({sampling_rate}Hz) doesn't match the target "
                         f"sampling rate ({self.sampling_rate}Hz)!")
      # one upload (int16 stays int16), one launch, one copy back: this path hands out a CPU tensor, as the reference's
      from .resample import resample
      if wav.ndim != 1:
        raise ValueError(f"{wav_path}: only mono files can be resampled")
      if wav.shape[0] == 0:
        return torch.zeros(0, dtype=torch.float32)
      if wav.dtype != np.int16:
        wav = np.ascontiguousarray(convert_wav(wav, np.float32), dtype=np.float32)
      out, lens = resample(torch.from_numpy(wav[None]).to(self.device), None, sampling_rate, self.sampling_rate, clip=True)
      return out[0, :lens[0]].cpu()
    return _float32_tensor(wav)

  def get_mel_tensor_from_file(self, wav_path) -> torch.Tensor:
    return self.get_mel_tensor(self.get_wav_tensor_from_file(wav_path))

  def get_mel_tensors_from_files(self, wav_paths):
    """``mel_spectrogram_ragged`` of wav files (each checked like ``get_wav_tensor_from_file``): ``(mel, frames)``.  With
    ``resample_inputs`` files of other rates are resampled on the device first (``_resampled_from_files``)."""
    mel, frames, _, _ = self.get_mel_and_wav_tensors_from_files(wav_paths)
    return mel, frames

  def get_mel_and_wav_tensors_from_files(self, wav_paths):
    """``mel_spectrogram_ragged_keep`` of wav files, each read once: ``(mel, frames, audio, lens)``.  With
    ``resample_inputs`` and a file of another rate, ``audio`` / ``lens`` are the resampled ones."""
    if self.resample_inputs:
      files = [read_wav_raw(p) for p in wav_paths]
      if all(sr == self.sampling_rate for _, sr in files):                  # today's way, on the arrays just read
        return self.mel_spectrogram_ragged_keep([_float32_tensor(w) for w, _ in files])
      for p, (w, sr) in zip(wav_paths, files):
        if w.ndim != 1:
          raise ValueError(f"{p}: only mono files can be resampled or batched with resampled ones")
      audio, lens = self._resampled_from_files(files)
      mel, frames, _ = self.mel_spectrogram_ragged_device(audio, lens)
      return mel, frames, audio, torch.tensor(lens, dtype=torch.int32).to(self.device)
    return self.mel_spectrogram_ragged_keep([self.get_wav_tensor_from_file(p) for p in wav_paths])

  def _resampled_from_files(self, files):
    """``files``: ``(samples, rate)`` of mono files as ``read_wav_raw`` gives them, at least one at a rate other than the model's.
    Returns ``(audio, lens)``: fp32 [B, N] on the module's device in the order of the files, row b holding ``lens[b]``
    samples at the model's rate in [-1, 1], and the host list of the lengths (each above 512, WgError otherwise).  The
    files go up as read, one upload and one ``wg_resample`` call (``clip=True``) per distinct rate; files at the model's
    rate are converted and range-checked on the host as ``mel_spectrogram_ragged_keep`` does it and only copied.  Nothing
    comes back to the host and nothing synchronises."""
    from .resample import resample
    B = len(files)
    groups = {}
    for i, (_, sr) in enumerate(files):
      groups.setdefault(int(sr), []).append(i)
    lens, parts = [0] * B, []
    for sr, idx in groups.items():
      wavs = [files[i][0] for i in idx]
      n = [int(w.shape[0]) for w in wavs]
      if sr == self.sampling_rate or not all(w.dtype == np.int16 for w in wavs):
        wavs = [np.ascontiguousarray(convert_wav(w, np.float32), dtype=np.float32) for w in wavs]
        for w in wavs:
          if w.size:
            assert float(w.min()) >= FLOAT32_64_MIN_WAV and float(w.max()) <= FLOAT32_64_MAX_WAV   # taco_stft.py:95-97
      host = np.zeros((len(idx), max(max(n), 1)), dtype=wavs[0].dtype)
      for k, w in enumerate(wavs):
        host[k, :n[k]] = w
      dev = torch.from_numpy(host).to(self.device)
      if sr != self.sampling_rate:
        dev, n = resample(dev, n, sr, self.sampling_rate, clip=True)
      for k, i in enumerate(idx):
        lens[i] = n[k]
      parts.append((idx, dev))
    for n in lens:
      if n <= 512:
        raise _lib.WgError(f"mel front-end: audio of {n} samples is too short (reflect padding needs > 512)")
    if len(parts) == 1:                                    # one rate: the resampled batch is in file order already
      return parts[0][1][:, :max(lens)].contiguous(), lens
    audio = torch.zeros((B, max(lens)), dtype=torch.float32, device=self.device)
    for idx, dev in parts:
      w = min(dev.shape[1], audio.shape[1])
      audio[:, :w].index_copy_(0, torch.tensor(idx, dtype=torch.int64).to(self.device), dev[:, :w])
    return audio, lens

  def get_mel_tensor(self, wav_tensor: torch.Tensor) -> torch.Tensor:
    return self.mel_spectrogram(wav_tensor.unsqueeze(0)).squeeze(0)
