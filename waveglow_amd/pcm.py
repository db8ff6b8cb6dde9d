"""int16 PCM of a synthesised batch, finished on the device (``wg_wav_finish``): per utterance what the host path does
with ``is_overamp`` on the raw audio and ``convert_wav(normalize_wav(denoised), int16)`` (audio.py; src/waveglow/
audio_utils.py:36-95, :132-138), bit for bit, so that one int16 copy comes back instead of two fp32 copies per utterance.
No CPU fallback."""
from __future__ import annotations

import numpy as np
import torch

from . import _args, _lib

# columns of the statistics, one row of 8 floats per utterance (include/waveglow_amd.h: wg_wav_finish)
RAW_MIN, RAW_MAX, RAW_PEAK, DEN_MIN, DEN_MAX, DEN_PEAK, NON_FINITE = range(7)
N_STATS = 8


def finish_enqueue(raw: torch.Tensor, denoised: torch.Tensor, lengths_dev: torch.Tensor) -> torch.Tensor:
  """Enqueue ``wg_wav_finish`` on the current stream.  ``raw`` / ``denoised``: contiguous fp32 [B, N] on one GPU (N a
  multiple of 8; they may be the same tensor), ``lengths_dev``: int32 [B] on that GPU.  Returns one uint8 device
  buffer: the int16 samples [B, N], then the statistics [B, 8] fp32 -- what ``finish_read`` takes apart on the host."""
  if raw.device.type != "cuda" or denoised.device != raw.device or lengths_dev.device != raw.device:
    raise _lib.WgError("wav finish runs on the GPU library only: audio and lengths must be on one GPU")
  if raw.dtype != torch.float32 or denoised.dtype != torch.float32 or lengths_dev.dtype != torch.int32:
    raise _lib.WgError("wav finish takes float32 audio and int32 lengths")
  if raw.dim() != 2 or raw.shape != denoised.shape or not raw.is_contiguous() or not denoised.is_contiguous():
    raise _lib.WgError("wav finish takes contiguous audio [B, N], raw and denoised of one shape")
  B, N = raw.shape
  if lengths_dev.numel() != B:
    raise _lib.WgError(f"wav finish: {lengths_dev.numel()} lengths for a batch of {B}")
  lib = _lib.load()
  out = torch.empty(2 * B * N + 4 * N_STATS * B, dtype=torch.uint8, device=raw.device)
  ws = torch.empty(lib.wg_wav_finish_workspace_bytes(B), dtype=torch.uint8, device=raw.device)
  _lib.check(lib.wg_wav_finish(_args.ptr(raw), _args.ptr(denoised), _args.ptr(lengths_dev), _args.ptr(out),
                               out.data_ptr() + 2 * B * N, B, N, _args.ptr(ws), ws.numel(), _args.stream(raw.device)))
  return out


def finish_read(host: torch.Tensor, B: int, N: int):
  """(pcm int16 [B, N], stats fp32 [B, 8]) as numpy views of the host copy of ``finish_enqueue``'s buffer.  Raises WgError
  naming the first utterance with a NaN or infinite sample (the host path fails its own asserts on such audio)."""
  buf = host.numpy()
  pcm = buf[:2 * B * N].view(np.int16).reshape(B, N)
  stats = buf[2 * B * N:2 * B * N + 4 * N_STATS * B].view(np.float32).reshape(B, N_STATS)
  bad = np.nonzero(stats[:, NON_FINITE])[0]
  if bad.size:
    raise _lib.WgError(f"utterance {int(bad[0])} of the batch has NaN or infinite samples: it cannot be written as PCM")
  return pcm, stats


def finish(raw: torch.Tensor, denoised: torch.Tensor, lengths):
  """``finish_enqueue`` + one copy to the host + one synchronise.  ``lengths``: B sample counts in [1, N].
  Returns (pcm int16 [B, N] with zeros behind each utterance, stats fp32 [B, 8])."""
  B, N = raw.shape
  out = finish_enqueue(raw, denoised, _args.counts("wav finish: lengths", lengths, B, 1, N, device=raw.device)[0])
  host = out.cpu()
  return finish_read(host, B, N)
