"""Validation metrics of mel-spectrogram pairs on the device (``wg_metrics_*``): MFCCs, mel-cepstral distortion with and
without exact dynamic time warping, the alignment penalties and the per-channel cosine similarity -- what the reference's
``validate`` computes per utterance on the host with ``mel_cepstral_distance.get_metrics_mels(n_mfcc=16, take_log=False)``
and ``cosine_dist_mels`` (src/waveglow/validation.py:211-235, utils.py:510-523).

Ragged batches in the project's usual form: fp32 tensors ``[B, C, Tmax]`` on one GPU and per-utterance frame counts.
Everything is enqueued on the current stream; only ``mel_metrics`` copies to the host.  The definitions are stated in
include/waveglow_amd.h and DESIGN.md section 7; parity with the ``mel_cepstral_distance`` package itself is unpinned (the
package is absent), and the alignment here is exact where that package's ``fastdtw`` is approximate.  No CPU fallback.
"""
from __future__ import annotations

import ctypes as C
from dataclasses import dataclass
from typing import List, Optional, Sequence, Tuple, Union

import torch

from . import _lib

MAX_FRAMES = 4096       # frames per utterance (include/waveglow_amd.h: wg_metrics_*)
MAX_FEATURES = 128      # mel channels / feature rows
N_ROW = 8               # fp64 values per utterance of the fused call
MCD, PENALTY, FRAMES, MCD_DTW, PENALTY_DTW, FRAMES_DTW, COSINE = range(7)

Frames = Union[None, Sequence[int], torch.Tensor]


@dataclass
class MelMetrics:
  mcd: float              # mean frame distance of the MFCCs, the shorter utterance's MFCCs zero behind its end
  penalty: float          # 2 - (Ta + Tb) / frames
  frames: int             # max(Ta, Tb)
  mcd_dtw: float          # cost of the optimal warping path / its length
  penalty_dtw: float      # 2 - (Ta + Tb) / frames_dtw
  frames_dtw: int         # length of the optimal warping path
  cosine: float           # 1 - mean over the mel channels of the cosine distance, zero-padded in time


def _features(name: str, x, device=None) -> torch.Tensor:
  if not isinstance(x, torch.Tensor) or x.device.type != "cuda":
    raise _lib.WgError(f"{name}: the metrics run on the GPU library only (no CPU fallback)")
  if device is not None and x.device != device:
    raise _lib.WgError(f"{name}: both sides must be on one GPU, got {x.device} and {device}")
  if x.dtype != torch.float32:
    raise _lib.WgError(f"{name} takes float32, got {x.dtype}")
  if x.dim() != 3:
    raise _lib.WgError(f"{name} takes [B, C, T], got shape {tuple(x.shape)}")
  B, K, T = x.shape
  if B < 1 or not 1 <= K <= MAX_FEATURES or not 1 <= T <= MAX_FRAMES:
    raise _lib.WgError(f"{name}: B >= 1, 1 <= C <= {MAX_FEATURES} and 1 <= T <= {MAX_FRAMES} expected, "
                       f"got shape {tuple(x.shape)}")
  return x.contiguous()


def _frames(name: str, frames: Frames, x: torch.Tensor) -> torch.Tensor:
  """int32 [B] on x's device.  A host list is range-checked here; a device tensor is never read on the host (the kernels
  treat a count outside the limits as 0)."""
  B, _, T = x.shape
  if frames is None:
    frames = [T] * B
  if isinstance(frames, torch.Tensor) and frames.device.type == "cuda":
    if frames.device != x.device or frames.dtype != torch.int32 or frames.dim() != 1 or frames.numel() != B:
      raise _lib.WgError(f"{name}: frame counts on the device must be int32 [{B}] on {x.device}")
    return frames.contiguous()
  host = [int(n) for n in (frames.tolist() if isinstance(frames, torch.Tensor) else frames)]
  if len(host) != B:
    raise _lib.WgError(f"{name}: {len(host)} frame counts for a batch of {B}")
  if any(n < 1 or n > min(T, MAX_FRAMES) for n in host):
    raise _lib.WgError(f"{name}: frame counts in [1, {min(T, MAX_FRAMES)}] expected, got {host}")
  return torch.tensor(host, dtype=torch.int32).to(x.device)


def _stream(x: torch.Tensor):
  return C.c_void_p(torch.cuda.current_stream(x.device).cuda_stream)


def mfcc(mel: torch.Tensor, frames: Frames = None, n_mfcc: int = 16) -> torch.Tensor:
  """Coefficients 1 .. n_mfcc of the orthonormal DCT-II over the mel axis: [B, n_mel, T] -> [B, n_mfcc, T] fp32, fp64
  inside, rounded once; columns behind an utterance's frames are 0.  The mel is a log-mel already: no logarithm."""
  mel = _features("mfcc: mel", mel)
  B, n_mel, T = mel.shape
  if not 1 <= n_mfcc < n_mel:
    raise _lib.WgError(f"mfcc: 1 <= n_mfcc < n_mel expected, got {n_mfcc} of {n_mel}")
  fr = _frames("mfcc", frames, mel)
  lib = _lib.load()
  out = torch.empty((B, n_mfcc, T), dtype=torch.float32, device=mel.device)
  ws = torch.empty(lib.wg_metrics_workspace_bytes(B, n_mel, n_mfcc, T, T), dtype=torch.uint8, device=mel.device)
  with torch.cuda.device(mel.device):
    _lib.check(lib.wg_metrics_mfcc(mel.data_ptr(), fr.data_ptr(), out.data_ptr(), B, n_mel, n_mfcc, T, ws.data_ptr(),
                                   ws.numel(), _stream(mel)))
  return out


def dtw_distance(feat_a: torch.Tensor, frames_a: Frames, feat_b: torch.Tensor,
                 frames_b: Frames) -> Tuple[torch.Tensor, torch.Tensor]:
  """Exact dynamic time warping of the columns of ``feat_a`` [B, K, Ta] against those of ``feat_b`` [B, K, Tb] under the
  Euclidean frame distance: ``(cost fp64 [B], frames int32 [B])`` on the device, the cost of the optimal path and its
  length.  Ties between predecessors go to (i-1, j), then (i, j-1), then (i-1, j-1)."""
  a = _features("dtw_distance: feat_a", feat_a)
  b = _features("dtw_distance: feat_b", feat_b, a.device)
  if a.shape[0] != b.shape[0] or a.shape[1] != b.shape[1]:
    raise _lib.WgError(f"dtw_distance: batch and feature sizes differ, {tuple(a.shape)} against {tuple(b.shape)}")
  fa, fb = _frames("dtw_distance: frames_a", frames_a, a), _frames("dtw_distance: frames_b", frames_b, b)
  B, K, Ta = a.shape
  cost = torch.empty(B, dtype=torch.float64, device=a.device)
  length = torch.empty(B, dtype=torch.int32, device=a.device)
  with torch.cuda.device(a.device):
    _lib.check(_lib.load().wg_metrics_dtw(a.data_ptr(), fa.data_ptr(), b.data_ptr(), fb.data_ptr(), cost.data_ptr(),
                                          length.data_ptr(), B, K, Ta, b.shape[2], _stream(a)))
  return cost, length


def mel_metrics_enqueue(mel_a: torch.Tensor, frames_a: Frames, mel_b: torch.Tensor, frames_b: Frames,
                        n_mfcc: int = 16) -> torch.Tensor:
  """All metrics of the pairs (mel_a[b], mel_b[b]) in one launch sequence, no synchronise: fp64 [B, 8] on the device,
  columns MCD, PENALTY, FRAMES, MCD_DTW, PENALTY_DTW, FRAMES_DTW, COSINE and one reserved."""
  a = _features("mel_metrics: mel_a", mel_a)
  b = _features("mel_metrics: mel_b", mel_b, a.device)
  if a.shape[0] != b.shape[0] or a.shape[1] != b.shape[1]:
    raise _lib.WgError(f"mel_metrics: batch and channel sizes differ, {tuple(a.shape)} against {tuple(b.shape)}")
  B, n_mel, Ta = a.shape
  Tb = b.shape[2]
  if not 1 <= n_mfcc < n_mel:
    raise _lib.WgError(f"mel_metrics: 1 <= n_mfcc < n_mel expected, got {n_mfcc} of {n_mel}")
  fa, fb = _frames("mel_metrics: frames_a", frames_a, a), _frames("mel_metrics: frames_b", frames_b, b)
  lib = _lib.load()
  rows = torch.empty((B, N_ROW), dtype=torch.float64, device=a.device)
  ws = torch.empty(lib.wg_metrics_workspace_bytes(B, n_mel, n_mfcc, Ta, Tb), dtype=torch.uint8, device=a.device)
  with torch.cuda.device(a.device):
    _lib.check(lib.wg_metrics_mel(a.data_ptr(), fa.data_ptr(), b.data_ptr(), fb.data_ptr(), rows.data_ptr(), B, n_mel,
                                  n_mfcc, Ta, Tb, ws.data_ptr(), ws.numel(), _stream(a)))
  return rows


def rows_to_metrics(rows) -> List[MelMetrics]:
  """Host copy of ``mel_metrics_enqueue``'s rows -> one MelMetrics per utterance."""
  out = []
  for r in rows.tolist():
    nan = r[FRAMES] != r[FRAMES]
    out.append(MelMetrics(mcd=r[MCD], penalty=r[PENALTY], frames=0 if nan else int(r[FRAMES]), mcd_dtw=r[MCD_DTW],
                          penalty_dtw=r[PENALTY_DTW], frames_dtw=0 if nan else int(r[FRAMES_DTW]), cosine=r[COSINE]))
  return out


def mel_metrics(mel_a: torch.Tensor, frames_a: Frames, mel_b: torch.Tensor, frames_b: Frames,
                n_mfcc: int = 16) -> List[MelMetrics]:
  """``mel_metrics_enqueue`` + one copy to the host + one stream synchronise."""
  rows = mel_metrics_enqueue(mel_a, frames_a, mel_b, frames_b, n_mfcc)
  host = torch.empty(rows.shape, dtype=rows.dtype, pin_memory=True)
  host.copy_(rows, non_blocking=True)
  torch.cuda.current_stream(rows.device).synchronize()
  return rows_to_metrics(host)
