"""Validation metrics on the device.  Of mel-spectrogram pairs (``wg_metrics_*``): MFCCs, mel-cepstral distortion with and
without exact dynamic time warping, the alignment penalties and the per-channel cosine similarity -- what the reference's
``validate`` computes per utterance on the host with ``mel_cepstral_distance.get_metrics_mels(n_mfcc=16, take_log=False)``
and ``cosine_dist_mels`` (src/waveglow/validation.py:211-235, utils.py:510-523).

Ragged batches in the project's usual form: fp32 tensors ``[B, C, Tmax]`` on one GPU and per-utterance frame counts.
Everything is enqueued on the current stream; only ``mel_metrics`` copies to the host.  The definitions are stated in
include/waveglow_amd.h and DESIGN.md section 7; parity with the ``mel_cepstral_distance`` package itself is unpinned (the
package is absent), and the alignment here is exact where that package's ``fastdtw`` is approximate.  No CPU fallback.

Of audio pairs (``wg_pitch_*``, the second half of this file): a YIN F0 tracker (steps 1-5 of de Cheveigne & Kawahara 2002)
over fp32 audio ``[B, N]`` with per-utterance sample counts, and the F0 RMSE, gross pitch error and voicing decision error of
two tracks.  The reference has no counterpart; parity with any external tracker (librosa's ``yin`` / ``pyin`` and others,
all absent) is unpinned, the numpy restatement tests/_pitch_oracle.py is the yardstick.

Of audio pairs at 10 kHz (``wg_stoi``, the last part of this file): short-time objective intelligibility (STOI, Taal et al.
2011) and its extended form (ESTOI, Jensen and Taal 2016) of a clean and a processed signal, with the project's resampler in
front for other rates.  The reference has no counterpart; parity with ``pystoi`` (absent) is unpinned, the numpy restatement
tests/_stoi_oracle.py is the yardstick.  ``stoi_differentiable`` gives the same two values with a graph back to the
processed signal (``wg_stoi_forward`` / ``wg_stoi_backward``); ``waveglow_amd.STOILoss`` is the loss built on it.
"""
from __future__ import annotations

import ctypes as C
from dataclasses import dataclass
from typing import List, Optional, Sequence, Tuple, Union

import torch

from . import _args, _lib
from ._args import ptr

MAX_FRAMES = 4096       # frames per utterance (include/waveglow_amd.h: wg_metrics_*)
MAX_FEATURES = 128      # mel channels / feature rows
N_ROW = 8               # fp64 values per utterance of the fused call
MCD, PENALTY, FRAMES, MCD_DTW, PENALTY_DTW, FRAMES_DTW, COSINE = range(7)

PITCH_MIN_FRAME, PITCH_MAX_FRAME = 16, 2048      # frame_length (include/waveglow_amd.h: wg_pitch_*)
PITCH_MAX_TAU = 1024                             # largest lag
F0_RMSE_CENTS, F0_RMSE_HZ, GPE, VUV_ERROR, PITCH_FRAMES, VOICED_A, VOICED_B, VOICED_BOTH = range(8)

STOI_RATE = 10000                                # Hz (include/waveglow_amd.h: wg_stoi)
STOI_FRAME, STOI_HOP, STOI_NFFT, STOI_BANDS, STOI_SEGMENT = 256, 128, 512, 15, 30
STOI_MAX_PITCH = 1 << 21                         # samples per row
STOI_FRAME_TILE = 8                              # frames per workgroup of the band-spectra kernel (csrc/wg_stoi.h)
STOI_SEGMENT_TILE = 4                            # segments per workgroup of the segment kernel
STOI, ESTOI, STOI_FRAMES, STOI_FRAMES_KEPT, STOI_SEGMENTS = range(5)

# Per-utterance frame counts and sample counts: None (all), or B integers as ``_args.counts`` takes them (a list, a
# tuple or a 1-D CPU tensor of an integer dtype; a float or a bool entry raises WgError), or an int32 tensor ``[B]`` on
# the device, which is trusted and never read on the host
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


@dataclass
class PitchMetrics:
  f0_rmse_cents: float    # over the frames voiced on both sides; NaN without one
  f0_rmse_hz: float
  gross_pitch_error: float   # share of the both-voiced frames more than 20 % apart
  vuv_error: float        # share of the frames voiced on exactly one side; NaN without a frame
  frames: int             # min(Fa, Fb)
  voiced_a: int
  voiced_b: int
  voiced_both: int


@dataclass
class IntelligibilityMetrics:
  stoi: float             # NaN without a segment (fewer than 30 frames after the silent ones are removed)
  estoi: float
  frames: int             # F0: frames of the common length at 10 kHz
  frames_kept: int        # K: frames within 40 dB of the loudest frame of the clean signal
  segments: int           # J = K - 30, or 0


def _features(name: str, x, device=None) -> torch.Tensor:
  _args.tensor(name, x, device=device, ndim=3)
  B, K, T = x.shape
  if B < 1 or not 1 <= K <= MAX_FEATURES or not 1 <= T <= MAX_FRAMES:
    raise _lib.WgError(f"{name}: B >= 1, 1 <= C <= {MAX_FEATURES} and 1 <= T <= {MAX_FRAMES} expected, "
                       f"got shape {tuple(x.shape)}")
  return x.contiguous()


def _frames(name: str, frames: Frames, x: torch.Tensor, upload: bool = True) -> torch.Tensor:
  """int32 [B] on x's device.  Host counts are range-checked (``_args.counts``); a device tensor is never read on the host
  (the kernels treat a count outside the limits as 0).  Without ``upload`` checked host counts stay on the host, for a
  caller that wants both sides of a pair checked before either goes up."""
  B, _, T = x.shape
  on_device = isinstance(frames, torch.Tensor) and frames.device.type != "cpu"
  return _args.counts(name, [T] * B if frames is None else frames, B, 1, min(T, MAX_FRAMES),
                      device=x.device if upload or on_device else "cpu", allow_device=True)[0]


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
    _lib.check(lib.wg_metrics_mfcc(ptr(mel), ptr(fr), ptr(out), B, n_mel, n_mfcc, T, ptr(ws),
                                   ws.numel(), _args.stream(mel.device)))
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
    _lib.check(_lib.load().wg_metrics_dtw(ptr(a), ptr(fa), ptr(b), ptr(fb), ptr(cost),
                                          ptr(length), B, K, Ta, b.shape[2], _args.stream(a.device)))
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
    _lib.check(lib.wg_metrics_mel(ptr(a), ptr(fa), ptr(b), ptr(fb), ptr(rows), B, n_mel,
                                  n_mfcc, Ta, Tb, ptr(ws), ws.numel(), _args.stream(a.device)))
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


# ------------------------------------------------------------------------------------------------------ pitch metrics
def pitch_params(sampling_rate=22050, frame_length: int = 1024, hop_length: int = 256, fmin: float = 60.0,
                 fmax: float = 600.0, threshold: float = 0.1) -> _lib.WgPitchParams:
  """The tracker's parameters with the lags derived from the frequency range, tau_max = ceil(sr / fmin) and tau_min =
  max(2, floor(sr / fmax)); WgError outside the limits of include/waveglow_amd.h (wg_pitch_*).  Needs no GPU."""
  import math
  try:
    sr, W, H, lo, hi, th = float(sampling_rate), int(frame_length), int(hop_length), float(fmin), float(fmax), \
        float(threshold)
  except (TypeError, ValueError) as e:
    raise _lib.WgError(f"pitch: numeric parameters expected ({e})")
  if W != frame_length or H != hop_length:
    raise _lib.WgError(f"pitch: integer frame_length and hop_length expected, got {frame_length}, {hop_length}")
  if not (math.isfinite(sr) and math.isfinite(lo) and math.isfinite(hi) and 0 < sr < 1e9 and 0 < lo < hi):
    raise _lib.WgError(f"pitch: 0 < fmin < fmax and a sampling rate in (0, 1e9) expected, got {fmin}, {fmax}, {sampling_rate}")
  if not PITCH_MIN_FRAME <= W <= PITCH_MAX_FRAME:
    raise _lib.WgError(f"pitch: frame_length in [{PITCH_MIN_FRAME}, {PITCH_MAX_FRAME}] expected, got {W}")
  if H < 1 or H >= 2 ** 31:
    raise _lib.WgError(f"pitch: hop_length >= 1 expected, got {H}")
  tau_max, tau_min = math.ceil(sr / lo), max(2, math.floor(sr / hi))
  if not 2 <= tau_min < tau_max <= PITCH_MAX_TAU:
    raise _lib.WgError(f"pitch: 2 <= tau_min < tau_max <= {PITCH_MAX_TAU} expected, got lags {tau_min} .. {tau_max} from "
                       f"fmin {fmin}, fmax {fmax} at {sampling_rate} Hz")
  if not 0 < th < 1:
    raise _lib.WgError(f"pitch: threshold in (0, 1) expected, got {threshold}")
  return _lib.WgPitchParams(sr, th, W, H, tau_min, tau_max)


def pitch_frames(n_samples: int, p: _lib.WgPitchParams) -> int:
  """F(n_samples): (n - W - tau_max) // H + 1, or 0 for fewer than W + tau_max samples."""
  need = p.frame_length + p.tau_max
  return (n_samples - need) // p.hop_length + 1 if n_samples >= need else 0


def _audio(name: str, x, device=None) -> torch.Tensor:
  _args.tensor(name, x, device=device, ndim=2)
  if x.shape[0] < 1 or x.shape[0] > 65535 or x.shape[1] < 1 or x.shape[1] >= 2 ** 31:
    raise _lib.WgError(f"{name} takes [B, N] with 1 <= B <= 65535 and N >= 1, got shape {tuple(x.shape)}")
  return x.contiguous()


def _lengths(name: str, lengths: Frames, x: torch.Tensor) -> torch.Tensor:
  """int32 [B] on x's device.  Host counts are range-checked (``_args.counts``); a device tensor is never read on the host
  (the kernels treat a length outside [0, N] as 0 frames)."""
  B, N = x.shape
  return _args.counts(name, [N] * B if lengths is None else lengths, B, 0, N, device=x.device, allow_device=True)[0]


def yin_f0(audio: torch.Tensor, lengths: Frames = None, *, sampling_rate=22050, frame_length: int = 1024,
           hop_length: int = 256, fmin: float = 60.0, fmax: float = 600.0,
           threshold: float = 0.1) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
  """YIN tracks (steps 1-5, include/waveglow_amd.h: wg_pitch_yin) of fp32 audio [B, N] on one GPU: ``(f0, aperiodicity,
  frames)``, fp64 [B, Fmax] twice and int32 [B], on the device.  Fmax = max(1, F(N)); utterance b has ``frames[b]`` =
  F(lengths[b]) frames, 0 behind them; an unvoiced frame has f0 = 0.  Nothing behind an utterance's length is read."""
  p = pitch_params(sampling_rate, frame_length, hop_length, fmin, fmax, threshold)
  x = _audio("yin_f0: audio", audio)
  ln = _lengths("yin_f0", lengths, x)
  B, N = x.shape
  F = max(1, pitch_frames(N, p))
  f0 = torch.empty((B, F), dtype=torch.float64, device=x.device)
  ap = torch.empty((B, F), dtype=torch.float64, device=x.device)
  frames = torch.empty(B, dtype=torch.int32, device=x.device)
  with torch.cuda.device(x.device):
    _lib.check(_lib.load().wg_pitch_yin(ptr(x), ptr(ln), C.byref(p), ptr(f0), ptr(ap),
                                        ptr(frames), B, N, F, _args.stream(x.device)))
  return f0, ap, frames


def pitch_compare(f0_a: torch.Tensor, frames_a: torch.Tensor, f0_b: torch.Tensor, frames_b: torch.Tensor) -> torch.Tensor:
  """Rows fp64 [B, 8] (wg_pitch_compare) of two track sets as ``yin_f0`` returns them: fp64 [B, F] and int32 [B] on one
  GPU."""
  fr = []
  for name, f0, frames in (("f0_a", f0_a, frames_a), ("f0_b", f0_b, frames_b)):
    _args.tensor(f"pitch_compare: {name}", f0, device=getattr(f0_a, "device", None), dtypes=(torch.float64,), ndim=2)
    B, F = f0.shape
    if not 1 <= B <= 65535 or F < 1 or B != f0_a.shape[0]:
      raise _lib.WgError(f"pitch_compare: {name} takes [B, F] with 1 <= B <= 65535 and F >= 1, one B on both sides, got "
                         f"{tuple(f0.shape)}")
    fr.append(_args.counts(f"pitch_compare: frames of {name}", frames, B, 0, F, device=f0.device, allow_device=True)[0])
  a, b = f0_a.contiguous(), f0_b.contiguous()
  rows = torch.empty((a.shape[0], N_ROW), dtype=torch.float64, device=a.device)
  with torch.cuda.device(a.device):
    _lib.check(_lib.load().wg_pitch_compare(ptr(a), ptr(fr[0]), ptr(b), ptr(fr[1]), ptr(rows), a.shape[0], a.shape[1],
                                            b.shape[1], _args.stream(a.device)))
  return rows


def pitch_metrics_enqueue(audio_a: torch.Tensor, lengths_a: Frames, audio_b: torch.Tensor, lengths_b: Frames, *,
                          sampling_rate=22050, frame_length: int = 1024, hop_length: int = 256, fmin: float = 60.0,
                          fmax: float = 600.0, threshold: float = 0.1) -> torch.Tensor:
  """The pitch metrics of the pairs (audio_a[b], audio_b[b]), a the original and b the synthesised audio, aligned frame
  by frame, in one launch sequence without a synchronise: fp64 [B, 8] on the device, columns F0_RMSE_CENTS, F0_RMSE_HZ,
  GPE, VUV_ERROR, PITCH_FRAMES, VOICED_A, VOICED_B, VOICED_BOTH (wg_pitch_metrics)."""
  p = pitch_params(sampling_rate, frame_length, hop_length, fmin, fmax, threshold)
  a = _audio("pitch_metrics: audio_a", audio_a)
  b = _audio("pitch_metrics: audio_b", audio_b, a.device)
  if a.shape[0] != b.shape[0]:
    raise _lib.WgError(f"pitch_metrics: batch sizes differ, {tuple(a.shape)} against {tuple(b.shape)}")
  la, lb = _lengths("pitch_metrics: lengths_a", lengths_a, a), _lengths("pitch_metrics: lengths_b", lengths_b, b)
  B = a.shape[0]
  lib = _lib.load()
  rows = torch.empty((B, N_ROW), dtype=torch.float64, device=a.device)
  ws = torch.empty(lib.wg_pitch_workspace_bytes(C.byref(p), B, a.shape[1], b.shape[1]), dtype=torch.uint8, device=a.device)
  with torch.cuda.device(a.device):
    _lib.check(lib.wg_pitch_metrics(ptr(a), ptr(la), a.shape[1], ptr(b), ptr(lb), b.shape[1],
                                    C.byref(p), ptr(rows), B, ptr(ws), ws.numel(), _args.stream(a.device)))
  return rows


def rows_to_pitch_metrics(rows) -> List[PitchMetrics]:
  """Host copy of ``pitch_metrics_enqueue``'s rows -> one PitchMetrics per pair."""
  return [PitchMetrics(f0_rmse_cents=r[F0_RMSE_CENTS], f0_rmse_hz=r[F0_RMSE_HZ], gross_pitch_error=r[GPE],
                       vuv_error=r[VUV_ERROR], frames=int(r[PITCH_FRAMES]), voiced_a=int(r[VOICED_A]),
                       voiced_b=int(r[VOICED_B]), voiced_both=int(r[VOICED_BOTH])) for r in rows.tolist()]


def pitch_metrics(audio_a: torch.Tensor, lengths_a: Frames, audio_b: torch.Tensor, lengths_b: Frames,
                  **params) -> List[PitchMetrics]:
  """``pitch_metrics_enqueue`` + one copy to the host + one stream synchronise."""
  rows = pitch_metrics_enqueue(audio_a, lengths_a, audio_b, lengths_b, **params)
  host = torch.empty(rows.shape, dtype=rows.dtype, pin_memory=True)
  host.copy_(rows, non_blocking=True)
  torch.cuda.current_stream(rows.device).synchronize()
  return rows_to_pitch_metrics(host)


# -------------------------------------------------------------------------------------------- intelligibility metrics
_stoi_tables = {}        # device index -> (blob on that device, WgStoiParams pointing into it)


def stoi_window():
  """fp64 [256]: w[i] = 0.5 - 0.5 cos(2 pi (i + 1) / 257), numpy's hanning(258) without its zero ends."""
  import numpy as np
  return np.hanning(STOI_FRAME + 2)[1:-1].copy()


def stoi_band_table():
  """int32 [15, 2]: (lo, hi) of the one-third-octave bands at 10 kHz; band b sums the bins lo .. hi - 1."""
  import numpy as np
  f = np.linspace(0, STOI_RATE, STOI_NFFT + 1)[:STOI_NFFT // 2 + 1]
  k = np.arange(STOI_BANDS, dtype=np.float64)
  edges = [150.0 * 2.0 ** ((2 * k - 1) / 6), 150.0 * 2.0 ** ((2 * k + 1) / 6)]
  return np.array([[int(np.argmin((f - v) ** 2)) for v in e] for e in edges], dtype=np.int32).T.copy()


def stoi_frames(n_samples: int) -> int:
  """F0(n_samples): the frame starts are range(0, n - 256, 128)."""
  return len(range(0, int(n_samples) - STOI_FRAME, STOI_HOP))


def _stoi_params(device: torch.device) -> _lib.WgStoiParams:
  """The tables wg_stoi reads, made on the host in fp64 and uploaded once per device: window | cos/sin | bands."""
  import numpy as np
  key = _lib.device_index(device)
  hit = _stoi_tables.get(key)
  if hit is None:
    ang = 2.0 * np.pi * np.arange(STOI_NFFT, dtype=np.float64) / STOI_NFFT
    cossin = np.stack([np.cos(ang), np.sin(ang)], axis=1)
    host = np.concatenate([stoi_window().view(np.uint8), np.ascontiguousarray(cossin).view(np.uint8).ravel(),
                           stoi_band_table().view(np.uint8).ravel()])
    blob = torch.from_numpy(host).to(device)
    base = blob.data_ptr()
    off_cs = STOI_FRAME * 8
    off_bands = off_cs + STOI_NFFT * 16
    hit = _stoi_tables[key] = (blob, _lib.WgStoiParams(base, base + off_bands, base + off_cs))
  return hit[1]


def _stoi_audio(name: str, x, device=None) -> torch.Tensor:
  x = _audio(name, x, device)
  if x.shape[1] > STOI_MAX_PITCH:
    raise _lib.WgError(f"{name}: rows of at most {STOI_MAX_PITCH} samples at 10 kHz expected, got {x.shape[1]}")
  return x


def stoi_enqueue(x10k: torch.Tensor, lengths_x: Frames, y10k: torch.Tensor, lengths_y: Frames) -> torch.Tensor:
  """STOI and ESTOI of the pairs (x10k[b], y10k[b]), x the clean and y the processed signal, fp32 [B, N] on one GPU and
  already at 10 kHz, cropped to the common length of a pair; one launch sequence without a synchronise: fp64 [B, 8] on the
  device, columns STOI, ESTOI, STOI_FRAMES, STOI_FRAMES_KEPT, STOI_SEGMENTS and three zeros (wg_stoi).  Both sides share
  one row pitch: the shorter tensor is padded on the device."""
  x = _stoi_audio("stoi: x10k", x10k)
  y = _stoi_audio("stoi: y10k", y10k, x.device)
  if x.shape[0] != y.shape[0]:
    raise _lib.WgError(f"stoi: batch sizes differ, {tuple(x.shape)} against {tuple(y.shape)}")
  lx, ly = _lengths("stoi: lengths_x", lengths_x, x), _lengths("stoi: lengths_y", lengths_y, y)
  B, N = x.shape[0], max(x.shape[1], y.shape[1])
  if x.shape[1] < N:
    x = torch.nn.functional.pad(x, (0, N - x.shape[1]))
  if y.shape[1] < N:
    y = torch.nn.functional.pad(y, (0, N - y.shape[1]))
  lib = _lib.load()
  with torch.cuda.device(x.device):
    p = _stoi_params(x.device)
    rows = torch.empty((B, N_ROW), dtype=torch.float64, device=x.device)
    ws = torch.empty(lib.wg_stoi_workspace_bytes(B, N), dtype=torch.uint8, device=x.device)
    _lib.check(lib.wg_stoi(ptr(x), ptr(lx), ptr(y), ptr(ly), B, N, C.byref(p), ptr(rows),
                           ptr(ws), ws.numel(), _args.stream(x.device)))
  return rows


def rows_to_intelligibility_metrics(rows) -> List[IntelligibilityMetrics]:
  """Host copy of ``stoi_enqueue``'s rows -> one IntelligibilityMetrics per pair."""
  return [IntelligibilityMetrics(stoi=r[STOI], estoi=r[ESTOI], frames=int(r[STOI_FRAMES]),
                                 frames_kept=int(r[STOI_FRAMES_KEPT]), segments=int(r[STOI_SEGMENTS])) for r in rows.tolist()]


def _read_rows(rows: torch.Tensor):
  host = torch.empty(rows.shape, dtype=rows.dtype, pin_memory=True)
  host.copy_(rows, non_blocking=True)
  torch.cuda.current_stream(rows.device).synchronize()
  return host


def stoi(x10k: torch.Tensor, lengths_x: Frames, y10k: torch.Tensor, lengths_y: Frames) -> List[IntelligibilityMetrics]:
  """``stoi_enqueue`` + one copy to the host + one stream synchronise."""
  return rows_to_intelligibility_metrics(_read_rows(stoi_enqueue(x10k, lengths_x, y10k, lengths_y)))


def intelligibility_metrics_enqueue(audio_a: torch.Tensor, lengths_a: Frames, audio_b: torch.Tensor, lengths_b: Frames,
                                    sampling_rate=22050) -> torch.Tensor:
  """STOI and ESTOI of the pairs (audio_a[b], audio_b[b]), a the original (clean) and b the synthesised audio, fp32 [B, N]
  on one GPU at ``sampling_rate``: the common length of a pair is taken on the device, both sides are resampled to 10 kHz by
  ``resample.resample_enqueue`` (scipy's default Kaiser filter, not clipped; skipped at 10 000 Hz) and go to ``wg_stoi``.
  Nothing is read back: fp64 [B, 8] on the device as ``stoi_enqueue`` returns it.  A rate the resampler refuses raises
  its WgError before any device work."""
  from . import resample
  up, down, _, _ = resample.resample_plan(sampling_rate, STOI_RATE)
  a = _audio("intelligibility_metrics: audio_a", audio_a)
  b = _audio("intelligibility_metrics: audio_b", audio_b, a.device)
  if a.shape[0] != b.shape[0]:
    raise _lib.WgError(f"intelligibility_metrics: batch sizes differ, {tuple(a.shape)} against {tuple(b.shape)}")
  la = _lengths("intelligibility_metrics: lengths_a", lengths_a, a)
  lb = _lengths("intelligibility_metrics: lengths_b", lengths_b, b)
  longest = resample.out_len(max(a.shape[1], b.shape[1]), up, down)
  if longest > STOI_MAX_PITCH:
    raise _lib.WgError(f"intelligibility_metrics: rows of {longest} samples at 10 kHz are beyond {STOI_MAX_PITCH}")
  with torch.cuda.device(a.device):
    n = torch.minimum(la, lb)                      # a length outside a row stays outside: 0 frames downstream
    n = torch.where((la < 0) | (la > a.shape[1]) | (lb < 0) | (lb > b.shape[1]), torch.zeros_like(n), n)
    if up == down:
      return stoi_enqueue(a, n, b, n)
    xa = resample.resample_enqueue(a, n, sampling_rate, STOI_RATE, pitch=longest)
    xb = resample.resample_enqueue(b, n, sampling_rate, STOI_RATE, pitch=longest)
    n10 = (n.to(torch.int64) * up + (down - 1)).div(down, rounding_mode="floor").to(torch.int32)
    return stoi_enqueue(xa, n10, xb, n10)


def intelligibility_metrics(audio_a: torch.Tensor, lengths_a: Frames, audio_b: torch.Tensor, lengths_b: Frames,
                            sampling_rate=22050) -> List[IntelligibilityMetrics]:
  """``intelligibility_metrics_enqueue`` + one copy to the host + one stream synchronise."""
  return rows_to_intelligibility_metrics(_read_rows(
    intelligibility_metrics_enqueue(audio_a, lengths_a, audio_b, lengths_b, sampling_rate)))


# ------------------------------------------------------------------------------------- STOI / ESTOI with a gradient
def stoi_saved_bytes(B: int, N: int) -> int:
  """Bytes ``stoi_forward_saved`` keeps for the backward besides ``y10k`` itself: the counts, the kept-frame lists and the
  band spectra of both sides (``wg_stoi_saved_bytes``; 0 for a refused geometry)."""
  return int(_lib.load().wg_stoi_saved_bytes(int(B), int(N)))


def stoi_forward_saved(x10k: torch.Tensor, lengths_x: Frames, y10k: torch.Tensor, lengths_y: Frames):
  """``(rows, state)``: the rows of ``stoi_enqueue`` bit for bit (``wg_stoi_forward`` runs the same five launches) and what
  ``stoi_backward_enqueue`` needs: the processed signal as the kernels read it and the saved buffer.  Both sides must have
  one row pitch here.  Enqueue-only."""
  x = _stoi_audio("stoi: x10k", x10k)
  y = _stoi_audio("stoi: y10k", y10k, x.device)
  if x.shape != y.shape:
    raise _lib.WgError(f"stoi with a gradient takes both sides in one shape, got {tuple(x.shape)} and {tuple(y.shape)}")
  lx, ly = _lengths("stoi: lengths_x", lengths_x, x), _lengths("stoi: lengths_y", lengths_y, y)
  B, N = x.shape
  lib = _lib.load()
  with torch.cuda.device(x.device):
    p = _stoi_params(x.device)
    rows = torch.empty((B, N_ROW), dtype=torch.float64, device=x.device)
    saved = torch.empty(lib.wg_stoi_saved_bytes(B, N), dtype=torch.uint8, device=x.device)
    ws = torch.empty(lib.wg_stoi_workspace_bytes(B, N), dtype=torch.uint8, device=x.device)
    _lib.check(lib.wg_stoi_forward(ptr(x), ptr(lx), ptr(y), ptr(ly), B, N, C.byref(p),
                                   ptr(rows), ptr(saved), saved.numel(), ptr(ws), ws.numel(), _args.stream(x.device)))
  return rows, (y.detach(), saved)


def stoi_backward_enqueue(state, g_rows: torch.Tensor) -> torch.Tensor:
  """fp64 ``[B, N]``: the gradient of ``sum_b g_rows[b, 0] STOI_b + g_rows[b, 1] ESTOI_b`` with respect to ``y10k``
  (``wg_stoi_backward``), from the state of ``stoi_forward_saved`` and fp64 ``[B, 2]`` upstream gradients on the device.
  Exact zeros at and behind a pair's common length and in a row without a segment.  Writes to nothing the forward left:
  calling it twice gives the same bits.  Enqueue-only."""
  y, saved = state
  B, N = y.shape
  if not isinstance(g_rows, torch.Tensor) or g_rows.device != y.device or g_rows.dtype != torch.float64 or \
      tuple(g_rows.shape) != (B, 2):
    raise _lib.WgError(f"stoi backward takes the upstream gradients as float64 [{B}, 2] on {y.device}")
  g = g_rows.contiguous()
  lib = _lib.load()
  with torch.cuda.device(y.device):
    p = _stoi_params(y.device)
    d_y = torch.empty((B, N), dtype=torch.float64, device=y.device)
    ws = torch.empty(lib.wg_stoi_backward_workspace_bytes(B, N), dtype=torch.uint8, device=y.device)
    _lib.check(lib.wg_stoi_backward(ptr(y), B, N, C.byref(p), ptr(g), ptr(saved), saved.numel(),
                                    ptr(d_y), ptr(ws), ws.numel(), _args.stream(y.device)))
  return d_y


class _StoiFn(torch.autograd.Function):
  """(x10k, lengths_x, y10k, lengths_y) -> fp64 [B, 2]; the gradient goes to y10k alone, rounded to its fp32 once."""

  @staticmethod
  def forward(ctx, x, lx, y, ly):
    rows, ctx.state = stoi_forward_saved(x, lx, y.detach(), ly)
    return rows[:, :2].clone()

  @staticmethod
  def backward(ctx, g):
    return None, None, stoi_backward_enqueue(ctx.state, g.to(torch.float64)).to(torch.float32), None


def stoi_differentiable(x10k: torch.Tensor, lengths_x: Frames, y10k: torch.Tensor, lengths_y: Frames) -> torch.Tensor:
  """fp64 ``[B, 2]`` on the device: STOI and ESTOI of the pairs (``x10k[b]`` clean, ``y10k[b]`` processed; fp32 ``[B, N]`` at
  10 kHz, one shape), the bits of ``stoi_enqueue``'s first two columns, with a graph back to ``y10k``.  NaN where a pair has
  no segment (its gradient is all zeros).  The energy gate and ``x10k`` are constants: an ``x10k`` that requires grad
  raises WgError.  The gradient follows the definition the metric uses (include/waveglow_amd.h: wg_stoi_backward, with its
  conventions at the points that are not smooth) in fp64 and is rounded to fp32 once.  Without grad mode, or when ``y10k``
  does not require grad, nothing is saved and no graph comes back.  Enqueue-only; no double backward."""
  if isinstance(x10k, torch.Tensor) and x10k.requires_grad:
    raise _lib.WgError("stoi_differentiable: only y10k gets a gradient (the gate runs on the clean side); detach x10k")
  x = _stoi_audio("stoi: x10k", x10k)
  y = _stoi_audio("stoi: y10k", y10k, x.device)
  if x.shape != y.shape:
    raise _lib.WgError(f"stoi_differentiable takes both sides in one shape, got {tuple(x.shape)} and {tuple(y.shape)}")
  lx, ly = _lengths("stoi: lengths_x", lengths_x, x), _lengths("stoi: lengths_y", lengths_y, y)
  if torch.is_grad_enabled() and y10k.requires_grad:
    return _StoiFn.apply(x, lx, y10k, ly)
  return stoi_enqueue(x, lx, y, ly)[:, :2].clone()
