"""Per-utterance likelihood of recorded audio under a WaveGlow model, on the device.

WaveGlow is a normalising flow: the quantity it is trained on, the negative log-likelihood of audio given its mel
(``WaveGlowLoss``, src/waveglow/train.py:31-45), is also the most direct figure of merit of a checkpoint.  The reference
logs it as one scalar of a dense batch; here every utterance of a batch of different lengths gets its own, with a track per
mel frame: the no-grad forward with per-utterance frame counts (``wg_forward`` with ``frames``,
src/waveglow/model.py:178-221) and a two-level fp64 reduction (``wg_nll``).  The definitions are stated in
include/waveglow_amd.h and DESIGN.md section 7.

Always without a hipGraph and without autograd: this is for evaluation.  Everything is enqueued on the current stream;
only ``log_likelihood`` copies to the host (once).  No CPU fallback.
"""
from __future__ import annotations

import ctypes as C
from typing import List, NamedTuple, Optional, Sequence, Tuple, Union

import torch

from . import _args, _lib

N_ROW = 8               # fp64 values per utterance (include/waveglow_amd.h: wg_nll)
NLL, BITS_PER_SAMPLE, SUM_Z2, SUM_LOG_S, LOG_DET, SAMPLES, Z_MEAN, Z_VAR = range(8)
FRAME_SAMPLES = 256     # samples of one mel frame: the unit of a length

Frames = Union[None, Sequence[int], torch.Tensor]


class Likelihood(NamedTuple):
  nll: float              # nats per sample: WaveGlowLoss of this utterance alone
  bits_per_sample: float  # (nll + ln(2 pi sigma^2) / 2) / ln 2: with the constant the training loss drops
  samples: int            # 8 * columns scored
  z_mean: float           # of the utterance's z; a fitted model gives 0
  z_var: float            # ... and sigma^2
  sum_z2: float
  sum_log_s: float
  log_det: float          # columns * sum_k log|det W_k|


def rows_to_likelihoods(rows: torch.Tensor) -> List[Likelihood]:
  """Host rows [B, 8] of ``log_likelihood_enqueue`` as tuples."""
  out = []
  for r in rows.tolist():
    out.append(Likelihood(nll=r[NLL], bits_per_sample=r[BITS_PER_SAMPLE], samples=int(r[SAMPLES]), z_mean=r[Z_MEAN],
                          z_var=r[Z_VAR], sum_z2=r[SUM_Z2], sum_log_s=r[SUM_LOG_S], log_det=r[LOG_DET]))
  return out


def _inputs(model, mel, audio) -> None:
  for name, t, ndim in (("mel [B, n_mel, T]", mel, 3), ("audio [B, S]", audio, 2)):
    _args.tensor(f"log_likelihood: {name}", t, dtypes=(torch.float32, torch.float16), ndim=ndim)
  if mel.shape[0] != audio.shape[0] or mel.shape[0] < 1:
    raise _lib.WgError(f"log_likelihood: mel [B, n_mel, T] and audio [B, S] expected, got {tuple(mel.shape)} and "
                       f"{tuple(audio.shape)}")
  if mel.dtype != audio.dtype or mel.device != audio.device:
    raise _lib.WgError("log_likelihood: mel and audio must share dtype and device")


def _frames(frames: Frames, mel: torch.Tensor, audio: torch.Tensor) -> torch.Tensor:
  """int32 [B] on the device.  Host counts are range-checked here, before any launch; a device tensor is trusted (the
  kernels give an utterance with a count outside the range zeros, and read nothing outside the buffers)."""
  B, _, T = mel.shape
  dev, host = _args.counts("log_likelihood: frame counts", frames, B, 1, T, device=mel.device, allow_device=True)
  if host is not None and FRAME_SAMPLES * max(host) > audio.shape[1]:
    raise _lib.WgError(f"log_likelihood: frame counts with {FRAME_SAMPLES} * frames <= {audio.shape[1]} samples expected, "
                       f"got {host}")
  return dev


def _forward(model, mel: torch.Tensor, audio: torch.Tensor, frames: Frames):
  """The no-grad forward at fp32 outputs: ``(engine, z [B, 8, L], [log_s_k [B, h_k, L]], frames_dev or None)``.
  Dense: the batch on ``S - S % 8`` samples as ``WaveGlow.forward`` crops it.  With counts: both inputs are brought
  to the pitch ``min(T, S // 256)`` frames and ``wg_forward`` takes them as ``frames``."""
  _inputs(model, mel, audio)
  if frames is not None:
    fr = _frames(frames, mel, audio)          # refused before any launch
  eng = model._get_engine(mel.device)
  if frames is None:
    S = audio.shape[1] - audio.shape[1] % model.n_group
    T = mel.shape[2]
    if S < model.n_group or (T - 1) * 256 + 1024 < S:       # model.py:187
      raise _lib.WgError(f"log_likelihood: {audio.shape[1]} samples do not fit under {T} mel frames")
    fr = None
  else:
    T = min(mel.shape[2], audio.shape[1] // FRAME_SAMPLES)
    if T < 1:
      raise _lib.WgError(f"log_likelihood: {audio.shape[1]} samples are less than one frame of {FRAME_SAMPLES}")
    S = FRAME_SAMPLES * T
    mel = mel[:, :, :T]
  with torch.cuda.device(mel.device):
    z, log_s, _ = eng.run_forward(eng.pad_mel_input(mel).contiguous(), fr, audio[:, :S].contiguous(), S)
  return eng, z, log_s, fr


def forward_ragged(model, mel: torch.Tensor, audio: torch.Tensor, frames: Frames) -> Tuple[torch.Tensor, List[torch.Tensor]]:
  """``(z, [log_s_k])`` of the no-grad ``WaveGlow.forward`` for utterances of different lengths, in the dtype of the
  inputs: utterance b is ``audio[b, :256 * frames[b]]`` under ``mel[b, :, :frames[b]]`` and gets, bit for bit, what
  ``model((mel_b, audio_b))`` gives it alone; behind ``32 * frames[b]`` columns everything is 0.  Mel and audio behind an
  utterance are never used."""
  if frames is None:
    raise _lib.WgError("forward_ragged: frame counts expected (the dense batch is WaveGlow.forward)")
  with torch.no_grad():
    _, z, log_s, _ = _forward(model, mel, audio, frames)
  if mel.dtype != torch.float32:
    z, log_s = z.to(mel.dtype), [t.to(mel.dtype) for t in log_s]
  return z, log_s


def nll_enqueue(eng, z: torch.Tensor, log_s: List[torch.Tensor], frames_dev: Optional[torch.Tensor], sigma: float,
                per_frame: bool = False):
  """``wg_nll`` on fp32 ``z`` [B, 8, L] and ``log_s`` of the engine's model: fp64 rows [B, 8] on the device, and with
  ``per_frame`` the track [B, ceil(L / 32)] (None otherwise)."""
  sigma = float(sigma)
  if not sigma > 0.0 or sigma == float("inf"):
    raise _lib.WgError(f"log_likelihood: sigma > 0 expected, got {sigma}")
  B, _, L = z.shape
  dev = z.device
  nbytes = int(eng.lib.wg_nll_workspace_bytes(eng.handle, B, L))
  if nbytes == 0:
    raise _lib.WgError(eng.lib.wg_last_error().decode())
  rows = torch.empty((B, N_ROW), dtype=torch.float64, device=dev)
  track = torch.empty((B, (L + 31) // 32), dtype=torch.float64, device=dev) if per_frame else None
  ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
  ls = (C.c_void_p * len(log_s))(*[t.data_ptr() for t in log_s])
  with torch.cuda.device(dev):
    _lib.check(eng.lib.wg_nll(eng.handle, _args.ptr(z), ls, _args.ptr(frames_dev), sigma, B, L, _args.ptr(rows),
                              _args.ptr(track), _args.ptr(ws), ws.numel(), _args.stream(dev)))
  return rows, track


def log_likelihood_enqueue(model, mel: torch.Tensor, audio: torch.Tensor, frames: Frames = None,
                           sigma: Optional[float] = None, per_frame: bool = False):
  """fp64 rows [B, 8] on the device (``N_ROW`` figures per utterance, see ``Likelihood``), nothing read back; with
  ``per_frame`` also the track fp64 [B, n_frames] (NaN behind an utterance), as a pair."""
  sigma = 1.0 if sigma is None else sigma
  if not float(sigma) > 0.0:
    raise _lib.WgError(f"log_likelihood: sigma > 0 expected, got {sigma}")
  with torch.no_grad():
    eng, z, log_s, fr = _forward(model, mel, audio, frames)
    rows, track = nll_enqueue(eng, z, log_s, fr, sigma, per_frame)
  return (rows, track) if per_frame else rows


def log_likelihood(model, mel: torch.Tensor, audio: torch.Tensor, frames: Frames = None, sigma: Optional[float] = None,
                   per_frame: bool = False):
  """One ``Likelihood`` per utterance (one device-to-host copy); with ``per_frame`` a pair with the track, which stays
  on the device.  ``frames``: B integers as ``_args.counts`` takes them (a list, a tuple or a 1-D CPU tensor of an
  integer dtype; a float or a bool entry raises WgError), the mel-frame counts, each in ``[1, mel.shape[2]]`` with ``256
  * f <= audio.shape[1]`` (``WgError`` before any launch otherwise), or an int32 tensor ``[B]`` on the device, which is
  trusted and never read on the host; None scores the dense batch on ``S - S % 8`` samples as ``forward`` crops it.
  ``sigma`` None: 1.0, the ``WaveGlowLoss`` default."""
  res = log_likelihood_enqueue(model, mel, audio, frames, sigma, per_frame)
  rows = rows_to_likelihoods((res[0] if per_frame else res).cpu())
  return (rows, res[1]) if per_frame else rows
