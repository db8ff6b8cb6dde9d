"""Streaming synthesis: audio in chunks while the mel is still arriving, with the bits of whole-utterance synthesis.

WaveGlow's flows are not causal, but their receptive field is finite: with ``R = n_flows * (2^n_layers - 1)`` columns
(kernel size 3; one column is ``n_group`` samples, 32 columns per mel frame) the audio of frames ``[s, e)`` reads

* mel frames ``[s - ceil(R / 32) - 3, e + ceil(R / 32))`` (the 3: the transposed-conv upsample, 1024 / 256 - 1),
* noise columns ``[32 s - R, 32 e + R)`` of ``z_init`` and every ``z_early``,

and the denoiser reads 3 more frames of raw audio on either side (``filter_length / hop - 1``).  A chunk synthesised
inside a window that carries this halo on both sides therefore sees exactly the inputs it sees in the whole utterance;
the library's ragged entry points give every utterance of a batch the bits of its own call wherever its columns lie, and
treat the padding behind a count as the end of the sequence.  So the windows of a step run as a ragged batch
(``wg_infer``, ``wg_stft_denoise`` with counts) and the interiors, concatenated, ARE the whole-utterance audio -- no
overlap-add, no seams.  Every chunk recomputes its halo: a step over a ``C``-frame chunk does the flow's work for
``C + Hl + Hr`` frames, and a chunk can only leave once ``Hr`` frames behind it have arrived (the algorithmic look-ahead).

This module holds the halo arithmetic and the chunk planner (pure functions, no GPU), the session object, and the step
that advances many sessions in one launch sequence; ``Synthesizer.open_stream`` / ``stream_step`` / ``infer_stream`` are
the public surface.  No CPU fallback.
"""
from __future__ import annotations

import ctypes as C
from dataclasses import dataclass
from typing import List, Optional, Sequence, Tuple

import numpy as np
import torch

from . import _args, _lib

# columns of the statistics, one row of 8 floats per chunk (include/waveglow_amd.h: wg_stream_emit)
RAW_MIN, RAW_MAX, DEN_MIN, DEN_MAX, CLIPPED, NON_FINITE = range(6)
N_STATS = 8
MAX_EARLY = 8                      # WG_STREAM_MAX_EARLY
UPSAMPLE_KERNEL, UPSAMPLE_STRIDE = 1024, 256      # model.py:148-149, fixed in the library (wg_config)


class WgStreamWindow(C.Structure):
  _fields_ = [("mel", C.c_void_p), ("z_init", C.c_void_p), ("z_early", C.c_void_p * MAX_EARLY),
              ("mel_pitch", C.c_int64), ("noise_pitch", C.c_int64), ("start", C.c_int32), ("count", C.c_int32)]


class WgStreamCrop(C.Structure):
  _fields_ = [("raw", C.c_void_p), ("denoised", C.c_void_p), ("offset", C.c_int32), ("count", C.c_int32),
              ("gain", C.c_float), ("reserved", C.c_int32)]


# ------------------------------------------------------------------------------------------------ halo and planner
def receptive_columns(hparams) -> int:
  """R: columns the flow reads on either side of a column -- every flow's WN adds ``(k - 1) / 2 * (2^n_layers - 1)``."""
  return hparams.n_flows * ((hparams.kernel_size - 1) // 2) * (2 ** hparams.n_layers - 1)


def stream_halo(hparams) -> Tuple[int, int, int, int]:
  """``(mel_left, mel_right, noise_cols, denoise_frames)``: the mel frames in front of and behind a chunk, and the noise
  columns on either side, that its audio reads; and the frames of raw audio on either side that the denoiser reads."""
  cpf = UPSAMPLE_STRIDE // hparams.n_group
  R = receptive_columns(hparams)
  frames = -(-R // cpf)
  return frames + UPSAMPLE_KERNEL // UPSAMPLE_STRIDE - 1, frames, R, hparams.filter_length // hparams.hop_length - 1


def halo_frames(hparams, denoise: bool) -> Tuple[int, int]:
  """``(Hl, Hr)``: the window of a chunk in frames, on the left and on the right.  Noise travels with whole frames, so the
  window's noise columns cover ``noise_cols`` (``32 * mel_right >= R``)."""
  ml, mr, _, df = stream_halo(hparams)
  return (ml + df, mr + df) if denoise else (ml, mr)


@dataclass(frozen=True)
class ChunkPlan:
  index: int
  w0: int            # the window [w0, w1) in frames
  w1: int
  offset: int        # first sample of the chunk inside the window's audio
  count: int         # samples of the chunk
  start_sample: int  # first sample of the chunk in the utterance
  final: bool


def ready_chunks(frames: int, chunk_frames: int, Hr: int, closed: bool) -> int:
  """Chunks of a stream that can be emitted with ``frames`` frames pushed: chunk j as soon as frames up to
  ``(j + 1) C + Hr`` are there; all ``ceil(T / C)`` once the stream is closed."""
  if closed:
    return -(-frames // chunk_frames)
  return max(0, (frames - Hr) // chunk_frames)


def plan_chunk(j: int, frames: int, chunk_frames: int, Hl: int, Hr: int, closed: bool) -> Optional[ChunkPlan]:
  """Chunk ``j`` of a stream with ``frames`` frames pushed (all of them when ``closed``), or None when it cannot be
  emitted yet.  It covers frames ``[j C, min((j + 1) C, T))`` inside the window ``[max(0, j C - Hl), min(T, (j + 1) C +
  Hr))``.  A chunk that is ready before the end is known uses exactly the right edge ``(j + 1) C + Hr``, not whatever more
  has arrived -- the window, and with it the launch geometry, does not depend on how the pushes fell."""
  Cf = chunk_frames
  if j < 0 or j >= ready_chunks(frames, Cf, Hr, closed):
    return None
  s = j * Cf
  if frames >= (j + 1) * Cf + Hr:
    e, w1 = (j + 1) * Cf, (j + 1) * Cf + Hr
  else:                                    # closed, and the end of the utterance is inside the halo or the chunk
    e, w1 = min((j + 1) * Cf, frames), frames
  w0 = max(0, s - Hl)
  return ChunkPlan(j, w0, w1, UPSAMPLE_STRIDE * (s - w0), UPSAMPLE_STRIDE * (e - s), UPSAMPLE_STRIDE * s,
                   closed and e == frames)


def plan_stream(frames: int, chunk_frames: int, Hl: int, Hr: int, closed: bool = True) -> List[ChunkPlan]:
  """Every chunk that can be emitted, in order."""
  return [plan_chunk(j, frames, chunk_frames, Hl, Hr, closed)
          for j in range(ready_chunks(frames, chunk_frames, Hr, closed))]


# ------------------------------------------------------------------------------------------------ the two kernels
def _io(dtype) -> int:
  if dtype == torch.float32:
    return _lib.WG_F32
  if dtype == torch.float16:
    return _lib.WG_F16
  raise _lib.WgError(f"unsupported dtype {dtype} (float32 or float16)")


def _upload(device, raw: bytes) -> torch.Tensor:
  """A small table on the device (the tests' way; ``stream_step`` sends its tables through its pinned ring)."""
  return torch.frombuffer(bytearray(raw), dtype=torch.uint8).to(device)


def pack_windows(windows, cols_per_frame: int = 32) -> bytes:
  """The table of ``wg_stream_gather``: ``windows`` is a sequence of ``(mel [n_mel, cap], z_init [1, n_rem, Lcap],
  [z_early [1, n_early, Lcap], ...], start, count)``; every window is checked against its buffers here, on the host."""
  rows = (WgStreamWindow * len(windows))()
  for r, (mel, z_init, z_early, start, count) in zip(rows, windows):
    if start < 0 or count < 0 or start + count > mel.shape[-1]:
      raise _lib.WgError(f"stream gather: window [{start}, {start + count}) outside a mel of {mel.shape[-1]} frames")
    if cols_per_frame * (start + count) > z_init.shape[-1]:
      raise _lib.WgError(f"stream gather: window [{start}, {start + count}) outside a noise of {z_init.shape[-1]} columns")
    if len(z_early) > MAX_EARLY:
      raise _lib.WgError(f"stream gather: at most {MAX_EARLY} early-noise tensors")
    for t in (mel, z_init, *z_early):
      if t.stride(-1) != 1 or (t.dim() == 3 and t.shape[0] != 1):
        raise _lib.WgError("stream gather: sources are [rows, pitch] with unit column stride")
    r.mel, r.mel_pitch = mel.data_ptr(), mel.stride(-2)
    r.z_init, r.noise_pitch = z_init.data_ptr(), z_init.stride(-2)
    for i, z in enumerate(z_early):
      if z.stride(-2) != z_init.stride(-2) or z.shape[-1] != z_init.shape[-1]:
        raise _lib.WgError("stream gather: the noise tensors of a stream share one pitch")
      r.z_early[i] = z.data_ptr()
    r.start, r.count = int(start), int(count)
  return bytes(rows)


def gather_launch(table_ptr: int, B: int, n_mel: int, n_mel_out: int, n_rem: int, n_early: int, n_early_size: int,
                  w_max: int, cpf: int, dtype, device, out=None):
  """One ``wg_stream_gather`` launch on the current stream from a table already on the device.  Returns ``(mel [B,
  n_mel_out, w_max], z_init [B, n_rem, cpf w_max], [z_early [B, n_early_size, cpf w_max], ...])`` -- ``out`` if given."""
  if out is None:
    # the early tensors are slices of one allocation: one allocator call however many there are
    ze = torch.empty((max(n_early, 1), B, n_early_size, cpf * w_max), dtype=dtype, device=device)
    out = (torch.empty((B, n_mel_out, w_max), dtype=dtype, device=device),
           torch.empty((B, n_rem, cpf * w_max), dtype=dtype, device=device), [ze[i] for i in range(n_early)])
  mel, z_init, z_early = out
  for t, shape in ((mel, (B, n_mel_out, w_max)), (z_init, (B, n_rem, cpf * w_max)),
                   *((z, (B, n_early_size, cpf * w_max)) for z in z_early)):
    if tuple(t.shape) != shape or t.dtype != dtype or not t.is_contiguous() or t.device != torch.device(device):
      raise _lib.WgError(f"stream gather: an output is not a contiguous {dtype} tensor {shape} on {device}")
  ze = (C.c_void_p * max(1, n_early))(*[z.data_ptr() for z in z_early])
  _lib.check(_lib.load().wg_stream_gather(table_ptr, _args.ptr(mel), _args.ptr(z_init), ze, n_early, B, n_mel, n_mel_out,
                                          n_rem, n_early_size, w_max, cpf, _io(dtype), _args.stream(device)))
  return mel, z_init, list(z_early)


def gather_enqueue(windows, w_max: int, *, n_mel_out: Optional[int] = None, cols_per_frame: int = 32, out=None):
  """``wg_stream_gather`` on the current stream: the padded batch tensors of ``windows`` (see ``pack_windows``) at pitch
  ``w_max`` frames, zeros behind every count.  The table goes up in one small copy."""
  mel, z_init, z_early = windows[0][:3]
  if mel.device.type != "cuda":
    raise _lib.WgError("stream gather runs on the GPU library only")
  for m, zi, ze, _, count in windows:
    if count > w_max:
      raise _lib.WgError(f"stream gather: a window of {count} frames at pitch {w_max}")
    if any(t.device != mel.device or t.dtype != mel.dtype for t in (m, zi, *ze)) or len(ze) != len(z_early):
      raise _lib.WgError("stream gather: the sources of a batch share device, dtype and layout")
  table = _upload(mel.device, pack_windows(windows, cols_per_frame))
  n_es = z_early[0].shape[-2] if z_early else 1
  return gather_launch(table.data_ptr(), len(windows), mel.shape[-2], n_mel_out or mel.shape[-2], z_init.shape[-2],
                       len(z_early), n_es, w_max, cols_per_frame, mel.dtype, mel.device, out)


def pack_crops(crops) -> bytes:
  """The table of ``wg_stream_emit``: ``crops`` is a sequence of ``(raw, denoised, offset, count, gain)`` with ``raw`` /
  ``denoised`` contiguous fp32 rows of window audio; every crop is checked against its row here, on the host."""
  rows = (WgStreamCrop * len(crops))()
  for r, (raw, den, offset, count, gain) in zip(rows, crops):
    for t in (raw, den):
      if t.dtype != torch.float32 or t.dim() != 1 or t.stride(0) != 1:
        raise _lib.WgError("stream emit takes contiguous float32 rows")
      if offset < 0 or count < 0 or offset + count > t.numel():
        raise _lib.WgError(f"stream emit: crop [{offset}, {offset + count}) outside a row of {t.numel()} samples")
    r.raw, r.denoised, r.offset, r.count, r.gain, r.reserved = raw.data_ptr(), den.data_ptr(), offset, count, gain, 0
  return bytes(rows)


def emit_launch(table_ptr: int, B: int, n_max: int, device) -> torch.Tensor:
  """One ``wg_stream_emit`` launch on the current stream from a table already on the device.  Returns one uint8 device
  buffer: the int16 samples [B, n_max], then the statistics [B, 8] fp32 -- what ``emit_read`` takes apart on the host."""
  out = torch.empty(2 * B * n_max + 4 * N_STATS * B, dtype=torch.uint8, device=device)
  _lib.check(_lib.load().wg_stream_emit(table_ptr, _args.ptr(out), out.data_ptr() + 2 * B * n_max, B, n_max,
                                        _args.stream(device)))
  return out


def emit_enqueue(crops, n_max: int) -> torch.Tensor:
  """``wg_stream_emit`` on the current stream for ``crops`` (see ``pack_crops``) at pitch ``n_max`` samples (a multiple
  of 8, no crop longer)."""
  dev = crops[0][0].device
  if dev.type != "cuda" or any(t.device != dev for c in crops for t in c[:2]):
    raise _lib.WgError("stream emit runs on the GPU library only: all audio on one GPU")
  if n_max < 8 or n_max % 8 or any(c[3] > n_max for c in crops):
    raise _lib.WgError(f"stream emit: pitch {n_max} must be a multiple of 8 and hold every crop")
  table = _upload(dev, pack_crops(crops))
  return emit_launch(table.data_ptr(), len(crops), n_max, dev)


def emit_read(host: torch.Tensor, B: int, n_max: int):
  """(pcm int16 [B, n_max], stats fp32 [B, 8]) as numpy views of the host copy of ``emit_launch``'s buffer."""
  buf = host.numpy()
  pcm = buf[:2 * B * n_max].view(np.int16).reshape(B, n_max)
  stats = buf[2 * B * n_max:2 * B * n_max + 4 * N_STATS * B].view(np.float32).reshape(B, N_STATS)
  return pcm, stats


# ------------------------------------------------------------------------------------------------ session
@dataclass
class StreamChunk:
  """One chunk of a stream.  ``pcm``: int16 numpy, ``convert_wav(np.clip(denoised * gain, -1, 1), np.int16)`` -- NOT
  peak-normalised, a stream does not know its utterance's peak; or, from ``stream_step(pcm=False)``, ``raw`` /
  ``denoised``: fp32 device tensors (the same tensor without a denoiser), and the statistics are None."""
  pcm: Optional[np.ndarray]
  raw: Optional[torch.Tensor]
  denoised: Optional[torch.Tensor]
  start_sample: int
  sampling_rate: int
  raw_min: Optional[float]
  raw_max: Optional[float]
  clipped: Optional[int]       # samples the clip to [-1, 1] changed
  final: bool


class StreamSession:
  """One utterance being synthesised in chunks (``Synthesizer.open_stream``).  Holds the stream's mel on the device,
  ``[n_mel, capacity]`` with the capacity growing geometrically, and its noise in the layouts ``infer_with_noise`` takes.

  Noise, two modes:

  * ``total_frames=T`` at open: the noise of the whole utterance is drawn once, exactly as ``Synthesizer.infer`` draws
    it -- ``init_global_seeds(seed)`` (which resets the GLOBAL generators, as every ``infer`` call does), then
    ``[1, n_rem, 32 T]``, then the early tensors in the reference's order.  The stream reproduces
    ``Synthesizer.infer(mel, seed=seed)``.
  * open-ended: every ``push`` draws the noise of its new columns from a generator of the session's own, seeded with
    ``seed``; the global generators are not touched.  The draws depend on how the pushes fell, so the stream reproduces
    ``model.infer_with_noise(mel, *session.noise())``, not ``infer``.
  """

  def __init__(self, synth, *, sigma, denoiser_strength, seed, chunk_frames, total_frames, gain, dtype):
    model, hp = synth.model, synth.hparams
    if int(chunk_frames) < 1:
      raise _lib.WgError(f"chunk_frames={chunk_frames}: a chunk has at least one frame")
    if total_frames is not None and int(total_frames) < 1:
      raise _lib.WgError(f"total_frames={total_frames}: a stream has at least one frame")
    _io(dtype)
    self.synth, self.device, self.dtype = synth, synth.device, dtype
    self.sigma, self.strength, self.seed, self.gain = float(sigma), float(denoiser_strength), int(seed), float(gain)
    self.chunk_frames = int(chunk_frames)
    self.total_frames = None if total_frames is None else int(total_frames)
    self.denoise = self.strength > 0
    self.Hl, self.Hr = halo_frames(hp, self.denoise)
    self.n_mel, self.cpf = hp.n_mel_channels, UPSAMPLE_STRIDE // hp.n_group
    self.n_rem, self.n_early_size, self.n_early = model.n_remaining_channels, model.n_early_size, model.n_early_flows()
    if self.n_early > MAX_EARLY:
      raise _lib.WgError(f"streaming takes at most {MAX_EARLY} early-output flows, the model has {self.n_early}")
    self._check_length(self.total_frames)
    self.frames = 0              # mel frames pushed
    self.closed = False
    self.next_chunk = 0          # index of the next chunk to emit
    self.emitted_frames = 0
    self.name = f"stream {id(self):#x}"
    cap = self.total_frames if self.total_frames is not None else 64
    self._mel = torch.empty((self.n_mel, cap), dtype=dtype, device=self.device)
    if self.total_frames is not None:
      from .synthesizer import init_global_seeds
      init_global_seeds(self.seed)                                                      # synthesizer.py:56
      L = self.cpf * cap
      draw = lambda c: torch.empty((1, c, L), dtype=dtype, device=self.device).normal_()
      self._z_init = draw(self.n_rem)                                                   # model.py:243
      self._z_early = [draw(self.n_early_size) for _ in range(self.n_early)]            # model.py:266-268
      self._gen = None
    else:
      self._gen = torch.Generator(device=self.device)
      self._gen.manual_seed(self.seed)
      self._z_init = torch.empty((1, self.n_rem, self.cpf * cap), dtype=dtype, device=self.device)
      self._z_early = [torch.empty((1, self.n_early_size, self.cpf * cap), dtype=dtype, device=self.device)
                       for _ in range(self.n_early)]

  def _check_length(self, T):
    if T is not None and self.denoise and T < 4:
      raise _lib.WgError(f"a stream of {T} frames with the denoiser on: the denoiser takes at least 4 frames "
                         "(1024 samples), as the whole-utterance path; denoiser_strength=0 takes one frame")

  def _grow(self, need: int) -> None:
    cap = self._mel.shape[1]
    if need <= cap:
      return
    while cap < need:
      cap *= 2
    def grown(old, n_valid, width):
      new = torch.empty(old.shape[:-1] + (width,), dtype=old.dtype, device=old.device)
      new[..., :n_valid] = old[..., :n_valid]
      return new
    self._mel = grown(self._mel, self.frames, cap)
    self._z_init = grown(self._z_init, self.cpf * self.frames, self.cpf * cap)
    self._z_early = [grown(z, self.cpf * self.frames, self.cpf * cap) for z in self._z_early]

  def push(self, mel_chunk: torch.Tensor) -> None:
    """Append ``[n_mel, t]`` or ``[1, n_mel, t]`` (``t >= 0``) mel frames, in the session's dtype, from the host or from
    the session's device.  Refused with WgError before anything is copied: a push after ``close()``, past
    ``total_frames``, or of the wrong channel count, dtype or device."""
    if self.closed:
      raise _lib.WgError(f"{self.name}: push after close()")
    m = mel_chunk
    if not torch.is_tensor(m) or m.dim() not in (2, 3) or (m.dim() == 3 and m.shape[0] != 1):
      raise _lib.WgError(f"{self.name}: a mel chunk is a tensor [n_mel, t] or [1, n_mel, t]")
    if m.dim() == 3:
      m = m[0]
    if m.shape[0] != self.n_mel:
      raise _lib.WgError(f"{self.name}: a mel chunk of {m.shape[0]} channels, the model takes {self.n_mel}")
    if m.dtype != self.dtype:
      raise _lib.WgError(f"{self.name}: a mel chunk of dtype {m.dtype}, the stream was opened with {self.dtype}")
    if m.device.type != "cpu" and m.device != self.device:
      raise _lib.WgError(f"{self.name}: a mel chunk on {m.device}, the stream lives on {self.device}")
    t = int(m.shape[1])
    if self.total_frames is not None and self.frames + t > self.total_frames:
      raise _lib.WgError(f"{self.name}: {self.frames + t} frames pushed, the stream was opened with total_frames="
                         f"{self.total_frames}")
    if t == 0:
      return
    self._grow(self.frames + t)
    self._mel[:, self.frames:self.frames + t].copy_(m, non_blocking=True)
    if self._gen is not None:
      lo, n = self.cpf * self.frames, self.cpf * t
      for z in (self._z_init, *self._z_early):                                          # the reference's order per push
        z[0, :, lo:lo + n] = torch.empty((z.shape[1], n), dtype=self.dtype, device=self.device).normal_(generator=self._gen)
    self.frames += t

  def close(self) -> None:
    """No more frames: the rest of the stream becomes ready.  WgError for a stream that ends short of ``total_frames``,
    without a frame, or (denoiser on) with fewer than 4 frames."""
    if self.closed:
      return
    if self.total_frames is not None and self.frames != self.total_frames:
      raise _lib.WgError(f"{self.name}: closed at {self.frames} frames, opened with total_frames={self.total_frames}")
    if self.frames < 1:
      raise _lib.WgError(f"{self.name}: closed without a frame")
    self._check_length(self.frames)
    self.closed = True

  @property
  def ready(self) -> int:
    """Chunks that can be emitted now."""
    return ready_chunks(self.frames, self.chunk_frames, self.Hr, self.closed) - self.next_chunk

  @property
  def finished(self) -> bool:
    return self.closed and self.ready == 0

  def next_plan(self) -> Optional[ChunkPlan]:
    return plan_chunk(self.next_chunk, self.frames, self.chunk_frames, self.Hl, self.Hr, self.closed)

  def noise(self):
    """``(z_init, z_early)`` drawn so far, ``[1, c, 32 * frames]`` each, as ``infer_with_noise`` takes them."""
    L = self.cpf * (self.total_frames if self.total_frames is not None else self.frames)
    return self._z_init[:, :, :L], [z[:, :, :L] for z in self._z_early]

  def _advance(self, plan: ChunkPlan) -> None:
    self.next_chunk = plan.index + 1
    self.emitted_frames += plan.count // UPSAMPLE_STRIDE


# ------------------------------------------------------------------------------------------------ the step
class _PinnedRing:
  """Pinned staging buffers for the step's small uploads and its one download: a rotating set, each guarded by an event
  recorded behind its copy, so a buffer is never rewritten while a copy out of or into it is pending."""

  def __init__(self, n: int = 4):
    self.bufs: List[Optional[torch.Tensor]] = [None] * n
    self.events: List[Optional[torch.cuda.Event]] = [None] * n
    self.next = 0

  def take(self, nbytes: int) -> Tuple[torch.Tensor, int]:
    i = self.next
    self.next = (i + 1) % len(self.bufs)
    if self.events[i] is not None:
      self.events[i].synchronize()
    if self.bufs[i] is None or self.bufs[i].numel() < nbytes:
      self.bufs[i] = torch.empty(max(nbytes, 4096), dtype=torch.uint8, pin_memory=True)
    return self.bufs[i][:nbytes], i

  def guard(self, i: int, stream) -> None:
    if self.events[i] is None:
      self.events[i] = torch.cuda.Event()
    self.events[i].record(stream)


def stream_step(synth, sessions: Sequence[StreamSession], pcm: bool = True) -> list:
  """``Synthesizer.stream_step``: every session with a ready chunk advances by one chunk, all of them in one launch
  sequence on the current stream --

  1. one table (gather rows, crop rows, frame and sample counts) through a pinned buffer,
  2. one ``wg_stream_gather`` launch,
  3. one ``wg_infer`` sequence over the windows as a ragged batch at the fixed pitch ``C + Hl + Hr``,
  4. one ``wg_stft_denoise`` call with lengths over the sessions with a strength above 0 (one strength per step),
  5. one ``wg_stream_emit`` launch,
  6. one pinned copy and one stream synchronise.

  With ``pcm=False`` steps 5 and 6 are left out and nothing is synchronised."""
  out: list = [None] * len(sessions)
  if len({id(s) for s in sessions}) != len(sessions):
    raise _lib.WgError("stream_step: a session is listed twice")
  act = [(i, s, s.next_plan()) for i, s in enumerate(sessions) if s.ready > 0]
  if not act:
    return out
  for _, s, _ in act:
    if s.synth is not synth:
      raise _lib.WgError(f"{s.name} belongs to another Synthesizer")
  if len({s.dtype for _, s, _ in act}) != 1 or len({s.sigma for _, s, _ in act}) != 1:
    raise _lib.WgError("stream_step: the sessions of one step share dtype and sigma")
  strengths = {s.strength for _, s, _ in act if s.denoise}
  if len(strengths) > 1:
    raise _lib.WgError(f"stream_step: one denoiser strength per step, got {sorted(strengths)}")
  act.sort(key=lambda a: not a[1].denoise)               # the denoised rows first: the denoiser takes the leading rows
  model, dev, hp = synth.model, synth.device, synth.hparams
  s0 = act[0][1]
  dtype, cpf = s0.dtype, s0.cpf
  B, Bd = len(act), sum(1 for _, s, _ in act if s.denoise)
  w_max = max(s.chunk_frames + s.Hl + s.Hr for _, s, _ in act)
  n_max = UPSAMPLE_STRIDE * max(s.chunk_frames for _, s, _ in act)
  N = UPSAMPLE_STRIDE * w_max
  eng = model._get_engine(dev)
  # everything the table names is allocated first (no launch), so that ONE table holds both kernels' rows
  ze_all = torch.empty((max(s0.n_early, 1), B, s0.n_early_size, cpf * w_max), dtype=dtype, device=dev)
  bufs = (torch.empty((B, eng.mel_width, w_max), dtype=dtype, device=dev),
          torch.empty((B, s0.n_rem, cpf * w_max), dtype=dtype, device=dev), [ze_all[i] for i in range(s0.n_early)])
  audio = torch.empty((B, N), dtype=dtype, device=dev)
  raw = audio if dtype == torch.float32 else torch.empty((B, N), dtype=torch.float32, device=dev)
  den = torch.empty((Bd, N), dtype=torch.float32, device=dev) if Bd else None
  windows, crops, frames, lengths = [], [], [], []
  for b, (_, s, p) in enumerate(act):
    windows.append((s._mel, s._z_init, s._z_early, p.w0, p.w1 - p.w0))
    crops.append((raw[b], den[b] if b < Bd else raw[b], p.offset, p.count, s.gain))
    frames.append(p.w1 - p.w0)
    lengths.append(UPSAMPLE_STRIDE * (p.w1 - p.w0))
  parts = [pack_windows(windows, cpf), pack_crops(crops), np.asarray(frames, dtype=np.int32).tobytes(),
           np.asarray(lengths[:Bd], dtype=np.int32).tobytes()]
  offs = np.cumsum([0] + [-(-len(x) // 16) * 16 for x in parts])
  ring = getattr(synth, "_stream_ring", None)
  if ring is None:
    ring = synth._stream_ring = _PinnedRing()
  stream = torch.cuda.current_stream(dev)
  host, slot = ring.take(int(offs[-1]))
  hb = host.numpy()
  for o, x in zip(offs, parts):
    hb[o:o + len(x)] = np.frombuffer(x, dtype=np.uint8)
  table = torch.empty(int(offs[-1]), dtype=torch.uint8, device=dev)
  with torch.no_grad():
    table.copy_(host, non_blocking=True)
    ring.guard(slot, stream)
    base = table.data_ptr()
    gather_launch(base + int(offs[0]), B, s0.n_mel, eng.mel_width, s0.n_rem, s0.n_early, s0.n_early_size, w_max, cpf, dtype,
                  dev, out=bufs)
    frames_dev = table[int(offs[2]):int(offs[2]) + 4 * B].view(torch.int32)
    eng.run_infer(bufs[0], frames_dev, bufs[1], bufs[2], s0.sigma, audio)      # its address stands in the step's table
    if raw is not audio:
      raw.copy_(audio)
    if Bd:
      lengths_dev = table[int(offs[3]):int(offs[3]) + 4 * Bd].view(torch.int32)
      synth.denoiser.run_ragged(raw[:Bd], lengths[:Bd], lengths_dev, s0.strength, den)    # s0 denoises: sorted to the front
    if not pcm:
      for b, (i, s, p) in enumerate(act):
        r = raw[b, p.offset:p.offset + p.count]
        d = den[b, p.offset:p.offset + p.count] if b < Bd else r
        out[i] = StreamChunk(None, r, d, p.start_sample, hp.sampling_rate, None, None, None, p.final)
        s._advance(p)
      return out
    fin = emit_launch(base + int(offs[1]), B, n_max, dev)
    back, slot = ring.take(fin.numel())
    back.copy_(fin, non_blocking=True)
    ring.guard(slot, stream)
    stream.synchronize()
  samples, stats = emit_read(back, B, n_max)
  bad = np.nonzero(stats[:, NON_FINITE])[0]
  if bad.size:
    i, s, p = act[int(bad[0])]
    raise _lib.WgError(f"{s.name} (session {i} of the step) has NaN or infinite samples in the chunk at sample "
                       f"{p.start_sample}: it cannot be written as PCM")
  for b, (i, s, p) in enumerate(act):
    out[i] = StreamChunk(samples[b, :p.count].copy(), None, None, p.start_sample, hp.sampling_rate,
                         float(stats[b, RAW_MIN]), float(stats[b, RAW_MAX]), int(stats[b, CLIPPED]), p.final)
    s._advance(p)
  return out
