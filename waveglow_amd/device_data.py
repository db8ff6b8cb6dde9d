"""Opt-in training data path that keeps the whole wav set on the device (``train(..., device_dataset=True)``).

``MelLoader`` (waveglow_amd/training.py, the reference's dataloader.py:45-54) builds a batch one utterance at a time: a
host crop, a blocking upload, a ``B = 1`` mel call with two host synchronisations, and a stack at the end.  Here the
files are read once into one device array (``DeviceWavPool``), and a batch is one small upload of ``[B][2]`` picks, one
``wg_data_gather`` launch and one batched ``wg_stft_mel`` call (``DeviceBatchLoader``), enqueued without a synchronise.

The batches are the ones ``DataLoader(MelLoader(...))`` delivers under the same seed, bit for bit: the host draws are
made by the same calls in the same order (``shuffled`` / ``draw_batch``), the int16 -> fp32 scaling is by a power of two,
and the mel kernels give an utterance of a batch the bits of its own call.
"""
from __future__ import annotations

import ctypes as C
import random
from logging import getLogger
from typing import Iterator, List, Sequence, Tuple

import numpy as np
import torch

from . import _args, _lib
from .audio import convert_wav
from .taco_stft import FLOAT32_64_MAX_WAV, FLOAT32_64_MIN_WAV, TacotronSTFT

Pick = Tuple[int, int]      # (utterance index, start sample)


# ---------------------------------------------------------------- host draws (no device needed)
def shuffled(entries: Sequence, seed: int) -> list:
  """The file order of ``MelLoader.__init__`` (dataloader.py:24-27): re-seeds ``random``, then shuffles a copy."""
  data = list(entries)
  random.seed(seed)
  random.shuffle(data)
  return data


def batch_count(n_items: int, batch_size: int, drop_last: bool) -> int:
  return n_items // batch_size if drop_last else (n_items + batch_size - 1) // batch_size


def draw_batch(lengths: Sequence[int], segment_length: int, lo: int, hi: int) -> List[Pick]:
  """Picks of the items ``lo .. hi - 1`` in index order, consuming ``random`` as ``get_wav_tensor_segment`` does
  (audio_utils.py:141-150): one ``randint(0, len - segment_length)`` iff ``len >= segment_length`` (``randint(0, 0)`` for
  an utterance of exactly the segment length), nothing and start 0 for a shorter one."""
  picks = []
  for i in range(lo, hi):
    n = int(lengths[i])
    picks.append((i, random.randint(0, n - segment_length) if n >= segment_length else 0))
  return picks


def iter_picks(lengths: Sequence[int], segment_length: int, batch_size: int, drop_last: bool,
               skip: int = 0) -> Iterator[List[Pick]]:
  """The picks of one epoch, batch by batch, each drawn when it is asked for -- as ``DataLoader`` fetches the items of a
  batch when the loop asks for it.  With ``drop_last`` the items of an incomplete last batch are never drawn.  The first
  ``skip`` batches are drawn and dropped (a resumed epoch: the legacy loop loads and discards them)."""
  n = len(lengths)
  for k in range(batch_count(n, batch_size, drop_last)):
    picks = draw_batch(lengths, segment_length, k * batch_size, min((k + 1) * batch_size, n))
    if k >= skip:
      yield picks


# ---------------------------------------------------------------- the pool
class DeviceWavPool:
  """Every wav of ``entries``, in their order, back to back in one device array.

  Each file is read once with the reader of ``wav_to_float32`` and its sampling rate checked as
  ``TacotronSTFT.get_wav_tensor_from_file`` checks it.  If every file is int16 the pool keeps the raw int16 samples
  (``wg_data_gather`` scales them by 1 / 32768, which is what ``convert_wav`` gives); otherwise it keeps fp32 after
  ``convert_wav``, and the reference's [-1, 1] assert (taco_stft.py:95-97) is applied here, once, on the host.  A file
  without samples is allowed: its rows come out as zeros.

  ``resample_inputs`` (not in the reference): files at other rates are resampled to ``hparams.sampling_rate`` on the device
  while the pool is built (waveglow_amd/resample.py, clipped to [-1, 1]), ``RESAMPLE_FILES`` files of one rate per launch.
  Such a pool is fp32, and ``lengths`` are the resampled lengths."""

  RESAMPLE_FILES = 64      # files per upload and wg_resample launch while a resampled pool is built

  def __init__(self, entries: Sequence, hparams, device, resample_inputs: bool = False):
    from scipy.io.wavfile import read
    self.device = torch.device(device)
    if self.device.type != "cuda":
      raise _lib.WgError("the device wav pool lives on the GPU only")
    wavs, rates = [], []
    for e in entries:
      sampling_rate, wav = read(e.wav_absolute_path)
      rates.append(int(sampling_rate))
      if sampling_rate != hparams.sampling_rate and not resample_inputs:
        raise ValueError(f"{e.wav_absolute_path}: The sampling rate of the file ({sampling_rate}Hz) doesn't match the "
                         f"target sampling rate ({hparams.sampling_rate}Hz)!")
      if wav.ndim != 1:
        raise ValueError(f"{e.wav_absolute_path}: only mono files can be pooled")
      wavs.append(wav)
    if len(wavs) == 0:
      raise _lib.WgError("the device wav pool needs at least one file")
    if any(r != hparams.sampling_rate for r in rates):
      self._build_resampled(entries, wavs, rates, int(hparams.sampling_rate))
      return
    self.is_int16 = all(w.dtype == np.int16 for w in wavs)
    if not self.is_int16:
      wavs = [np.ascontiguousarray(convert_wav(w, np.float32), dtype=np.float32) for w in wavs]
      for e, w in zip(entries, wavs):
        if w.size:
          assert float(w.min()) >= FLOAT32_64_MIN_WAV and float(w.max()) <= FLOAT32_64_MAX_WAV, e.wav_absolute_path
    self.lengths: List[int] = [int(w.shape[0]) for w in wavs]
    offsets = np.zeros(len(wavs) + 1, dtype=np.int64)
    np.cumsum(self.lengths, out=offsets[1:])
    self.n_utt = len(wavs)
    self.elems = int(offsets[-1])
    host = np.concatenate(wavs) if self.elems else np.zeros(0, dtype=wavs[0].dtype)
    if host.size == 0:
      host = np.zeros(1, dtype=host.dtype)        # a pointer to hand over; pool_elems stays 0 and nothing is read
    self.pool = torch.from_numpy(host).to(self.device)
    self.offsets = torch.from_numpy(offsets).to(self.device)
    self._log()

  def _log(self) -> None:
    self.dtype_code = _lib.WG_PCM_I16 if self.is_int16 else _lib.WG_PCM_F32
    getLogger(__name__).info(f"Device wav pool: {self.n_utt} files, {self.elems} samples, "
                             f"{self.pool.numel() * self.pool.element_size()} bytes "
                             f"({'int16' if self.is_int16 else 'float32'}) on {self.device}")

  def _build_resampled(self, entries, wavs, rates, target: int) -> None:
    """The pool of files of which at least one is not at ``target`` Hz: fp32.  Files at ``target`` are converted and
    range-checked on the host as above and uploaded; the others go up as read (int16 stays int16) in batches of at most
    ``RESAMPLE_FILES`` files of one rate, padded to the longest of the batch, and each batch is one ``wg_resample`` launch
    whose rows are then copied to their places in the pool.  The lengths follow from the file lengths on the host."""
    from .resample import out_len, resample, resample_plan
    self.is_int16 = False
    lens = []
    for w, r in zip(wavs, rates):
      up, down, _, _ = resample_plan(r, target)
      lens.append(out_len(int(w.shape[0]), up, down))
    self.lengths = lens
    offsets = np.zeros(len(wavs) + 1, dtype=np.int64)
    np.cumsum(lens, out=offsets[1:])
    self.n_utt = len(wavs)
    self.elems = int(offsets[-1])
    self.pool = torch.zeros(max(self.elems, 1), dtype=torch.float32, device=self.device)
    self.offsets = torch.from_numpy(offsets).to(self.device)
    by_rate = {}
    for i, r in enumerate(rates):
      by_rate.setdefault(r, []).append(i)
    for r, idx in by_rate.items():
      for lo in range(0, len(idx), self.RESAMPLE_FILES):
        chunk = [i for i in idx[lo:lo + self.RESAMPLE_FILES] if wavs[i].shape[0] > 0]
        if not chunk:
          continue
        part = [wavs[i] for i in chunk]
        if r == target or not all(w.dtype == np.int16 for w in part):
          part = [np.ascontiguousarray(convert_wav(w, np.float32), dtype=np.float32) for w in part]
          for i, w in zip(chunk, part):
            assert float(w.min()) >= FLOAT32_64_MIN_WAV and float(w.max()) <= FLOAT32_64_MAX_WAV, \
                entries[i].wav_absolute_path
        n = [int(w.shape[0]) for w in part]
        host = np.zeros((len(part), max(n)), dtype=part[0].dtype)
        for k, w in enumerate(part):
          host[k, :n[k]] = w
        dev = torch.from_numpy(host).to(self.device)
        if r != target:
          dev, _ = resample(dev, n, r, target, clip=True)
        for k, i in enumerate(chunk):
          self.pool[int(offsets[i]):int(offsets[i + 1])].copy_(dev[k, :lens[i]])
    self._log()

  def gather(self, picks_dev: torch.Tensor, segment_length: int, status: torch.Tensor = None) -> torch.Tensor:
    """Enqueue ``wg_data_gather`` on the current stream: ``picks_dev`` int32 [B, 2] on the pool's device ->
    fp32 [B, segment_length].  ``status`` (int32 [1] on the device) is set to 1 by a pick outside the pool."""
    if picks_dev.dtype != torch.int32 or picks_dev.dim() != 2 or picks_dev.shape[1] != 2 or \
        not picks_dev.is_contiguous() or picks_dev.device.type != "cuda" or \
        _lib.device_index(picks_dev.device) != _lib.device_index(self.device):
      raise _lib.WgError(f"gather takes contiguous int32 picks [B, 2] on {self.device}")
    B = picks_dev.shape[0]
    out = torch.empty((B, segment_length), dtype=torch.float32, device=self.device)
    _lib.check(_lib.load().wg_data_gather(_args.ptr(self.pool), self.dtype_code, self.elems, _args.ptr(self.offsets),
                                          self.n_utt, _args.ptr(picks_dev), _args.ptr(out), _args.ptr(status), B,
                                          segment_length, _args.stream(self.device)))
    return out


# ---------------------------------------------------------------- the loader
class DeviceBatchLoader:
  """``(mel, audio)`` batches of the shapes, dtypes and values ``DataLoader(MelLoader(entries, hparams, device))``
  yields: ``mel`` [B, n_mel, segment_length // 256 + 1] and ``audio`` [B, segment_length], fp32 on the device.

  The constructor re-seeds and shuffles as ``MelLoader.__init__`` does, so loaders are built in the legacy order (train,
  then validation).  ``for batch in loader`` walks one epoch; ``epoch(skip)`` does the same with the batch index, and
  draws but does not build the first ``skip`` batches.  ``prefetch()`` enqueues the next batch -- batch 0 of the next
  epoch behind the last one -- on the current stream; the running iterator then hands it out.  Nothing here synchronises
  with the device: ``post_status()`` enqueues the copy of the bad-pick flag behind the work queued so far and
  ``check_status()`` reads it once the caller has synchronised (``train()`` does both around its ``loss.item()``)."""

  def __init__(self, entries: Sequence, hparams, device, drop_last: bool, resample_inputs: bool = False):
    self.device = torch.device(device)
    self.hparams = hparams
    self.drop_last = bool(drop_last)
    self.batch_size = int(hparams.batch_size)
    self.segment_length = int(hparams.segment_length)
    data = shuffled(entries, hparams.seed)
    self.taco_stft = TacotronSTFT(hparams, self.device, resample_inputs=resample_inputs)
    self.pool = DeviceWavPool(data, hparams, self.device, resample_inputs=resample_inputs) if data else None
    self.lengths = self.pool.lengths if self.pool is not None else []
    self._n = batch_count(len(self.lengths), self.batch_size, self.drop_last)
    self.status = torch.zeros(1, dtype=torch.int32, device=self.device)
    self._status_host = torch.zeros(1, dtype=torch.int32).pin_memory()
    # two pinned pick buffers, each guarded by an event recorded behind the upload that reads it
    self._pin = [torch.zeros((self.batch_size, 2), dtype=torch.int32).pin_memory() for _ in range(2)]
    self._pin_ev = [None, None]
    self._pin_next = 0
    self._pos = 0             # batch the next _produce() builds
    self._ahead = None        # (batch index, batch) enqueued by prefetch() and not handed out yet

  def __len__(self) -> int:
    return self._n

  def _bounds(self, k: int) -> Tuple[int, int]:
    return k * self.batch_size, min((k + 1) * self.batch_size, len(self.lengths))

  def _enqueue(self, picks: List[Pick]):
    slot = self._pin_next
    self._pin_next ^= 1
    if self._pin_ev[slot] is not None:
      self._pin_ev[slot].synchronize()        # the upload out of this buffer two batches ago (long done)
    B = len(picks)
    host = self._pin[slot][:B]
    host.numpy()[:] = picks
    picks_dev = torch.empty((B, 2), dtype=torch.int32, device=self.device)
    picks_dev.copy_(host, non_blocking=True)
    ev = torch.cuda.Event()
    ev.record(torch.cuda.current_stream(self.device))
    self._pin_ev[slot] = ev
    audio = self.pool.gather(picks_dev, self.segment_length, self.status)
    return self.taco_stft._mel(audio), audio

  def _produce(self):
    if self._pos >= self._n:
      self._pos = 0
    k = self._pos
    self._pos += 1
    return k, self._enqueue(draw_batch(self.lengths, self.segment_length, *self._bounds(k)))

  def prefetch(self) -> None:
    if self._ahead is None and self._n > 0:
      self._ahead = self._produce()

  def epoch(self, skip: int = 0):
    """One epoch as ``(batch index, (mel, audio))``; the first ``skip`` batches are drawn, not built."""
    if self._ahead is not None:
      if skip or self._ahead[0] != 0:
        raise _lib.WgError("a prefetched batch is pending: an epoch continues with it")
      k = -1
    else:
      for j in range(min(skip, self._n)):
        draw_batch(self.lengths, self.segment_length, *self._bounds(j))
      self._pos = skip
      k = skip - 1
    while k + 1 < self._n:
      if self._ahead is not None:
        (k, batch), self._ahead = self._ahead, None
      else:
        k, batch = self._produce()
      yield k, batch

  def __iter__(self):
    for _, batch in self.epoch():
      yield batch

  def post_status(self) -> None:
    """Enqueue the copy of the bad-pick flag to the host behind everything queued so far."""
    self._status_host.copy_(self.status, non_blocking=True)

  def check_status(self, sync: bool = False) -> None:
    """Raise if a gather met a pick outside the pool.  Reads the copy ``post_status()`` enqueued; the caller has
    synchronised since (``sync=True``: post and wait here)."""
    if sync:
      self.post_status()
      torch.cuda.current_stream(self.device).synchronize()
    if int(self._status_host[0]) != 0:
      raise _lib.WgError("device data loader: a pick lies outside the wav pool")
