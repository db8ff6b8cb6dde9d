"""CPU-side checks of the device-resident training data path (waveglow_amd/device_data.py, wg_data_gather): the host
draws are the legacy loader's, the gather's arithmetic is convert_wav's, and the entry point refuses bad arguments before
any device work."""
import ctypes as C
import random

import numpy as np
import pytest
import torch
from torch.utils.data import DataLoader, Dataset

from _device_data_ref import gather_ref
from waveglow_amd import _lib, build
from waveglow_amd.audio import convert_wav, get_wav_tensor_segment
from waveglow_amd.device_data import iter_picks, shuffled

LENGTHS = [5000, 4096, 4095, 300, 9000, 4096, 1]
SEG, BATCH, SEED = 4096, 2, 1234


class _LegacySet(Dataset):
  """The host part of MelLoader (waveglow_amd/training.py) on ``torch.arange(len)`` "wavs": the first element of a
  returned segment is its start (0 for a padded one)."""

  def __init__(self, lengths, seed):
    data = list(lengths)
    random.seed(seed)
    random.shuffle(data)
    self.lengths = data

  def __getitem__(self, index):
    return get_wav_tensor_segment(torch.arange(self.lengths[index]), SEG)

  def __len__(self):
    return len(self.lengths)


def _legacy_loader(lengths, drop_last):
  return DataLoader(_LegacySet(lengths, SEED), num_workers=0, shuffle=False, batch_size=BATCH, drop_last=drop_last)


def _starts(batch):
  return [int(x) for x in batch[:, 0]]


@pytest.mark.parametrize("drop_last", [True, False])
def test_draws_are_the_legacy_loaders_over_two_epochs(drop_last):
  loader = _legacy_loader(LENGTHS, drop_last)
  legacy = [[_starts(b) for b in loader] for _ in range(2)]
  legacy_state = random.getstate()
  order = loader.dataset.lengths

  lengths = shuffled(LENGTHS, SEED)
  assert lengths == order
  ours = [[[s for _, s in picks] for picks in iter_picks(lengths, SEG, BATCH, drop_last)] for _ in range(2)]
  assert ours == legacy
  assert random.getstate() == legacy_state
  assert len(ours[0]) == (3 if drop_last else 4) and len(ours[0][-1]) == (2 if drop_last else 1)
  # every utterance of at least the segment length drew (4096 included), the shorter ones start at 0
  flat = [s for picks in iter_picks(lengths, SEG, BATCH, False) for s in picks]
  for (i, s), n in zip(flat, lengths):
    assert 0 <= s <= max(n - SEG, 0)
  assert [i for i, _ in flat] == list(range(len(lengths)))


def test_draws_in_the_train_then_validation_order():
  """train() builds the train loader, then the validation loader (the second constructor re-seeds), and runs a full
  validation pass between train batches."""
  val_lengths = [4200, 100, 8000]
  trn, val = _legacy_loader(LENGTHS, True), _legacy_loader(val_lengths, False)
  legacy = []
  for _ in range(2):
    for k, b in enumerate(trn):
      legacy.append(_starts(b))
      if k % 2 == 1:
        legacy.extend(_starts(v) for v in val)
  legacy_state = random.getstate()

  trn_l = shuffled(LENGTHS, SEED)
  val_l = shuffled(val_lengths, SEED)
  ours = []
  for _ in range(2):
    for k, picks in enumerate(iter_picks(trn_l, SEG, BATCH, True)):
      ours.append([s for _, s in picks])
      if k % 2 == 1:
        ours.extend([s for _, s in v] for v in iter_picks(val_l, SEG, BATCH, False))
  assert ours == legacy
  assert random.getstate() == legacy_state


def test_a_resume_that_skips_two_batches_still_consumes_their_draws():
  loader = _legacy_loader(LENGTHS, True)
  legacy = [_starts(b) for k, b in enumerate(loader) if k >= 2]      # the legacy loop loads and discards
  legacy += [_starts(b) for b in loader]
  legacy_state = random.getstate()
  lengths = shuffled(LENGTHS, SEED)
  ours = [[s for _, s in p] for p in iter_picks(lengths, SEG, BATCH, True, skip=2)]
  assert len(ours) == 1
  ours += [[s for _, s in p] for p in iter_picks(lengths, SEG, BATCH, True)]
  assert ours == legacy
  assert random.getstate() == legacy_state


def test_numpy_gather_is_convert_wav_and_segment_bit_for_bit():
  """slice, zero pad, / 32768 against convert_wav + get_wav_tensor_segment, on int16 rows that hold both extremes."""
  rng = np.random.default_rng(5)
  lens = [1031, 520, 519, 4097, 1]
  wavs = [rng.integers(-32768, 32768, size=n, dtype=np.int64).astype(np.int16) for n in lens]
  wavs[0][[0, 1030]] = (-32768, 32767)
  wavs[3][[1, 4096]] = (32767, -32768)
  wavs[4][0] = -32768
  pool = np.concatenate(wavs)
  offsets = np.concatenate([[0], np.cumsum(lens)])
  seen = set()
  for seg in (520, 4096):
    for u, w in enumerate(wavs):
      for seed in range(4):
        random.seed(seed)
        start = random.randint(0, len(w) - seg) if len(w) >= seg else 0
        random.seed(seed)
        legacy = get_wav_tensor_segment(torch.from_numpy(convert_wav(w, np.float32).astype(np.float32)), seg).numpy()
        ours, status = gather_ref(pool, offsets, [(u, start)], seg)
        assert status == 0 and ours.dtype == legacy.dtype == np.float32
        assert np.array_equal(ours[0].view(np.int32), legacy.view(np.int32))
        seen.update((float(ours.min()), float(ours.max())))
  assert -1.0 in seen and 32767 / 32768 in seen


def test_gather_refuses_bad_arguments_without_a_gpu():
  build.build_library()
  lib = _lib.load()
  assert "wg_data_gather" in _lib.SIGNATURES and hasattr(lib, "wg_data_gather")
  p = C.addressof((C.c_char * 64)())
  ok = dict(pool=p, dtype=_lib.WG_PCM_I16, elems=8, offsets=p, n_utt=1, picks=p, out=p, status=None, B=1, seg=4)

  def call(**kw):
    a = dict(ok, **kw)
    return lib.wg_data_gather(a["pool"], a["dtype"], a["elems"], a["offsets"], a["n_utt"], a["picks"], a["out"],
                              a["status"], a["B"], a["seg"], None)

  for name in ("pool", "offsets", "picks", "out"):
    assert call(**{name: None}) == -1 and b"null" in lib.wg_last_error(), name
  assert call(B=0) == -1
  assert call(n_utt=0) == -1
  assert call(seg=0) == -1
  assert call(dtype=2) == -1 and b"dtype" in lib.wg_last_error()
  assert call(dtype=-1) == -1
