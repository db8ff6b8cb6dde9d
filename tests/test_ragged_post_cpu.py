"""CPU-side checks of the batched post-processing entry points (wg_stft_denoise and wg_stft_mel with per-utterance
lengths, wg_wav_finish): exported, bound, and refusing null arguments before any device work."""
import ctypes as C

import numpy as np
import pytest

from waveglow_amd import _lib, build

NEW = ("wg_stft_denoise", "wg_stft_mel", "wg_wav_finish")


@pytest.fixture(scope="module")
def lib():
  build.build_library()
  return _lib.load()


def test_new_symbols_exported_and_bound(lib):
  for name in NEW + ("wg_wav_finish_workspace_bytes",):
    assert name in _lib.SIGNATURES, name
    assert hasattr(lib, name), name


def test_null_arguments_are_refused_without_a_device(lib):
  buf = C.addressof((C.c_char * 64)())
  assert lib.wg_stft_denoise(None, None, None, None, 0.5, None, None, 2, 2048, None, 0, None) == -1
  assert b"null" in lib.wg_last_error()
  # null lengths are the dense batch, not an argument error: with a handle-shaped pointer and otherwise sound arguments
  # the call gets the answer of the call with lengths.  Compared at the last refusal that needs no device, a workspace
  # one byte short: past it the call enqueues work.
  need = lib.wg_stft_workspace_bytes(buf, 2, 2048)
  assert need > 0
  answers = [(lib.wg_stft_denoise(buf, buf, lens, None, 0.5, buf, None, 2, 2048, buf, need - 1, None), lib.wg_last_error())
             for lens in (buf, None)]
  assert answers[0] == answers[1] and answers[0][0] == -4 and b"workspace" in answers[0][1]
  assert lib.wg_stft_denoise(buf, None, None, None, 0.5, buf, None, 2, 2048, buf, need, None) == -1
  assert lib.wg_stft_mel(None, None, 80, None, None, None, 2, 2048, None, 0, None) == -1
  assert lib.wg_wav_finish(None, None, None, None, None, 2, 2048, None, 0, None) == -1
  assert b"null" in lib.wg_last_error()
  assert lib.wg_wav_finish(buf, buf, None, buf, buf, 2, 2048, buf, 1 << 20, None) == -1


def test_wav_finish_checks_geometry_before_any_launch(lib):
  raw = (C.c_char * 256)()
  p = (C.addressof(raw) + 15) // 16 * 16
  assert lib.wg_wav_finish_workspace_bytes(0) == 0
  assert lib.wg_wav_finish_workspace_bytes(3) >= 3 * 64 * 5 * 4          # 64 chunks x 5 values per utterance
  assert lib.wg_wav_finish(p, p, p, p, p, 1, 2044, p, 1 << 20, None) == -1   # not a multiple of 8
  assert lib.wg_wav_finish(p, p, p, p, p, 0, 2048, p, 1 << 20, None) == -1
  assert lib.wg_wav_finish(p + 4, p, p, p, p, 1, 2048, p, 1 << 20, None) == -1 and b"aligned" in lib.wg_last_error()
  assert lib.wg_wav_finish(p, p, p, p, p, 1, 2048, p, 16, None) == -4        # WG_ERR_WORKSPACE


def test_tie_row_of_the_gpu_test_is_what_it_claims():
  """The rounding row of tests/test_gpu_ragged_post.py, checked where no GPU is needed: 65 534 exact .5 ties, not
  rescaled by normalize_wav (peak 1), rounded half to even by convert_wav."""
  from waveglow_amd.audio import convert_wav, normalize_wav
  k = np.arange(-32767, 32767, dtype=np.float32)
  row = np.concatenate([(k + np.float32(0.5)) / np.float32(32767), np.ones(1, np.float32)]).astype(np.float32)
  t = row * np.float32(32767)
  assert int(np.sum(t - np.floor(t) == 0.5)) == 65534
  assert normalize_wav(row) is row
  out = convert_wav(row, np.int16)
  assert out.dtype == np.int16 and np.all(out[:-1] % 2 == 0) and out[-1] == 32767
