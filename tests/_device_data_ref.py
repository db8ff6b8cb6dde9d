"""Numpy restatement of wg_data_gather (include/waveglow_amd.h), shared by the CPU and the GPU tests of the device data
path: slice, zero pad, / 32768 for int16."""
import numpy as np


def gather_ref(pool: np.ndarray, offsets, picks, segment_length: int):
  """(audio [B, segment_length] float32, status) of the picks [(utterance, start), ...]."""
  n_utt = len(offsets) - 1
  out = np.zeros((len(picks), segment_length), dtype=np.float32)
  status = 0
  for b, (u, s) in enumerate(picks):
    if not 0 <= u < n_utt:
      status = 1
      continue
    lo, n = int(offsets[u]), int(offsets[u + 1] - offsets[u])
    if s < 0 or s > max(n - segment_length, 0):
      status = 1
      continue
    x = pool[lo + s:lo + min(s + segment_length, n)]
    if x.dtype == np.int16:
      x = x.astype(np.float32) / np.float32(32768)
    out[b, :len(x)] = x
  return out, status
