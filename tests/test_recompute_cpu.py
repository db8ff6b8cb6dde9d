"""CPU checks of activation recomputation (include/waveglow_amd.h: WG_TRAIN_RECOMPUTE): workspace sizing, the refusal of
a call whose flags do not match its workspace, and the training-workspace pool keyed by mode.  No device work runs: the
argument checks come before any launch."""
import ctypes as C

import pytest
import torch

from waveglow_amd import _lib
from waveglow_amd.model import _Engine

RC = _lib.WG_TRAIN_RECOMPUTE


@pytest.fixture
def handle():
  lib = _lib.load()
  h = C.c_void_p()
  assert lib.wg_create(C.byref(_lib.WgConfig(80, 12, 8, 4, 2, 8, 256, 3, 1024, 256)), 0, C.byref(h)) == 0
  yield lib, h
  lib.wg_destroy(h)


def test_workspace_bytes_of_both_modes(handle):
  lib, h = handle
  full = lib.wg_train_workspace_bytes(h, 32, 63, 16000, 0)
  rec = lib.wg_train_workspace_bytes(h, 32, 63, 16000, RC)
  assert full > 20 * 2 ** 30
  assert 0 < rec <= 0.25 * full                                     # 0.20 at 256 channels
  # whole utterances: 16 x 10 s (861 frames) -- about 135 GB of saved planes without recomputation
  assert lib.wg_train_workspace_bytes(h, 16, 861, 861 * 256, RC) < 0.25 * lib.wg_train_workspace_bytes(h, 16, 861, 861 * 256, 0)
  assert lib.wg_train_workspace_bytes(h, 32, 63, 16000, 2) == 0 and b"flags" in lib.wg_last_error()
  assert lib.wg_train_workspace_bytes(h, 32, 63, 16001, RC) == 0


def test_recompute_refused_where_two_slots_hold_every_flow():
  """Two flows: the two slots hold every flow, so the flag saves nothing.  It used to be refused there; it is accepted now
  (a model's depth does not decide whether the switch works), on a workspace of its own size -- no smaller than the
  full-save one, so the size check that tells the layouts apart does not apply: both calls get as far as the weight checks."""
  lib = _lib.load()
  h = C.c_void_p()
  assert lib.wg_create(C.byref(_lib.WgConfig(80, 2, 8, 1, 2, 2, 128, 3, 1024, 256)), 0, C.byref(h)) == 0
  try:
    full = lib.wg_train_workspace_bytes(h, 2, 7, 1792, 0)
    rec = lib.wg_train_workspace_bytes(h, 2, 7, 1792, RC)
    assert 0 < full <= rec
    w = _lib.WgTrainWeights()
    buf = (C.c_char * 64)()
    p = C.addressof(buf)
    ls = (C.c_void_p * 2)(p, p)
    for nbytes, flags in ((rec, RC), (full, 0), (rec, 0)):
      assert lib.wg_train_forward(h, C.byref(w), p, p, p, ls, 2, 7, 1792, 0, p, nbytes, flags, None) == -1
      assert b"null member" in lib.wg_last_error(), (nbytes, flags)
    if rec > full:
      assert lib.wg_train_forward(h, C.byref(w), p, p, p, ls, 2, 7, 1792, 0, p, full, RC, None) == -4   # too small
  finally:
    lib.wg_destroy(h)


def test_flags_must_match_the_workspace_size(handle):
  """A workspace keeps one layout from its forward to its backward: every flag-taking entry point refuses a workspace
  of the other mode's size with WG_ERR_INVALID (-1); with matching sizes the call gets as far as its weight checks."""
  lib, h = handle
  B, T, S = 2, 8, 2048
  full = lib.wg_train_workspace_bytes(h, B, T, S, 0)
  rec = lib.wg_train_workspace_bytes(h, B, T, S, RC)
  assert 0 < rec < full
  w = _lib.WgTrainWeights()
  buf = (C.c_char * 64)()
  p = C.addressof(buf)
  ls = (C.c_void_p * 12)(*[p] * 12)

  def fwd(nbytes, flags):
    return lib.wg_train_forward(h, C.byref(w), p, p, p, ls, B, T, S, 0, p, nbytes, flags, None)

  def bwd(nbytes, flags):
    return lib.wg_train_backward(h, C.byref(w), None, p, ls, C.c_float(1.0), p, None, None, B, T, S, p, nbytes, 11, 0, flags,
                                 None)

  def ifwd(nbytes, flags):
    ze = (C.c_void_p * 2)(p, p)
    return lib.wg_train_infer_forward(h, C.byref(w), p, p, ze, 2, C.c_float(1.0), p, B, T, None, 0, p, nbytes, flags, None)

  def ibwd(nbytes, flags):
    return lib.wg_train_infer_backward(h, C.byref(w), None, p, C.c_float(1.0), C.c_float(1.0), None, None, None, 2, B, T, None,
                                       p, nbytes, flags, None)

  for call in (fwd, bwd, ifwd, ibwd):
    assert call(full, RC) == -1 and b"do not match" in lib.wg_last_error(), call.__name__
    assert call(rec, 0) == -1 and b"do not match" in lib.wg_last_error(), call.__name__
    assert call(rec - 1, RC) == -4, call.__name__                                        # too small
    assert call(rec, RC) == -1 and b"null member" in lib.wg_last_error(), call.__name__   # past the size checks
    assert call(full, 0) == -1 and b"null member" in lib.wg_last_error(), call.__name__


def test_training_workspace_pool_is_keyed_by_mode():
  """Both modes' workspaces of one geometry live side by side (no reallocation when the mode alternates); a geometry
  change drops both."""
  eng = object.__new__(_Engine)
  eng._train_pool = []
  eng.device = torch.device("cpu")
  a, fresh_a = eng.train_workspace(100, (2, 8, 2048), 0)
  b, fresh_b = eng.train_workspace(40, (2, 8, 2048), RC)
  assert fresh_a and fresh_b and a is not b and len(eng._train_pool) == 2
  a["busy"] = b["busy"] = False
  for _ in range(3):
    for flags, want in ((0, a), (RC, b)):
      e, fresh = eng.train_workspace(100 if flags == 0 else 40, (2, 8, 2048), flags)
      assert e is want and not fresh
      e["busy"] = False
  c, fresh_c = eng.train_workspace(100, (2, 8, 2048), 0)           # both outstanding in one mode: a second one
  d, fresh_d = eng.train_workspace(100, (2, 8, 2048), 0)
  assert c is a and d is not a and fresh_d and len(eng._train_pool) == 3
  eng.train_workspace(60, (4, 8, 2048), RC)
  assert len(eng._train_pool) == 1
