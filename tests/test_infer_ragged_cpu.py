"""CPU companion of tests/test_gpu_infer_ragged.py (tests/_ragged_infer_grads.py): ``infer_differentiable(..., frames=)``.

* the keyword, its host validation (before any launch and before anything else about the call) and the C ABI of the two
  entry points behind it, header against binding, and their argument checks without a device;
* the recorded float32 ratios the GPU bound is made of, measured again;
* the defect the keyword removes, on the fp64 oracle: near its end an utterance synthesised alone differs from its row of
  the padded dense call -- so the cases can see it.
"""
import ctypes as C
import inspect
import os
import re

import pytest
import torch

import _ragged_infer_grads as R
from waveglow_amd import _lib, build
from waveglow_amd._lib import WgError
from waveglow_amd.model import WaveGlow

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("wg_train_infer_forward", "wg_train_infer_backward")
# the calls that take per-utterance lengths: (the nullable pointer, the argument it follows, the number of arguments)
LENGTHS = {
  "wg_infer": ("frames", "const void* mel", 14),
  "wg_forward": ("frames", "const void* mel", 14),
  "wg_train_infer_forward": ("frames", "int32_t n_frames", 16),
  "wg_train_infer_backward": ("frames", "int32_t n_frames", 17),
  "wg_stft_denoise": ("lens", "const float* audio", 12),
  "wg_stft_mel": ("lens", "const float* audio", 11),
  "wg_stft_mel_forward_saved": ("lens", "const float* audio", 11),
  "wg_stft_mel_backward": ("lens", "const float* g_mel", 11),
  "wg_stftloss_forward": ("lens", "const float* target", 13),
  "wg_stftloss_backward": ("lens", "const float* g_out3", 11),
}
_KINDS = {C.c_float: "float", C.c_int32: "int32_t", C.c_size_t: "size_t"}      # (c_int32 is c_int where int has 32 bits)


def test_frames_is_a_keyword_only_argument():
  sig = inspect.signature(WaveGlow.infer_differentiable)
  p = sig.parameters["frames"]
  assert p.kind is inspect.Parameter.KEYWORD_ONLY and p.default is None
  assert sig.parameters["weight_grads"].kind is inspect.Parameter.KEYWORD_ONLY
  assert [n for n, q in sig.parameters.items() if q.kind is inspect.Parameter.POSITIONAL_OR_KEYWORD] == \
      ["self", "spect", "sigma", "z_init", "z_early"]


def _frozen(rc):
  model = WaveGlow(rc.hp)
  model.load_state_dict(rc.sd)
  return model.requires_grad_(False)


@pytest.mark.parametrize("frames,match", [
  ([13, 0, 1, 9], r"frame counts in \[1, 13\]"),                              # a count of 0
  ([13, 5, 14, 9], r"frame counts in \[1, 13\]"),                             # T + 1
  ((13, 5, -1, 9), r"frame counts in \[1, 13\]"),
  ([13, 5, 1], "3 frame counts for a batch of 4"),                            # the wrong length
  ([13, 5, 1, 9, 9], "5 frame counts for a batch of 4"),
  (torch.tensor([13, 5, 1]), "3 frame counts for a batch of 4"),
  (torch.tensor([13.0, 5.0, 1.0, 9.0]), "integer frame counts"),              # a float tensor
  ([13, 5.0, 1, 9], "integer frame counts"),
  (torch.tensor([[13, 5, 1, 9]]), "1-d tensor of integer frame counts"),
  (torch.tensor([True, True, True, True]), "integer frame counts"),
  (13, "a list, a tuple or a tensor"),
])
def test_host_validation_refuses_before_anything_else(frames, match):
  """The counts are refused for what is wrong with THEM (the message says so), although the tensors of this call are on the
  CPU, which is refused too: the counts are looked at first, before any launch."""
  rc = R.case("c64_l8")
  mel, zi, ze, _ = rc.padded()
  model = _frozen(rc)
  with pytest.raises(WgError, match=match):
    model.infer_differentiable(mel.requires_grad_(True), R.SIGMA, z_init=zi, z_early=ze, frames=frames)


@pytest.mark.parametrize("frames", [[13, 5, 1, 9], (13, 13, 13, 13), torch.tensor([1, 1, 1, 1]),
                                    torch.tensor([13, 5, 1, 9], dtype=torch.int64)])
def test_cpu_input_tensors_are_refused_with_good_counts(frames):
  rc = R.case("c64_l8")
  mel, zi, ze, _ = rc.padded()
  with pytest.raises(WgError, match="no CPU fallback"):
    _frozen(rc).infer_differentiable(mel.requires_grad_(True), R.SIGMA, z_init=zi, z_early=ze, frames=frames)
  with pytest.raises(TypeError):
    _frozen(rc).infer_differentiable(mel, R.SIGMA, zi, ze, False, frames)      # keyword-only, both of them


def _header_decl(name):
  text = open(os.path.join(ROOT, "include", "waveglow_amd.h")).read()
  text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
  m = re.search(r"\b(\w[\w \*]*?)\b" + name + r"\s*\(([^;]*?)\)\s*;", text, flags=re.S)
  assert m, name
  return m.group(1).strip(), [" ".join(a.split()) for a in m.group(2).split(",")]


def _kinds(args):
  return ["ptr" if "*" in a else a.split()[0] for a in args]


@pytest.mark.parametrize("name", sorted(LENGTHS))
def test_header_and_binding_agree_argument_by_argument(name):
  """Return type and every argument: pointer / float / int32_t / size_t in the header is the same kind, at the same place,
  in _lib.SIGNATURES; and the call takes its per-utterance lengths as ``const int32_t* frames`` / ``lens`` where the ABI
  puts them: directly after mel (wg_infer, wg_forward), after n_frames (wg_train_infer_*), after the audio or gradient
  input (the STFT calls)."""
  ret, args = _header_decl(name)
  res, argtypes = _lib.SIGNATURES[name]
  assert (ret, res) == ("int", C.c_int)
  assert _kinds(args) == [_KINDS.get(t, "ptr") for t in argtypes]
  pointer, after, arity = LENGTHS[name]
  at = args.index(after) + 1
  assert args[at] == f"const int32_t* {pointer}" and argtypes[at] is C.c_void_p
  assert [a for a in args if a.split()[-1] in ("frames", "lens")] == [args[at]]       # the one pointer, once
  assert len(args) == len(argtypes) == arity


def test_argument_checks_need_no_device():
  """Null pointers and scale <= 0 are refused with WG_ERR_INVALID (-1) before anything touches a device."""
  build.build_library()
  lib = _lib.load()
  for name in NEW:
    assert hasattr(lib, name)
  buf = (C.c_float * 16)()
  p = C.cast(buf, C.c_void_p)
  w, g = _lib.WgTrainWeights(), _lib.WgTrainGrads()
  ze = (C.c_void_p * 1)(p)
  fwd, bwd = lib.wg_train_infer_forward, lib.wg_train_infer_backward
  # forward: (h, w, mel, z_init, z_early, n_z_early, sigma, audio, B, n_frames, frames, fresh, workspace, bytes, flags, stream)
  ok = [None, C.byref(w), p, p, ze, 1, 0.7, p, 1, 1, p, 1, p, 64, 0, None]
  for i in (1, 2, 3, 4, 7, 12):                      # every pointer the call dereferences; frames and stream may be null
    a = list(ok)
    a[i] = None
    assert fwd(*a) == -1, i
    assert b"null" in lib.wg_last_error()
  assert fwd(*ok) == -1 and b"null handle" in lib.wg_last_error()      # ... and then the handle
  a = list(ok)
  a[10] = None
  assert fwd(*a) == -1 and b"null handle" in lib.wg_last_error()       # frames == NULL is the dense call: same checks
  # backward: (h, w, grads, g_audio, scale, sigma, g_mel, g_z_init, g_z_early, n_z_early, B, n_frames, frames, workspace, bytes, flags, stream)
  ok = [None, C.byref(w), C.byref(g), p, 1.0, 0.7, p, p, ze, 1, 1, 1, p, p, 64, 0, None]
  for i in (1, 3, 13):
    a = list(ok)
    a[i] = None
    assert bwd(*a) == -1, i
    assert b"null argument" in lib.wg_last_error()
  for scale in (0.0, -1.0, float("nan")):
    a = list(ok)
    a[4] = scale
    assert bwd(*a) == -1 and b"scale must be positive" in lib.wg_last_error()
  assert bwd(*ok) == -1 and b"null handle" in lib.wg_last_error()
  # the dense batch is this call with frames == NULL: the same answers
  assert bwd(None, C.byref(w), C.byref(g), p, 0.0, 0.7, p, p, ze, 1, 1, 1, None, p, 64, 0, None) == -1
  assert b"scale must be positive" in lib.wg_last_error()


def test_cases_reach_the_corners():
  for name, frames in R.FRAMES.items():
    rc = R.case(name)
    assert len(frames) == rc.B == len(R.FRAMES_2[name]) and max(frames) == rc.T and min(frames) < rc.T
    assert all(1 <= f <= rc.T and f != f2 for f, f2 in zip(frames, R.FRAMES_2[name]))
    assert 0.0 < R.bound(name) <= R.BOUND_LIMIT
  f = R.FRAMES["c64_l8"]
  assert f[0] == 13 and 32 * f[1] == 160 and 160 % 128 and 32 * f[2] == 32          # a full row; inside a tile; below d >= 32
  assert R.case("c64_l10").B % 2 == 1 and 32 * max(R.FRAMES["c64_l10"]) < 256        # no half-batch split; d = 256, 512 outside
  mel, zi, ze, r = R.case("c64_l8").padded()
  for b, n in enumerate(f):
    for t, unit in [(mel, 1), (zi, 32), (r, 256)] + [(z, 32) for z in ze]:
      assert bool(torch.isfinite(t[b, ..., :unit * n]).all()) and bool(torch.isnan(t[b, ..., unit * n:]).all())


@pytest.mark.parametrize("name", sorted(R.FRAMES))
def test_float32_ratios_still_hold(name):
  """The constants the GPU bound is made of, measured again on the float32 oracle (as tests/test_batch_independence_cpu.py
  holds its own: within a factor of two above and four below a fresh measurement), and the bound below GRAD_TOL / 50."""
  fresh, q = R.measure_f32(name)
  rec = R.F32_RATIO[name]
  print(f"{name}: float32 ratio {fresh:.3e} ({q}), recorded {rec:.3e}, GPU bound {R.bound(name):.3e}")
  assert fresh <= 2.0 * rec and rec <= 4.0 * fresh
  assert 0.0 < R.bound(name) <= R.BOUND_LIMIT


def test_padded_dense_call_differs_from_the_crops_near_their_ends():
  """The defect: the flow on the padded batch computes an utterance's last columns from the mel's padding (here: the
  neighbouring frames of the padded mel, and the noise behind the count).  fp64 oracle, case 1: every short utterance's
  crop differs from its row of the dense call in its last frames by far more than rounding -- in the audio and in d mel --
  while the full row agrees to rounding, and well inside an utterance longer than the receptive field the two agree."""
  rc = R.case("c64_l8")
  dense = R.oracle_dense(rc)
  seen = 0
  for b, f in enumerate(rc.frames):
    one = R.oracle_crop(rc, b)
    for q, unit in (("audio", 256), ("d mel", 1)):
      x, y = dense[q][b:b + 1, ..., :unit * f], one[q]
      tail = slice(unit * (f - 1), unit * f)
      d_tail = float((x[..., tail] - y[..., tail]).norm()) / float(y[..., tail].norm())
      d_all = float((x - y).norm()) / float(y.norm())
      print(f"c64_l8 fp64 row {b} ({f} frames) {q}: last frame differs by {d_tail:.3e}, whole crop by {d_all:.3e}")
      if f == rc.T:
        assert d_all <= R.BI.ROW_TOL_64, (b, q, d_all)
      else:
        assert d_tail >= 1e-3, (b, q, d_tail)
        seen += 1
  assert seen == 2 * sum(1 for f in rc.frames if f < rc.T)
  # ... and the dense call's d mel behind a count is not zero (its flow ran there), which frames= makes exact zeros
  for b, f in enumerate(rc.frames):
    if f < rc.T:
      assert float(dense["d mel"][b, :, f:].abs().max()) > 0.0
