"""CPU-side checks of the STOI loss: the torch restatement the GPU tests differentiate (tests/_stoi_loss_oracle.py) against
the numpy oracle of the metric and against finite differences, the shared cases' margins, the rounding yardstick of the
device bar, the numpy pair of the resampler and its transpose, the transposed polyphase table, and the argument refusals
of the new entry points and of the Python layer that need no device."""
import ctypes as C

import numpy as np
import pytest
import torch

import _stoi_loss_cases as cases
import _stoi_loss_oracle as lo
import _stoi_oracle as oracle


@pytest.mark.parametrize("dft", ["rfft", "direct"])
def test_torch_restatement_equals_the_numpy_oracle(dft):
  for name in cases.NAMES + ("short",):
    x, y = cases.pair(name)
    ref = oracle.stoi(x, y)
    d, e, info = lo.scores(x, torch.from_numpy(y.astype(np.float64)), dft)
    assert (info["frames"], info["frames_kept"], info["segments"]) == (ref["frames"], ref["frames_kept"], ref["segments"])
    assert info["margin"] == ref["margin"]
    if ref["segments"] == 0:
      assert np.isnan(ref["stoi"]) and torch.isnan(d) and torch.isnan(e)
    else:
      print(name, dft, float(d) - ref["stoi"], float(e) - ref["estoi"])
      assert abs(float(d) - ref["stoi"]) <= 1e-12 and abs(float(e) - ref["estoi"]) <= 1e-12


def test_cases_are_what_their_names_say():
  want = {"j1": (31, 31, 1), "j5": (35, 35, 5), "f33": (34, 34, 4), "gated": (50, 43, 13), "loud": (31, 31, 1),
          "silent": (31, 31, 1), "short": (20, 20, 0)}
  for name, counts in want.items():
    x, y = cases.pair(name)
    assert x.dtype == y.dtype == np.float32
    r = oracle.stoi(x, y)
    print(name, r)
    assert (r["frames"], r["frames_kept"], r["segments"]) == counts, name
    assert r["margin"] >= cases.MIN_MARGIN, name
  assert len(cases.pair("j1")[0]) == 4224
  # the gated case: frame 0, frames 20 .. 24 and the last frame
  x, _ = cases.pair("gated")
  w = oracle.window()
  e = np.array([20 * np.log10(np.sqrt(np.sum((w * x[i:i + 256].astype(np.float64)) ** 2)) + oracle.EPS)
                for i in range(0, len(x) - 256, 128)])
  assert np.flatnonzero(e.max() - 40 - e >= 0).tolist() == [0, 20, 21, 22, 23, 24, 49]
  assert cases.reference("loud")[3]["clipped"] > 0 and cases.reference("j1")[3]["clipped"] == 0
  g, d, e, _ = cases.reference("silent")
  assert d == 0.0 and e == 0.0 and not g.any() and not np.isnan(g).any()
  assert not cases.reference("short")[0].any()


def test_gradcheck_of_the_restatement_at_the_smallest_case():
  """J = 1, away from ties: the analytic gradient of both values against central differences."""
  x, y = cases.pair("j1")
  for dft in ("rfft", "direct"):
    for pick in (0, 1):
      fn = lambda yt: lo.scores(x, yt, dft)[pick]
      yt = torch.tensor(y.astype(np.float64), requires_grad=True)
      assert torch.autograd.gradcheck(fn, (yt,), eps=1e-6, atol=1e-7, rtol=1e-5, nondet_tol=0.0, fast_mode=True)
  # a few single coordinates slowly, the first and the last sample included
  yt = torch.tensor(y.astype(np.float64), requires_grad=True)
  d, e, _ = lo.scores(x, yt)
  (d + 0.5 * e).backward()
  for i in (0, 127, 128, 2000, 4095, 4096, 4223):
    step = np.zeros(len(y))
    step[i] = 1e-6
    f = lambda v: (lambda r: float(r[0] + 0.5 * r[1]))(lo.scores(x, torch.from_numpy(v)))
    fd = (f(y.astype(np.float64) + step) - f(y.astype(np.float64) - step)) / 2e-6
    assert abs(fd - float(yt.grad[i])) <= 1e-8 + 1e-5 * abs(fd), (i, fd, float(yt.grad[i]))
  assert float(yt.grad[4096:].abs().max()) == 0.0                  # behind the last frame


def test_rounding_yardstick_of_the_gradient():
  worst = 0.0
  for name in cases.NAMES:
    g, g2 = cases.reference(name)[0], cases.reference(name, "direct")[0]
    top = float(np.max(np.abs(g)))
    if top > 0:
      worst = max(worst, float(np.max(np.abs(g - g2))) / top)
  print(f"Y = max |g_rfft - g_direct| / max |g| over the cases: {worst:.3e} (stated: {cases.Y:.3e})")
  assert 0 < worst <= cases.Y


@pytest.mark.parametrize("up,down", [(147, 320), (320, 147), (1, 1), (1, 8), (8, 1)])
def test_adjoint_identity_of_the_numpy_resampler_pair(up, down):
  rng = np.random.default_rng(up * 1000 + down)
  n_in = 700
  x = rng.standard_normal(n_in)
  y = lo.resample_forward(x, up, down)
  g = rng.standard_normal(len(y))
  d = lo.resample_backward(g, n_in, up, down)
  lhs, rhs = float(np.dot(y, g)), float(np.dot(x, d))
  scale = float(np.sum(np.abs(y) * np.abs(g)))
  print(up, down, lhs, rhs, abs(lhs - rhs) / scale)
  assert abs(lhs - rhs) <= 1e-13 * scale
  if up == down:
    assert d.tobytes() == g.tobytes()


@pytest.mark.parametrize("up,down", [(147, 320), (320, 147), (2, 1), (1, 8)])
def test_polyphase_table_backward_index_by_index(up, down):
  from waveglow_amd import resample
  half, h = lo.plan(up, down)
  t = resample.polyphase_table_backward(down, half, h)
  Kt = -(-(2 * half + 1) // down)
  assert t.shape == (down, Kt) and t.dtype == np.float64 and t.flags["C_CONTIGUOUS"]
  for r in range(down):
    for i in range(Kt):
      k = r + i * down
      assert t[r, i] == (h[k] if k <= 2 * half else 0.0), (r, i)
  # one input sample reads one row ascending in n
  m = 5
  c = half - m * up
  r = c % down
  n0 = (r - c) // down
  for i in range(Kt):
    k = half + (n0 + i) * down - m * up
    assert k == r + i * down


def test_new_entry_points_validate_arguments_without_a_gpu():
  from waveglow_amd import _lib, build
  build.build_library()
  lib = _lib.load()
  assert lib.wg_stoi_saved_bytes(0, 20000) == 0 and lib.wg_stoi_backward_workspace_bytes(0, 20000) == 0
  for B, n in ((-1, 20000), (65536, 20000), (1, 0), (1, (1 << 21) + 1)):
    assert lib.wg_stoi_saved_bytes(B, n) == 0 and lib.wg_stoi_backward_workspace_bytes(B, n) == 0
  # counts, kept lists of 155 frames, both band spectra of 154 frames
  assert lib.wg_stoi_saved_bytes(1, 20000) >= 16 + 155 * 4 + 2 * 15 * 154 * 8
  assert lib.wg_stoi_saved_bytes(2, 20000) < lib.wg_stoi_workspace_bytes(2, 20000) + 4096
  # 125 segment blocks, band gradients, frame gradients
  assert lib.wg_stoi_backward_workspace_bytes(1, 20000) >= 125 * 450 * 8 + 15 * 154 * 8 + 154 * 256 * 8
  dummy = (C.c_char * 128)()
  p = (C.addressof(dummy) + 15) & ~15
  big = 1 << 40
  ok = _lib.WgStoiParams(p, p, p)
  fwd = lambda *a: lib.wg_stoi_forward(*a)
  assert fwd(p, p, p, p, 1, 20000, C.byref(ok), p, p, 64, p, big, None) == -4 and b"saved" in lib.wg_last_error()
  assert fwd(p, p, p, p, 1, 20000, C.byref(ok), p, p, big, p, 64, None) == -4
  for i in (0, 1, 2, 3, 7, 8, 10):
    args = [p, p, p, p, 1, 20000, C.byref(ok), p, p, big, p, big, None]
    args[i] = None
    assert fwd(*args) == -1 and b"null" in lib.wg_last_error(), i
  assert fwd(p, p, p, p, 1, 20000, None, p, p, big, p, big, None) == -1
  assert fwd(p, p, p, p, 1, 20000, C.byref(_lib.WgStoiParams(p, None, p)), p, p, big, p, big, None) == -1
  assert fwd(p, p, p, p, 1, 20000, C.byref(_lib.WgStoiParams(p, p, p + 8)), p, p, big, p, big, None) == -1
  assert b"aligned" in lib.wg_last_error()
  assert fwd(p, p, p, p, 1, 20000, C.byref(ok), p, p + 4, big, p, big, None) == -1 and b"aligned" in lib.wg_last_error()
  bwd = lambda *a: lib.wg_stoi_backward(*a)
  assert bwd(p, 1, 20000, C.byref(ok), p, p, 64, p, p, big, None) == -4
  assert bwd(p, 1, 20000, C.byref(ok), p, p, big, p, p, 64, None) == -4 and b"workspace" in lib.wg_last_error()
  for i in (0, 4, 5, 7, 8):
    args = [p, 1, 20000, C.byref(ok), p, p, big, p, p, big, None]
    args[i] = None
    assert bwd(*args) == -1 and b"null" in lib.wg_last_error(), i
  assert bwd(p, 1, 20000, None, p, p, big, p, p, big, None) == -1
  for B, n in ((0, 20000), (65536, 20000), (1, 0), (1, (1 << 21) + 1)):
    assert fwd(p, p, p, p, B, n, C.byref(ok), p, p, big, p, big, None) == -1 and b"stoi" in lib.wg_last_error()
    assert bwd(p, B, n, C.byref(ok), p, p, big, p, p, big, None) == -1 and b"stoi" in lib.wg_last_error()
  # the transposed resampler
  rb = lambda *a: lib.wg_resample_backward(*a)
  F32, F64 = _lib.WG_PCM_F32, _lib.WG_PCM_F64
  assert (_lib.WG_PCM_I16, F32, F64) == (0, 1, 2)
  for i in (0, 2, 3, 4):
    args = [p, F64, p, p, p, 200, 441, 4410, 1, 1000, 454, None]
    args[i] = None
    assert rb(*args) == -1 and b"null" in lib.wg_last_error(), i
  assert rb(p, _lib.WG_PCM_I16, p, p, p, 200, 441, 4410, 1, 1000, 454, None) == -1 and b"dtype" in lib.wg_last_error()
  assert rb(p, 3, p, p, p, 200, 441, 4410, 1, 1000, 454, None) == -1
  for up, down, half, B, n_in, n_out in ((0, 441, 4410, 1, 1000, 454), (200, 0, 4410, 1, 1000, 454),
                                         (400, 882, 4410, 1, 1000, 454),          # not reduced
                                         (1025, 1, 10250, 1, 1000, 1025000), (200, 441, -1, 1, 1000, 454),
                                         (200, 441, 4410, 0, 1000, 454), (200, 441, 4410, 1, 0, 454),
                                         (200, 441, 4410, 1, (1 << 26) + 1, 1 << 30),
                                         (200, 441, 4410, 1, 1000, 453)):         # n_out below out_len(n_in) = 454
    assert rb(p, F32, p, p, p, up, down, half, B, n_in, n_out, None) == -1, (up, down, half, B, n_in, n_out)
    assert b"resample" in lib.wg_last_error()


def test_python_layer_refuses_bad_arguments_before_any_launch():
  import waveglow_amd
  from waveglow_amd import _lib, metrics, resample, stoi_loss
  assert waveglow_amd.STOILoss is stoi_loss.STOILoss
  x = torch.zeros((2, 4000))
  for call in (lambda: resample.resample_differentiable(x, None, 22050, 10000),                 # a CPU tensor
               lambda: resample.resample_differentiable(x, None, 22050, 10000, clip=True),
               lambda: resample.resample_differentiable(x.requires_grad_(False).to(torch.int16), None, 22050, 10000),
               lambda: metrics.stoi_differentiable(x, None, x, None),
               lambda: metrics.stoi_differentiable(x.clone().requires_grad_(True), None, x, None),   # the clean side
               lambda: stoi_loss.STOILoss(sampling_rate=10001),
               lambda: stoi_loss.STOILoss(sampling_rate=22050.5),
               lambda: stoi_loss.STOILoss(sampling_rate=0),
               lambda: stoi_loss.STOILoss(device="cpu")):
    with pytest.raises(_lib.WgError):
      call()
  with pytest.raises(_lib.WgError, match="clean side"):
    metrics.stoi_differentiable(x.clone().requires_grad_(True), None, x, None)
  crit = stoi_loss.STOILoss()
  assert (crit.sampling_rate, crit.factor_stoi, crit.factor_estoi) == (22050, 1.0, 0.0)
  for call in (lambda: crit(x, x), lambda: crit.scores(x, x),                                    # CPU tensors
               lambda: crit(x.double(), x.double()), lambda: crit(x[0], x[0]), lambda: crit([0.0], x)):
    with pytest.raises(_lib.WgError):
      call()
  # what a forward keeps: the processed side at 10 kHz and the saved buffer
  n10 = resample.out_len(22050, 200, 441)
  assert crit.workspace_bytes(4, 22050) == 4 * 4 * n10 + metrics.stoi_saved_bytes(4, n10) > 0
  assert crit.workspace_bytes(0, 22050) == 0
  assert stoi_loss.STOILoss(sampling_rate=10000).workspace_bytes(1, 4224) == 4 * 4224 + metrics.stoi_saved_bytes(1, 4224)
