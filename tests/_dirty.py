"""Shared by tests/test_gpu_dirty_workspace.py, tests/test_gpu_workspace_reuse.py and tests/test_dirty_cpu.py: no result of
the library may depend on what a workspace, a saved-state buffer or an output buffer held before the call (DESIGN.md
section 4, "What a workspace holds before a call").

The Python layer gets every such buffer from ``torch.empty`` (or from a cache).  In a short test process a new allocation is
usually zero pages, so a kernel that reads a region before anything has written it passes there and is wrong in a
long-running job.  ``poisoned_allocations`` makes the allocations of a test start from a chosen byte pattern instead:

  pattern   uint8 buffer read as   fp16     fp32       fp64       int32
  0x00      (clean)                0        0          0          0
  0xFF                             NaN      NaN        NaN        -1
  0x47                             7.28     51015.3    ~2.4e35    0x47474747

0x47 stands beside 0xFF because ``max``, ``x > 0 ? x : 0`` and a ``<`` comparison swallow a NaN; a large finite value
goes through them.  Floating tensors (outputs, packed weights, gradient buffers) start from NaN under both dirty patterns
and from 0 under the clean one.  Integer tensors other than uint8, and every host tensor, are left alone.

``ENTRY_POINTS`` names, for every C function of include/waveglow_amd.h that takes a ``workspace`` or a ``saved`` buffer,
the GPU tests that reach it; tests/test_dirty_cpu.py holds the table to the header, so a new entry point fails there until
a test covers it.
"""
import contextlib

import torch

CLEAN, ONES, FINITE = 0x00, 0xFF, 0x47
PATTERNS = (CLEAN, ONES, FINITE)


def _poison(t, pattern):
  if not isinstance(t, torch.Tensor) or not t.is_cuda or t.numel() == 0:
    return t
  if t.dtype == torch.uint8:
    t.fill_(pattern)
  elif t.dtype.is_floating_point:
    t.fill_(0.0 if pattern == CLEAN else float("nan"))
  return t


@contextlib.contextmanager
def poisoned_allocations(monkeypatch, pattern):
  """``torch.empty`` and ``torch.empty_like`` give poisoned GPU tensors inside the block (module docstring).  The wrappers of
  waveglow_amd look ``torch.empty`` up at call time, so nothing of the product changes for this."""
  assert pattern in PATTERNS, pattern
  empty, empty_like = torch.empty, torch.empty_like

  def poisoned_empty(*args, **kwargs):
    return _poison(empty(*args, **kwargs), pattern)

  def poisoned_empty_like(*args, **kwargs):
    return _poison(empty_like(*args, **kwargs), pattern)

  with monkeypatch.context() as m:
    m.setattr(torch, "empty", poisoned_empty)
    m.setattr(torch, "empty_like", poisoned_empty_like)
    yield


def dirty_cached(engine, pattern):
  """Fills what an inference engine keeps between calls: the cached workspaces of ``_Engine._ws`` and the workspace of
  every captured-graph entry of ``_Engine._graphs``.  The training pool (``_train_pool``) is not touched: its slots hold
  saved state by contract (tests/test_gpu_workspace_reuse.py).  Returns the number of buffers filled."""
  n = 0
  for ws in engine._ws.values():
    ws.fill_(pattern)
    n += 1
  for ent in engine._graphs.values():
    ent[3].fill_(pattern)
    n += 1
  return n


def raw(t):
  """The bytes of a tensor as a flat uint8 tensor on its device."""
  return t.detach().contiguous().reshape(-1).view(torch.uint8)


def same_bytes(a, b, what):
  """Raw bytes, so NaNs compare equal and -0.0 differs from 0.0."""
  assert a.shape == b.shape and a.dtype == b.dtype, f"{what}: {tuple(a.shape)} {a.dtype} against {tuple(b.shape)} {b.dtype}"
  x, y = raw(a), raw(b.to(a.device))
  if not torch.equal(x, y):
    size = a.element_size()
    bad = torch.nonzero((x != y).reshape(-1, size).any(1)).flatten()
    nan = int(torch.isnan(a).sum()) if a.dtype.is_floating_point else 0
    raise AssertionError(f"{what}: {bad.numel()} of {a.numel()} entries differ, flat index {int(bad[0])} .. {int(bad[-1])}; "
                         f"{nan} entries are NaN")


def snapshot(out):
  """{name: tensor} -> the same with every tensor cloned (a later call may reuse its memory)."""
  return {q: t.detach().clone() for q, t in out.items()}


def same_outputs(a, b, what):
  assert list(a) == list(b), f"{what}: {sorted(set(a) ^ set(b))}"
  for q in a:
    same_bytes(a[q], b[q], f"{what}: {q}")


def four_runs(monkeypatch, call, what, excluded=()):
  """``call()`` -- one whole call on objects of its own, {name: tensor} -- under the three patterns and once with no hook:
  every output has the same bytes in all four runs.  ``call`` may take the pattern as its argument (None for the run
  without a hook).  ``excluded``: names left out of the comparison (parts the header documents as left unwritten).
  Returns the outputs of the run without a hook."""
  import inspect
  takes = len(inspect.signature(call).parameters) == 1
  runs = []
  for p in PATTERNS:
    with poisoned_allocations(monkeypatch, p):
      runs.append(snapshot(call(p) if takes else call()))
      torch.cuda.synchronize()
  assert torch.empty.__name__ == "empty"
  plain = snapshot(call(None) if takes else call())
  torch.cuda.synchronize()
  for p, out in zip(PATTERNS, runs):
    same_outputs({q: t for q, t in out.items() if q not in excluded}, {q: t for q, t in plain.items() if q not in excluded},
                 f"{what}: allocations of 0x{p:02X} against plain allocations")
  return plain


G = "tests/test_gpu_dirty_workspace.py::"
R = "tests/test_gpu_workspace_reuse.py::"

# C function -> the GPU tests that reach it.  A call with per-utterance lengths is the dense call with a non-null `frames` /
# `lens`: one row each, naming the tests that run it both ways.  wg_loss (the loss with log_det_W as host floats) has no
# Python caller and is called through ctypes by its test.
ENTRY_POINTS = {
  "wg_infer": (G + "test_inference", G + "test_inference_graph_replays"),
  "wg_forward": (G + "test_no_grad_forward_and_likelihood",),
  "wg_nll": (G + "test_no_grad_forward_and_likelihood",),
  "wg_loss": (G + "test_no_grad_forward_and_likelihood",),
  "wg_loss_dev": (G + "test_no_grad_forward_and_likelihood", G + "test_training_step_on_a_new_slot"),
  "wg_stft_denoise": (G + "test_denoiser",),
  "wg_stft_mel": (G + "test_mel_front_end",),
  "wg_stft_mel_forward_saved": (G + "test_mel_front_end_gradient",),
  "wg_stft_mel_backward": (G + "test_mel_front_end_gradient",),
  "wg_wav_finish": (G + "test_outputs_without_a_workspace",),
  "wg_metrics_mfcc": (G + "test_mel_metrics",),
  "wg_metrics_mel": (G + "test_mel_metrics",),
  "wg_pitch_metrics": (G + "test_pitch_metrics",),
  "wg_stoi": (G + "test_stoi",),
  "wg_stoi_forward": (G + "test_stoi_loss",),
  "wg_stoi_backward": (G + "test_stoi_loss",),
  "wg_stftloss_forward": (G + "test_stft_loss",),
  "wg_stftloss_backward": (G + "test_stft_loss",),
  "wg_train_forward": (G + "test_training_step_on_a_new_slot", R + "test_alternating_directions_on_one_slot"),
  "wg_train_backward": (G + "test_training_step_on_a_new_slot", R + "test_alternating_directions_on_one_slot"),
  "wg_train_infer_forward": (G + "test_infer_differentiable", R + "test_alternating_directions_on_one_slot"),
  "wg_train_infer_backward": (G + "test_infer_differentiable", R + "test_alternating_directions_on_one_slot"),
}
