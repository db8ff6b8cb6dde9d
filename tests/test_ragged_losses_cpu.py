"""CPU: the fp64 yardstick of the waveform losses with per-utterance lengths (tests/_ragged_ref.py), the host-side
length check, and the argument checks of the ragged C entry points on a planning handle.

The cases of ``_ragged_ref.CASES``:
  default      N = 4099, lens (1025, 2500, 4099): 1025 is the minimum for n_fft = 2048, where the head and tail
               reflections overlap; at hop 50 the first utterance's second 64-frame tile lies wholly behind it, the
               second's partly
  fft64-hop7   N = 1000, lens (33, 450, 1000): three frame tiles, a hop that does not divide the lengths
  hop-is-fft   N = 6200, lens (1025, 4096, 6200): hop = n_fft = 2048, one to four frames
"""
import ctypes as C

import pytest
import torch

from _ragged_ref import CASE_IDS, CASES, inputs, ragged_grad64, ragged_ref64, ragged_unfold
from test_stft_loss_cpu import grad_ref64, loss_ref64, rel
from waveglow_amd import _lib, build
from waveglow_amd.stft_loss import check_lengths


@pytest.mark.parametrize("silent", [False, True])
@pytest.mark.parametrize("res,N,lens", CASES, ids=CASE_IDS)
def test_crop_reference_agrees_with_its_unfold_restatement(res, N, lens, silent):
  """The bounds of test_two_fp64_restatements_agree: spectral convergence to 1e-8, the log-magnitude term at the default
  eps to 1e-5 (near-empty bins see the fp32 rounding of the basis), the SC gradient to 1e-6.  Everything is finite."""
  x, y = (t.double() for t in inputs(N, lens, silent))
  a, b = ragged_ref64(x, y, lens, res), ragged_unfold(x, y, lens, res)
  assert all(torch.isfinite(v) for v in a)
  assert abs(float(a[0]) - float(b[0])) <= 1e-8 * abs(float(a[0]))
  assert abs(float(a[1]) - float(b[1])) <= 1e-5 * abs(float(a[1]))
  ga = ragged_grad64(x, y, lens, res, factor_mag=0.0)
  gb = ragged_grad64(x, y, lens, res, factor_mag=0.0, fn=ragged_unfold)
  assert torch.isfinite(ga).all() and rel(gb, ga) <= 1e-6


@pytest.mark.parametrize("silent", [False, True])
@pytest.mark.parametrize("res,N,lens", CASES, ids=CASE_IDS)
def test_equal_lengths_reproduce_the_dense_reference(res, N, lens, silent):
  """The same terms summed per utterance instead of per batch: fp64 rounding of sums of up to 3e5 terms, bound 1e-12
  relative (measured 6e-16); the gradients agree to 1e-10."""
  x, y = inputs(N, lens, silent)
  full = (N,) * len(lens)
  for u, v in zip(ragged_ref64(x, y, full, res), loss_ref64(x, y, res)):
    assert abs(float(u) - float(v)) <= 1e-12 * abs(float(v))
  assert rel(ragged_grad64(x, y, full, res), grad_ref64(x, y, res)) <= 1e-10


@pytest.mark.parametrize("silent", [False, True])
@pytest.mark.parametrize("res,N,lens", CASES, ids=CASE_IDS)
def test_reference_gradient_behind_each_length_is_zero(res, N, lens, silent):
  x, y = inputs(N, lens, silent)
  g = ragged_grad64(x, y, lens, res)
  assert torch.isfinite(g).all()
  for b, n in enumerate(lens):
    assert not g[b, n:].any() and g[b, :n].abs().max() > 0


def test_check_lengths():
  assert check_lengths([1025, 4096], 2, 4096, 1024) == [1025, 4096]
  assert check_lengths((1025, 4096), 2, 4096, 1024) == [1025, 4096]
  assert check_lengths(torch.tensor([1025, 4096]), 2, 4096, 1024) == [1025, 4096]
  assert check_lengths(torch.tensor([1025, 4096], dtype=torch.int32), 2, 4096, 1024) == [1025, 4096]
  for bad, word in (([1025], "1 lengths"), ([1025, 4096, 2000], "3 lengths"),        # wrong count
                    ([1024, 4096], "1024"), ([1025, 4097], "4097"), ([2000, 0], "lengths[1] = 0"),
                    ([2000, -5], "-5"), ([2000.0, 4096], "2000.0"), ([2000, "x"], "'x'"), ([True, 2000], "True"),
                    (torch.tensor([2000.0, 4096.0]), "float32"), (torch.tensor([[2000, 4096]]), "shape"),
                    (torch.tensor([2000, 5000]), "5000"), (2000, "int"), (None, "NoneType")):
    with pytest.raises(_lib.WgError) as e:
      check_lengths(bad, 2, 4096, 1024)
    assert word in str(e.value), (bad, str(e.value))


@pytest.fixture(scope="module")
def lib():
  build.build_library()
  return _lib.load()


def test_ragged_entry_points_validate_arguments_without_a_gpu(lib):
  """One order of argument checks, with lens or without (a null lens is the dense batch): null arguments, then sizes, then
  the workspace size, and only then the refusal of the planning handle (device_id < 0)."""
  n_fft, hop, win = (1024, 2048, 512), (120, 240, 50), (600, 1200, 240)
  arr = lambda v: (C.c_int32 * len(v))(*v)
  h = C.c_void_p()
  assert lib.wg_stftloss_create(3, arr(n_fft), arr(hop), arr(win), None, 1e-7, -1, C.byref(h)) == 0
  dummy = (C.c_char * 64)()
  p = C.addressof(dummy)
  need = lib.wg_stftloss_workspace_bytes(h, 2, 4096, 1)
  assert need > 0
  # (h, audio, target, lens, factor_sc, factor_mag, out3, B, n_samples, saved, workspace, workspace_bytes, stream)
  fwd = lib.wg_stftloss_forward
  for saved in (0, 1):
    need = lib.wg_stftloss_workspace_bytes(h, 2, 4096, saved)
    assert fwd(h, None, p, p, 1.0, 1.0, p, 2, 4096, saved, p, need, None) == -1 and b"null" in lib.wg_last_error()
    assert fwd(None, p, p, p, 1.0, 1.0, p, 2, 4096, saved, p, need, None) == -1
    for lens in (p, None):
      assert fwd(h, p, p, lens, 1.0, 1.0, p, 2, 1024, saved, p, need, None) == -1 and b"n_samples" in lib.wg_last_error()
      assert fwd(h, p, p, lens, 1.0, 1.0, p, 0, 4096, saved, p, need, None) == -1
      assert fwd(h, p, p, lens, 1.0, 1.0, p, 2, 4096, saved, p, need - 1, None) == -4 and b"workspace" in lib.wg_last_error()
      # sound arguments: the planning handle is refused, with a null lens exactly as with one
      assert fwd(h, p, p, lens, 1.0, 1.0, p, 2, 4096, saved, p, need, None) == -2 and b"planning" in lib.wg_last_error()
  for lens in (p, None):
    for saved in (2, -1):                            # `saved` is the flag of wg_stftloss_workspace_bytes: 0 or 1
      assert fwd(h, p, p, lens, 1.0, 1.0, p, 2, 4096, saved, p, need, None) == -1 and b"saved" in lib.wg_last_error()
  # (h, g_out3, lens, factor_sc, factor_mag, audio_grad_out, B, n_samples, workspace, workspace_bytes, stream)
  bwd = lib.wg_stftloss_backward
  assert bwd(h, None, p, 1.0, 1.0, p, 2, 4096, p, need, None) == -1 and b"null" in lib.wg_last_error()
  for lens in (p, None):
    assert bwd(h, p, lens, 1.0, 1.0, None, 2, 4096, p, need, None) == -1
    assert bwd(h, p, lens, 1.0, 1.0, p, 2, 1024, p, need, None) == -1 and b"n_samples" in lib.wg_last_error()
    assert bwd(h, p, lens, 1.0, 1.0, p, 2, 4096, p, need - 1, None) == -4
    assert bwd(h, p, lens, 1.0, 1.0, p, 2, 4096, p, need, None) == -2 and b"planning" in lib.wg_last_error()
  assert lib.wg_stftloss_destroy(h) == 0
  # mel gradients: null arguments are refused before anything else; a null lens is not one of them (the dense batch) and
  # gets the answer of the call with lens.  Compared at the last refusal that needs no device, a workspace one byte short:
  # past it the call enqueues work.
  # (h, mel_basis, n_mel, audio / g_mel, lens, mel_out / audio_grad_out, B, n_samples, workspace, workspace_bytes, stream)
  need = lib.wg_stft_mel_grad_workspace_bytes(p, 2, 4096)
  assert need > 0
  for fn in (lib.wg_stft_mel_forward_saved, lib.wg_stft_mel_backward):
    assert fn(None, p, 80, p, p, p, 2, 4096, p, need, None) == -1 and b"null" in lib.wg_last_error()
    assert fn(p, p, 80, None, p, p, 2, 4096, p, need, None) == -1 and b"null" in lib.wg_last_error()
    answers = []
    for lens in (p, None):
      answers.append((fn(p, p, 80, p, lens, p, 2, 4096, p, need - 1, None), lib.wg_last_error()))
    assert answers[0] == answers[1] and answers[0][0] == -4 and b"workspace" in answers[0][1]
