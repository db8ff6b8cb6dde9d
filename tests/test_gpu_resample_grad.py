"""The transposed resampler on the device (``wg_resample_backward``, ``resample.resample_differentiable``) against its
numpy restatement (tests/_stoi_loss_oracle.py: resample_backward).

The bound per element is ``2^-24 |g| + 1e-12 sum|h| max|d_out|``: one rounding of the result to fp32, plus an allowance for
the order of the fp64 sum (the restatement uses ``np.dot``), four orders above what an fp64 sum of at most a few hundred
terms can lose.  Ratios: both directions of 147 / 320, the copy, 1 / 8 (the forward's unstaged variant) and 8 / 1 (the
backward's unstaged variant: a tile of 1024 inputs then spans more output gradients than a workgroup stages)."""
import numpy as np
import pytest
import torch

import _resample_oracle
import _stoi_loss_oracle as lo
from waveglow_amd import _lib, resample

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
RATIOS = [(147, 320), (320, 147), (1, 1), (1, 8), (8, 1)]                      # (up, down)
N_IN = 2100
LENS = (1023, 1025, 2100, 0)                                                   # around the 1024-input tile edge; an empty row


def _gradients(up, down, dtype, seed=3):
  """(d_out [B, n_out] of `dtype` with NaN behind every row's outputs, the per-row valid counts)."""
  n_out = _resample_oracle.out_len(N_IN, up, down) + 5                         # a pitch above out_len(n_in)
  rng = np.random.default_rng(seed + up)
  g = rng.standard_normal((len(LENS), n_out)).astype(dtype)
  olens = [_resample_oracle.out_len(n, up, down) for n in LENS]
  for b, n in enumerate(olens):
    g[b, n:] = np.nan
  return g, olens


def _device(g, up, down, lens=LENS, n_in=N_IN):
  lens_dev = torch.tensor(lens, dtype=torch.int32).to(DEV)
  out = resample.resample_backward_enqueue(torch.from_numpy(g).to(DEV), lens_dev, down, up, n_in)      # sr_out / sr_in = up / down
  assert out.dtype == torch.float32 and tuple(out.shape) == (len(lens), n_in)
  return out.cpu().numpy()


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("up,down", RATIOS)
def test_backward_equals_the_numpy_restatement(up, down, dtype):
  assert resample.resample_plan(down, up)[:2] == (up, down)
  g, olens = _gradients(up, down, dtype)
  got = _device(g, up, down)
  assert not np.isnan(got).any()
  half, h = lo.plan(up, down)
  worst = 0.0
  for b, n in enumerate(LENS):
    assert not got[b, n:].any(), "the gradient behind a row's length must be exactly zero"
    if n == 0:
      continue
    ref = lo.resample_backward(g[b, :olens[b]].astype(np.float64), n, up, down)
    tol = 2.0 ** -24 * np.abs(ref) + 1e-12 * float(np.abs(h).sum()) * float(np.max(np.abs(g[b, :olens[b]])))
    dist = np.abs(got[b, :n].astype(np.float64) - ref)
    worst = max(worst, float(np.max(dist / tol)))
    assert (dist <= tol).all(), (b, float(np.max(dist)), float(np.max(tol)))
    # the row's own call with B = 1 at another pitch gives the same bits
    own = _device(np.ascontiguousarray(g[b:b + 1, :olens[b]]), up, down, lens=(n,), n_in=n)
    assert own.tobytes() == got[b, :n].tobytes(), b
  print(f"{up}/{down} {np.dtype(dtype).name}: largest distance / bound {worst:.3f}")
  if up == down:
    assert got[2].tobytes() == g[2, :N_IN].astype(np.float32).tobytes()        # the copy


def test_variants_are_the_ones_the_ratios_were_chosen_for():
  assert resample.kernel_plan(320, 147)[2] and resample.kernel_plan(147, 320)[2]
  assert not resample.kernel_plan(8, 1)[2]                                     # 1 / 8: the forward reads through the cache
  # the backward stages at most 4096 gradients: 1023 up / down + Kt + 1 of them per tile
  span = lambda up, down: (1023 * up + down - 1) // down + -(-(20 * max(up, down) + 1) // down) + 1
  assert span(8, 1) > 4096 >= max(span(147, 320), span(320, 147), span(1, 8))


@pytest.mark.parametrize("up,down", RATIOS)
def test_adjoint_identity_on_the_device(up, down):
  """<resample(x), g> = <x, resample_backward(g)> with both sides' device results taken to fp64 on the host: each side is
  off by one fp32 rounding per element, 2^-24 sum |terms|, plus the fp64 sums' own rounding."""
  rng = np.random.default_rng(17)
  x = rng.standard_normal((1, N_IN)).astype(np.float32)
  xt = torch.from_numpy(x).to(DEV)
  y, (olen,) = resample.resample(xt, [N_IN], down, up)
  y = y.cpu().numpy()[0, :olen].astype(np.float64)
  g = rng.standard_normal((1, olen))
  d = _device(g, up, down, lens=(N_IN,))[0].astype(np.float64)
  lhs, rhs = float(np.dot(y, g[0])), float(np.dot(x[0].astype(np.float64), d))
  bound = (2.0 ** -24 + 1e-12) * float(np.sum(np.abs(y * g[0])) + np.sum(np.abs(x[0] * d)))
  print(f"{up}/{down}: {lhs!r} against {rhs!r}, distance {abs(lhs - rhs):.3e}, bound {bound:.3e}")
  assert abs(lhs - rhs) <= bound


def test_resample_differentiable():
  rng = np.random.default_rng(23)
  x = torch.from_numpy(rng.standard_normal((2, 3000)).astype(np.float32)).to(DEV)
  x[1, 2500:] = float("nan")
  lens = [3000, 2500]
  plain, plain_lens = resample.resample(x, lens, 22050, 10000)
  # no graph without grad mode or without a leaf that wants one
  out, out_lens = resample.resample_differentiable(x, lens, 22050, 10000)
  assert out.grad_fn is None and not out.requires_grad and torch.equal(out, plain) and out_lens == plain_lens
  leaf = x.clone().requires_grad_(True)
  with torch.no_grad():
    out, _ = resample.resample_differentiable(leaf, lens, 22050, 10000)
  assert out.grad_fn is None and not out.requires_grad
  out, out_lens = resample.resample_differentiable(leaf, lens, 22050, 10000)
  assert out.grad_fn is not None and torch.equal(out.detach(), plain) and out_lens == plain_lens
  g = torch.from_numpy(rng.standard_normal(tuple(out.shape)).astype(np.float32)).to(DEV)
  (out * g).sum().backward(retain_graph=True)
  first = leaf.grad.clone()
  leaf.grad = None
  (out * g).sum().backward()
  assert torch.equal(first, leaf.grad), "a second backward under retain_graph must give the same bits"
  lens_dev = torch.tensor(lens, dtype=torch.int32).to(DEV)
  assert torch.equal(first, resample.resample_backward_enqueue(g, lens_dev, 22050, 10000, 3000))
  assert not torch.isnan(first).any() and not first[1, 2500:].any() and first[1, :2500].any()
  with pytest.raises(_lib.WgError):
    resample.resample_differentiable(torch.zeros((2, 3000), dtype=torch.int16, device=DEV), lens, 22050, 10000)
  with pytest.raises(_lib.WgError):
    resample.resample_differentiable(leaf, lens, 22050, 10001)
  with pytest.raises(_lib.WgError):
    resample.resample_differentiable(leaf, lens, 22050, 10000, clip=True)      # there is no clipped variant
