"""Golden audio gradients of the denoiser from the REFERENCE's own ``STFT`` and ``Denoiser`` classes under autograd (build
container only).

  python tests/golden/make_golden_denoiser_grads.py            # writes tests/golden/denoiser_grads.npz
  python tests/golden/make_golden_denoiser_grads.py --search   # prints input seeds at which the clamp margin holds

``_ref_import.import_reference_stft`` (through make_golden_stft.py) imports the reference's classes with functional stand-ins for the librosa names
(see make_golden_stft.py).  The reference ``Denoiser`` is built on a stand-in vocoder (its bias is then overwritten with
the stored one: the gradient under test does not involve the vocoder) and run in fp32 on the CPU:
``L = <r, Denoiser.forward(x, s)>``, ``L.backward()``, ``x.grad`` stored.  ``STFT.transform`` detaches the phase
(stft.py:160-161), so this is the gradient ``forward_differentiable(phase_grad=False)`` restates.  No input has a silent
frame: the reference's sqrt gives NaN there.

Cases, keys and the quantised inputs: tests/_denoiser_grad_oracle.py.  Data only; the archive is written with fixed time
stamps, so two runs give the same bytes.
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.abspath(os.path.join(HERE, "..")))
sys.path.insert(0, os.path.abspath(os.path.join(HERE, "..", "..")))
import _denoiser_grad_oracle as D  # noqa: E402
from _corners import pack_f32  # noqa: E402

SIZE_LIMIT = os.path.getsize(os.path.join(HERE, "flow_corners.npz"))   # make_golden_stft.py's limit

NOTES = ("d <r, Denoiser.forward(x, s)> / d x from the reference's own STFT and Denoiser classes under torch autograd, fp32 "
         "on the CPU, with functional stand-ins for librosa.util.pad_center / tiny / normalize(norm=None).  The Denoiser's "
         "bias_spec is overwritten with the stored bias.  STFT.transform detaches the phase, so the gradient follows the "
         "magnitude path only.")


def search():
  bias = D.make_bias()
  half = dict(D.STRENGTHS)["shalf"]
  found = {}
  cases = [(f"N{N}", D.DENSE_B, N) for N in D.DENSE_N] + [("gap", D.DENSE_B, D.GAP_N)]
  for name, B, N in cases:
    for seed in range(10000):
      x = D.make_input(name, B, N, seed)[1]
      if name == "gap":
        x[:, D.GAP[0]:D.GAP[1]] = 0.0
      if D.clamp_margin(x, bias, half)[0] >= D.MARGIN:
        found[name] = seed
        break
  for seed in range(10000):
    x = D.make_input("ragged", len(D.RAGGED_LENS), D.RAGGED_PITCH, seed)[1]
    if all(D.clamp_margin(x[b:b + 1, :n], bias, half)[0] >= D.MARGIN for b, n in enumerate(D.RAGGED_LENS)):
      found["ragged"] = seed
      break
  print("SEEDS =", found)


class _Vocoder:
  """What ``Denoiser.__init__`` asks of a vocoder; the bias it yields is replaced below."""

  class _Up:
    weight = torch.zeros(1)

  upsample = _Up()

  @staticmethod
  def infer(mel, sigma):
    return torch.randn(1, 256 * mel.shape[2], generator=torch.Generator().manual_seed(0)) * 0.01


def main():
  from make_golden_stft import ref_denoiser, ref_taco, write_npz   # imports the reference through _ref_import
  cpu = torch.device("cpu")
  den = ref_denoiser.Denoiser(_Vocoder(), ref_taco.TSTFTHParams(), "zeros", cpu)
  bias = D.make_bias()
  assert den.bias_spec.shape == (1, D.CUT, 1)
  den.bias_spec.copy_(torch.from_numpy(bias)[None, :, None])
  out = {"notes": np.array(NOTES), "bias": pack_f32(bias)}
  for N in D.DENSE_N:
    name = f"N{N}"
    xq, x = D.make_input(name, D.DENSE_B, N)
    rq, r = D.make_weights(name, D.DENSE_B, N)
    out[f"{name}/x_q"], out[f"{name}/r_q"] = xq, rq
    for sname, s in D.STRENGTHS:
      xg = torch.from_numpy(x).clone().requires_grad_(True)
      y = den(xg, s)
      assert y.shape == (D.DENSE_B, 1, N) and y.dtype == torch.float32
      (y[:, 0, :] * torch.from_numpy(r)).sum().backward()
      g = xg.grad.numpy()
      assert g.shape == (D.DENSE_B, N) and np.isfinite(g).all(), (name, sname)
      is_zero = not g.any()
      out[f"{name}/{sname}/is_zero"] = np.array(is_zero)
      if not is_zero:
        out[f"{name}/{sname}/grad"] = pack_f32(g)
      margin, clamped = D.clamp_margin(x, bias, s)
      print(f"{name} {sname}: |g| {np.linalg.norm(g.astype(np.float64)):.4e}, {100 * clamped:.1f} % of the cells clamp, "
            f"margin {margin:.2e}{'  EXACT ZEROS' if is_zero else ''}")
      assert is_zero == (s == 1e4)
  write_npz(D.FIXTURE, out)
  size = os.path.getsize(D.FIXTURE)
  print("wrote", D.FIXTURE, size, "bytes (limit", SIZE_LIMIT, ")")
  assert size <= SIZE_LIMIT


if __name__ == "__main__":
  torch.set_num_threads(8)
  if "--search" in sys.argv[1:]:
    search()
  else:
    main()
