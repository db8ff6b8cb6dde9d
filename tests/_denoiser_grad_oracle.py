"""fp64 restatement of ``Denoiser.forward`` under autograd, and the cases of the denoiser-gradient tests (TEST
INFRASTRUCTURE; torch fp64 on the CPU), shared by tests/golden/make_golden_denoiser_grads.py,
tests/test_denoiser_grad_cpu.py and tests/test_gpu_denoiser_grad.py.

The restatement follows src/waveglow/stft.py:135-198 and src/waveglow/denoiser.py:51-57 with ``denoiser.stft_bases`` cast
to fp64: reflect padding, ``conv1d`` with the forward basis, magnitude, subtraction and clamp, recombination with the
phase, ``conv_transpose1d`` with the inverse basis, window-sum-square with its ``tiny`` threshold, the hop-ratio scale, the
crop.  ``phase_grad=True`` keeps the unit phasor X / |X| in the graph (the derivative of what is computed);
``phase_grad=False`` detaches it, as ``STFT.transform`` does (stft.py:160-161).  Every division is ``where``-guarded, so a
cell with |X| == 0 has the forward's value (max(-c, 0), 0) and gradient 0 where torch's sqrt would give NaN.

Keys of tests/golden/denoiser_grads.npz (fp32 arrays as byte planes: tests/_corners.py pack_f32, lossless):

  notes                  what the fixture holds
  bias                   the bias magnitudes [513], 1 + 5 |randn|: one for every case
  N<N>/x_q, N<N>/r_q     int16 [2, N]: input x = q / 32768 and loss weights r = q / 32768 (exact in fp32)
  N<N>/<strength>/grad   d <r, Denoiser.forward(x, s)> / d x [2, N] from the reference's own autograd; absent where it is 0
  N<N>/<strength>/is_zero   the reference's gradient was exactly 0 everywhere
"""
import os

import numpy as np
import torch
import torch.nn.functional as F

from waveglow_amd.denoiser import stft_bases

FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "denoiser_grads.npz")

FL, HOP, CUT = 1024, 256, 513
TINY = float(np.finfo(np.float32).tiny)

# N (B = 2): 1024 -> F = 5, every frame touches an edge, the reflections overlap, ws is partial everywhere;
# 8192 -> F = 33, one frame in the second 32-frame tile; 8448 -> F = 34
DENSE_N = (1024, 8192, 8448)
DENSE_B = 2
# one ragged batch: utterances ending before, at and behind the 32-frame tile seam, the longest not first
RAGGED_LENS = (1024, 8192, 2560)
RAGGED_PITCH = 8448
# strengths: none, the stored bias as it is (about half the cells clamp), every cell clamps
STRENGTHS = (("s0", 0.0), ("shalf", 1.0), ("s1e4", 1e4))
GAP_N, GAP = 8192, (1000, 3100)           # samples 1000 ... 3099 are zero: frames 6 ... 10 see silence only
GAP_SILENT_FRAMES = (6, 10)
GAP_ONLY_SILENT = (1792, 2304)            # output samples that frames 9 - 3 ... 10 alone reach
MARGIN = 1e-4                             # |mag - c| >= MARGIN max(mag, c) wherever mag > 0 (fp64), in every compared case

# seeds of the inputs, chosen on the CPU so that the clamp margin holds at strength "shalf" (make_golden_denoiser_grads.py
# --search prints them; tests/test_denoiser_grad_cpu.py asserts the margin)
SEEDS = {"N1024": 1, "N8192": 4, "N8448": 36, "gap": 4, "ragged": 6}


def quantise(x):
  """samples in (-1, 1) -> (int16 q, fp32 x' = q / 32768 exactly)."""
  q = np.clip(np.rint(np.asarray(x, dtype=np.float64) * 32768.0), -32768, 32767).astype(np.int16)
  return q, q.astype(np.float32) / np.float32(32768.0)


def make_bias():
  return (1.0 + np.abs(np.random.default_rng(999).standard_normal(CUT)) * 5.0).astype(np.float32)


def make_input(name, B, N, seed=None):
  """(x_q, x fp32 [B, N]) of case ``name``: 0.3 randn, quantised to int16 steps."""
  rng = np.random.default_rng([SEEDS[name] if seed is None else seed, N, B, 77])
  return quantise(0.3 * rng.standard_normal((B, N)))


def make_weights(name, B, N):
  """(r_q, r fp32 [B, N]): the weights of the loss L = <r, out>, uniform in (-1, 1) on int16 steps."""
  rng = np.random.default_rng([4242, N, B, len(name)])
  return quantise(rng.uniform(-0.999, 0.999, (B, N)))


def gap_input():
  q, x = make_input("gap", DENSE_B, GAP_N)
  x[:, GAP[0]:GAP[1]] = 0.0
  return x


def ragged_input():
  """fp32 [3, RAGGED_PITCH]; what lies behind a length is ordinary data here (the tests plant NaN there)."""
  return make_input("ragged", len(RAGGED_LENS), RAGGED_PITCH)[1]


_consts = None


def constants64():
  """(forward basis [1026, 1, 1024], inverse basis [1026, 1, 1024], window^2 [1024]) as fp64 tensors."""
  global _consts
  if _consts is None:
    fwd, inv, wsq = stft_bases()
    _consts = tuple(torch.from_numpy(np.asarray(a)).double() for a in (fwd[:, None, :], inv[:, None, :], wsq))
  return _consts


def window_sum(frames):
  """window_sumsquare over ``frames`` frames (stft.py:45-95) [1024 + 256 (frames - 1)], fp64."""
  wsq = constants64()[2]
  ws = torch.zeros(FL + HOP * (frames - 1), dtype=torch.float64)
  for f in range(frames):
    ws[f * HOP:f * HOP + FL] += wsq
  return ws


def spectrum64(x):
  """x [B, N] fp64 -> (re, im) [B, 513, F] (stft.py:135-157)."""
  fwd = constants64()[0]
  xp = F.pad(x[:, None, :], (FL // 2, FL // 2), mode="reflect")
  ft = F.conv1d(xp, fwd, stride=HOP)
  return ft[:, :CUT], ft[:, CUT:]


def magnitudes64(x):
  re, im = spectrum64(torch.as_tensor(x).double())
  return torch.sqrt(re * re + im * im)


def denoise64(x, bias, strength, phase_grad=True):
  """``Denoiser.forward`` in fp64: x [B, N] (may require grad), bias [513] -> [B, 1, N]."""
  inv = constants64()[1]
  re, im = spectrum64(x)
  m2 = re * re + im * im
  nz = m2 > 0
  mag = torch.where(nz, torch.sqrt(torch.where(nz, m2, torch.ones_like(m2))), torch.zeros_like(m2))
  safe = torch.where(nz, mag, torch.ones_like(mag))
  ur = torch.where(nz, re / safe, torch.ones_like(re))       # the phase of (0, 0) is 0: cos = 1, sin = 0
  ui = torch.where(nz, im / safe, torch.zeros_like(im))
  if not phase_grad:
    ur, ui = ur.detach(), ui.detach()
  md = torch.clamp(mag - torch.as_tensor(bias).double()[None, :, None] * strength, min=0.0)
  full = F.conv_transpose1d(torch.cat([md * ur, md * ui], dim=1), inv, stride=HOP)
  ws = window_sum(re.shape[2])
  full = torch.where(ws > TINY, full / torch.where(ws > TINY, ws, torch.ones_like(ws)), full) * (FL / HOP)
  return full[:, :, FL // 2:-(FL // 2)]


def grad64(x, r, bias, strength, phase_grad):
  """d <r, denoise64(x)> / d x as an fp64 tensor [B, N]; x, r: fp32 / fp64 arrays or tensors [B, N]."""
  xg = torch.as_tensor(x).double().clone().requires_grad_(True)
  out = denoise64(xg, bias, strength, phase_grad)
  (out[:, 0, :] * torch.as_tensor(r).double()).sum().backward()
  return xg.grad.detach()


def grad64_ragged(x, r, lens, bias, strength, phase_grad):
  """The same per utterance on its own crop; zeros behind each length.  Rows may hold NaN behind their length."""
  x, r = torch.as_tensor(x), torch.as_tensor(r)
  g = torch.zeros(x.shape, dtype=torch.float64)
  for b, n in enumerate(lens):
    g[b, :n] = grad64(x[b:b + 1, :n], r[b:b + 1, :n], bias, strength, phase_grad)[0]
  return g


def clamp_margin(x, bias, strength):
  """(smallest |mag - c| / max(mag, c) over the cells with mag > 0, fraction of those cells that clamp), fp64."""
  mag = magnitudes64(x)
  c = (torch.as_tensor(bias).double() * strength)[None, :, None].expand_as(mag)
  live = mag > 0
  rel = (mag - c).abs()[live] / torch.maximum(mag, c.abs())[live].clamp_min(1e-300)
  return float(rel.min()), float(((mag - c) < 0)[live].double().mean())


class Fixture:
  def __init__(self, path=FIXTURE):
    self.z = np.load(path, allow_pickle=False)

  def bias(self):
    from _corners import unpack_f32
    return unpack_f32(self.z["bias"])

  def audio(self, key):
    q = self.z[key]
    assert q.dtype == np.int16
    return q.astype(np.float32) / np.float32(32768.0)

  def grad(self, N, sname):
    """(the reference's gradient [2, N] fp32, whether it was exactly zero)."""
    from _corners import unpack_f32
    if bool(self.z[f"N{N}/{sname}/is_zero"]):
      return np.zeros((DENSE_B, N), dtype=np.float32), True
    return unpack_f32(self.z[f"N{N}/{sname}/grad"]), False


_fx = None


def fixture():
  global _fx
  if _fx is None:
    _fx = Fixture()
  return _fx
