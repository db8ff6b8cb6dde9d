"""CPU-side checks of the soft-DTW loss: the two oracle formulations of tests/_softdtw_oracle.py against each other and
against the properties of the definition (include/waveglow_amd.h: wg_softdtw_*), the C entry points' argument checks that
need no device, and the Python layer's refusals."""
import ctypes as C
import math
import os
import re

import numpy as np
import pytest
import torch

import _metrics_oracle as MO
import _softdtw_cases as cases
import _softdtw_oracle as O

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
NAMES = ("wg_softdtw_bytes", "wg_softdtw_forward", "wg_softdtw_backward")


@pytest.mark.parametrize("cost", cases.COSTS)
@pytest.mark.parametrize("index", range(len(cases.CASES)), ids=cases.IDS)
def test_the_two_formulations_agree(index, cost):
  """Y_case: the largest distance of (a), torch autograd through logsumexp, and (b), the explicit recursions in fp64, over
  the value, E and the gradients.  Both carry a rounding of 2^-53 |R| / gamma in every exponent argument along at most
  Ta + Tb cells, so Y stays within the rounding term of the device bar (tests/_softdtw_cases.py: bar), its factor 100
  included; (b) in fp64 and in longdouble agree to the same bound."""
  ref = cases.reference(index, cost)
  K, Ta, Tb, gamma = ref["case"]
  rounding = 100.0 * 2.0 ** -52 * (Ta + Tb) * max(1.0, ref["rmax"] / gamma)
  y, z = ref["Y_parts"], O.distance(ref["f64"], ref["ld"])
  print(f"{cases.IDS[index]} {cost}: Y value {y['value']:.2e} E {y['E']:.2e} grad {y['grad']:.2e}; fp64 against longdouble "
        f"{z['worst']:.2e}; max|R| {ref['rmax']:.4g}, bound {rounding:.2e}")
  assert ref["Y"] <= rounding and z["worst"] <= rounding
  assert all(np.isfinite(ref["auto"][q]).all() for q in ("value", "E", "g_a", "g_b"))


def test_gradcheck_of_the_autograd_formulation():
  a, b = cases.inputs(cases.CASES[3])
  assert a.shape == (3, 5) and b.shape == (3, 6)
  for cost in cases.COSTS:
    ta = torch.tensor(a, dtype=torch.float64, requires_grad=True)
    tb = torch.tensor(b, dtype=torch.float64, requires_grad=True)
    assert torch.autograd.gradcheck(lambda x, y: O.value_torch(O.distances_torch(x, y, cost), 1.0), (ta, tb))


@pytest.mark.parametrize("cost", cases.COSTS)
def test_one_row_is_a_plain_sum(cost):
  """Ta = 1: one path, so value = sum_j d(0, j) and E = 1 everywhere, whatever gamma is."""
  a, b = cases.inputs(cases.CASES[1])
  for gamma in (1e-3, 0.5, 30.0):
    r = O.explicit(a, b, gamma, cost)
    assert abs(r["value"] - r["D"][0].sum()) <= 1e-13 * r["D"][0].sum()
    # an exponent argument R(s) - R(c) - d(s) is 0 up to the rounding of R, 2^-53 |R|, and is divided by gamma; 8 cells
    tol = 2.0 ** -52 * 8 * max(1.0, float(np.abs(r["R"]).max()) / gamma)
    assert np.abs(r["E"] - 1.0).max() <= tol
    s = O.autograd(a, b, gamma, cost)
    assert abs(s["value"] - r["value"]) <= 1e-13 * r["value"] and np.abs(s["E"] - 1.0).max() <= tol


@pytest.mark.parametrize("cost", cases.COSTS)
@pytest.mark.parametrize("index", range(7), ids=cases.IDS[:7])
def test_the_alignment_is_a_distribution_over_paths(index, cost):
  """E(0,0) = E(Ta-1,Tb-1) = 1 (every path holds both cells), 0 <= E <= 1 (a probability), and every row and every
  column sums to at least 1 (every path crosses each of them at least once)."""
  E = np.asarray(cases.reference(index, cost)["ld"]["E"], dtype=np.float64)
  eps = 1e-12
  assert abs(E[0, 0] - 1.0) <= eps and E[-1, -1] == 1.0
  assert E.min() >= 0.0 and E.max() <= 1.0 + eps
  assert E.sum(axis=1).min() >= 1.0 - eps and E.sum(axis=0).min() >= 1.0 - eps


@pytest.mark.parametrize("index", range(7), ids=cases.IDS[:7])
def test_the_value_lies_between_the_dtw_cost_and_its_path_count_bound(index):
  """value = -gamma log sum over paths exp(-cost / gamma): at most the best path's cost, and at least that minus
  gamma log(number of paths), with at most 3^(Ta + Tb) paths."""
  ref = cases.reference(index, "l2")
  K, Ta, Tb, gamma = ref["case"]
  dtw, _, _ = MO.dtw(ref["a"], ref["b"])
  v = float(ref["ld"]["value"])
  tol = 1e-12 * max(1.0, dtw)
  assert dtw - gamma * (Ta + Tb) * math.log(3.0) - tol <= v <= dtw + tol, (v, dtw)


def test_the_value_tends_to_the_dtw_cost():
  ref = cases.reference(4, "l2")
  dtw, _, _ = MO.dtw(ref["a"], ref["b"])
  v = float(O.explicit(ref["a"], ref["b"], 1e-4, "l2")["value"])
  assert 0.0 <= dtw - v <= 1e-4 * (37 + 41) * math.log(3.0)


def test_identical_frames_have_zero_gradient_through_the_root():
  """d = 0: the L2 gradient through the root is taken as 0, in both formulations; nothing is NaN."""
  a, _ = cases.inputs(cases.CASES[3])
  for res in (O.autograd(a, a, 1.0, "l2"), O.explicit(a, a, 1.0, "l2")):
    assert all(np.isfinite(np.asarray(res[q], dtype=np.float64)).all() for q in ("value", "E", "g_a", "g_b"))
  x, y = O.autograd(a, a, 1.0, "l2"), O.explicit(a, a, 1.0, "l2")
  assert O.distance(x, y)["worst"] <= 1e-12


# ------------------------------------------------------------------------------------------------- the C entry points
def test_the_symbols_are_declared_and_bound():
  from waveglow_amd import _lib
  text = open(os.path.join(ROOT, "include", "waveglow_amd.h")).read()
  text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
  for n in NAMES:
    assert re.search(rf"\b{n}\s*\(", text), n
    assert n in _lib.SIGNATURES, n
  assert not re.search(r"\bvoid\s*\*\s*(workspace|saved)\b", "".join(
    m.group(0) for m in re.finditer(r"\bwg_softdtw_[a-z]+\s*\([^;{}]*?\)\s*;", text, flags=re.S)))
  assert (_lib.WG_SDTW_L2, _lib.WG_SDTW_SQ) == (0, 1)
  assert re.search(r"#define\s+WG_SDTW_L2\s+0\b", text) and re.search(r"#define\s+WG_SDTW_SQ\s+1\b", text)


@pytest.fixture(scope="module")
def lib():
  from waveglow_amd import _lib, build
  build.build_library()
  return _lib.load()


def test_r_buffer_size(lib):
  assert lib.wg_softdtw_bytes(1, 1, 1) == 8
  assert lib.wg_softdtw_bytes(3, 5, 6) == 3 * (5 + 6 - 1) * 5 * 8
  assert lib.wg_softdtw_bytes(16, 864, 865) == 16 * 1728 * 864 * 8
  assert lib.wg_softdtw_bytes(2, 4096, 4096) == 2 * 8191 * 4096 * 8
  for bad in ((0, 5, 6), (1, 0, 6), (1, 5, 0), (1, 4097, 6), (1, 5, 4097), (-1, 5, 6)):
    assert lib.wg_softdtw_bytes(*bad) == 0, bad


def test_entry_points_validate_arguments_without_a_gpu(lib):
  """Every refusal comes before any device work: the pointers below are host memory that no kernel may touch."""
  dummy = (C.c_char * 64)()
  p = C.addressof(dummy)
  fwd, bwd = lib.wg_softdtw_forward, lib.wg_softdtw_backward
  ok = dict(gamma=1.0, cost=0, B=1, K=4, ta=5, tb=6)

  def forward(fa=p, na=p, fb=p, nb=p, value=p, r=p, **kw):
    a = dict(ok, **kw)
    return fwd(fa, na, fb, nb, a["gamma"], a["cost"], value, r, a["B"], a["K"], a["ta"], a["tb"], None)

  def backward(fa=p, na=p, fb=p, nb=p, r=p, gv=p, e=p, ga=p, gb=p, **kw):
    a = dict(ok, **kw)
    return bwd(fa, na, fb, nb, a["gamma"], a["cost"], r, gv, e, ga, gb, a["B"], a["K"], a["ta"], a["tb"], None)

  for call in (forward, backward):
    for name in ("fa", "na", "fb", "nb"):
      assert call(**{name: None}) == -1 and b"null" in lib.wg_last_error(), name
    for kw, word in ((dict(K=0), b"K"), (dict(K=129), b"K"), (dict(B=0), b"B"), (dict(ta=4097), b"tmax"),
                     (dict(tb=4097), b"tmax"), (dict(ta=0), b"tmax"), (dict(gamma=0.0), b"gamma"),
                     (dict(gamma=-1.0), b"gamma"), (dict(gamma=float("inf")), b"gamma"), (dict(gamma=float("nan")), b"gamma"),
                     (dict(cost=2), b"cost"), (dict(cost=-1), b"cost")):
      assert call(**kw) == -1, kw
      assert word in lib.wg_last_error(), (kw, lib.wg_last_error())
  assert forward(value=None) == -1 and b"null" in lib.wg_last_error()
  assert backward(r=None) == -1 and b"null" in lib.wg_last_error()
  assert backward(gv=None) == -1 and b"g_value" in lib.wg_last_error()
  assert backward(gv=None, gb=None) == -1
  assert backward(gv=None, e=None, ga=None, gb=None) == 0          # nothing asked for: no device work, no error


# --------------------------------------------------------------------------------------------------- the Python layer
class OnGpu(torch.Tensor):
  """A host tensor that says it is on a GPU: what the refusals see, with no device behind it."""
  device = torch.device("cuda:0")


def _gpu(*shape, dtype=torch.float32):
  return torch.zeros(*shape, dtype=dtype).as_subclass(OnGpu)


def test_python_layer_refuses_bad_arguments_before_any_launch():
  import waveglow_amd
  from waveglow_amd import _lib, softdtw
  assert waveglow_amd.SoftDTWLoss is softdtw.SoftDTWLoss and waveglow_amd.soft_dtw is softdtw.soft_dtw
  assert waveglow_amd.soft_dtw_alignment is softdtw.soft_dtw_alignment
  x = torch.zeros((2, 4, 9))
  g = _gpu(2, 4, 9)
  for fn in (softdtw.soft_dtw, softdtw.soft_dtw_alignment):
    for call in (lambda: fn(x, None, x, None),                                        # CPU tensors
                 lambda: fn(g, None, x, None),
                 lambda: fn(_gpu(2, 4, 9, dtype=torch.float64), None, g, None),       # dtype
                 lambda: fn(g, None, _gpu(2, 4, 9, dtype=torch.float16), None),
                 lambda: fn(_gpu(4, 9), None, g, None),                               # rank
                 lambda: fn(g, None, _gpu(3, 4, 9), None),                            # B
                 lambda: fn(g, None, _gpu(2, 5, 9), None),                            # K
                 lambda: fn(_gpu(1, 129, 3), None, _gpu(1, 129, 3), None),            # K > 128
                 lambda: fn(_gpu(1, 2, 4097), None, _gpu(1, 2, 5), None),             # T > 4096
                 lambda: fn(g, None, g, None, gamma=0.0),
                 lambda: fn(g, None, g, None, gamma=-1.0),
                 lambda: fn(g, None, g, None, gamma=float("inf")),
                 lambda: fn(g, None, g, None, gamma=float("nan")),
                 lambda: fn(g, None, g, None, gamma="soft"),
                 lambda: fn(g, None, g, None, cost="l1"),
                 lambda: fn(g, [9, 0], g, None),                                      # counts outside [1, T]
                 lambda: fn(g, [9, 10], g, None),
                 lambda: fn(g, None, g, torch.tensor([9, 10])),
                 lambda: fn(g, (9,), g, None)):
      with pytest.raises(_lib.WgError):
        call()
  for call in (lambda: softdtw.SoftDTWLoss(device="cpu"), lambda: softdtw.SoftDTWLoss(features="lpc"),
               lambda: softdtw.SoftDTWLoss(cost="l1"), lambda: softdtw.SoftDTWLoss(gamma=0.0),
               lambda: softdtw.SoftDTWLoss(n_mfcc=0), lambda: softdtw.SoftDTWLoss(n_mfcc=129)):
    with pytest.raises(_lib.WgError):
      call()
  crit = softdtw.SoftDTWLoss(device="cuda:0")
  assert (crit.gamma, crit.features, crit.n_mfcc, crit.cost) == (1.0, "mfcc", 16, "l2")
  m = _gpu(2, 80, 9)
  for call in (lambda: crit(torch.zeros((2, 80, 9)), None, torch.zeros((2, 80, 9)), None),       # CPU tensors
               lambda: crit.values(torch.zeros((2, 80, 9)), None, m, None),
               lambda: crit(m.double(), None, m, None), lambda: crit(m[0], None, m[0], None),
               lambda: crit(m, None, _gpu(2, 40, 9), None), lambda: crit(m, None, _gpu(3, 80, 9), None),
               lambda: crit(_gpu(2, 16, 9), None, _gpu(2, 16, 9), None),                         # n_mfcc = n_mel
               lambda: crit(_gpu(2, 80, 4097), None, m, None),
               lambda: crit(m, [9, 10], m, None), lambda: crit(m, None, m, [0, 9]),
               lambda: softdtw.SoftDTWLoss(features="mel", device="cuda:0")(_gpu(1, 129, 4), None, _gpu(1, 129, 4), None)):
    with pytest.raises(_lib.WgError):
      call()
  # what a forward keeps: R, the fp32 features and, with the DCT in front, the fp64 mels
  assert softdtw.r_bytes(16, 864, 865) == 16 * 1728 * 864 * 8
  assert crit.workspace_bytes(16, 864, 865) == 16 * 1728 * 864 * 8 + 16 * (864 + 865) * (4 * 16 + 8 * 80)
  assert softdtw.SoftDTWLoss(features="mel").workspace_bytes(2, 10, 20, n_mel=40) == 2 * 29 * 10 * 8 + 4 * 2 * 40 * 30
  assert crit.workspace_bytes(0, 10, 10) == 0 and crit.workspace_bytes(1, 4097, 10) == 0


def test_the_dct_basis_is_the_metric_s():
  from waveglow_amd import softdtw
  got = softdtw.dct_basis(80, 16).numpy()
  assert got.dtype == np.float64 and np.abs(got - MO.dct_basis(80, 16)).max() <= 4e-16
  assert np.abs(got @ got.T - np.eye(16)).max() <= 1e-14                     # orthonormal rows
