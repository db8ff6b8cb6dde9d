"""Without a GPU: the band geometry of include/waveglow_amd.h (wg_softdtw_banded_*) against brute force, the banded oracle
of tests/_softdtw_band_oracle.py against itself and against the dense oracle, wg_softdtw_banded_bytes, the ``band``
refusals of the Python layer and the binding of the new symbols."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

import _softdtw_band_oracle as BO
import _softdtw_cases as cases
import _softdtw_oracle as O

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
NAMES = ("wg_softdtw_banded_bytes", "wg_softdtw_banded_forward", "wg_softdtw_banded_backward")
# (K, Ta, Tb, w, gamma): small shapes with a partial band, both orientations and a single row / column
SMALL = ((4, 1, 1, 1, 1.0), (4, 1, 9, 1, 1.0), (4, 9, 1, 2, 1.0), (3, 12, 17, 1, 0.5), (3, 17, 12, 2, 1.0), (5, 15, 15, 3, 0.1))


def _inputs(case):
  return cases.inputs((case[0], case[1], case[2], case[4]))


# ---------------------------------------------------------------------------------------------------------- geometry
def test_band_geometry_against_brute_force():
  """For all Ta, Tb <= 18 and w <= 4, and some larger shapes: the corners are inside; a diagonal's in-band rows are the
  interval of the closed formulas, at most 2 w + 1 wide, its ends advancing by 0 or 1; every cell is reachable from (0,0)
  and reaches (n,m) through in-band neighbours; w >= min(n, m) covers the matrix."""
  shapes = [(Ta, Tb, w) for Ta in range(1, 19) for Tb in range(1, 19) for w in range(1, 5)]
  shapes += [(70, 45, 2), (45, 70, 5), (200, 7, 1), (7, 200, 1), (64, 66, 31), (130, 129, 32)]
  for Ta, Tb, w in shapes:
    M = BO.mask(Ta, Tb, w)
    n, m = Ta - 1, Tb - 1
    assert M[0, 0] and M[n, m], (Ta, Tb, w)
    prev = None
    for d in range(Ta + Tb - 1):
      rows = [i for i in range(max(0, d - m), min(n, d) + 1) if M[i, d - i]]
      lo, hi = BO.interval(d, Ta, Tb, w)
      assert rows == list(range(lo, hi + 1)) and rows, (Ta, Tb, w, d, rows, lo, hi)
      assert hi - lo + 1 <= 2 * w + 1, (Ta, Tb, w, d)
      if prev is not None:
        assert lo - prev[0] in (0, 1) and hi - prev[1] in (0, 1), (Ta, Tb, w, d)
      prev = (lo, hi)
    for i in range(Ta):
      for j in range(Tb):
        if not M[i, j]:
          continue
        if (i, j) != (0, 0):
          assert any(p >= 0 and q >= 0 and M[p, q] for p, q in ((i - 1, j), (i, j - 1), (i - 1, j - 1))), (Ta, Tb, w, i, j)
        if (i, j) != (n, m):
          assert any(p <= n and q <= m and M[p, q] for p, q in ((i + 1, j), (i, j + 1), (i + 1, j + 1))), (Ta, Tb, w, i, j)
    if w >= min(n, m):
      assert M.all(), (Ta, Tb, w)
    if Ta == Tb:
      i, j = np.indices((Ta, Tb))
      assert (M == (np.abs(i - j) <= w)).all(), (Ta, w)


def test_the_products_of_the_largest_shape_fit_int32():
  n = m = 4095
  assert max(n * m + 511 * n, (n + m) * n + 511 * n) < 2 ** 31


# ------------------------------------------------------------------------------------------------------------ oracle
@pytest.mark.parametrize("cost", BO.COSTS)
@pytest.mark.parametrize("case", SMALL, ids=[f"{c[1]}x{c[2]}-w{c[3]}" for c in SMALL])
def test_the_formulations_agree(case, cost):
  a, b = _inputs(case)
  w, gamma = case[3], case[4]
  auto, f64 = BO.autograd(a, b, gamma, cost, w), BO.explicit(a, b, gamma, cost, w)
  ld = BO.explicit(a, b, gamma, cost, w, np.longdouble)
  assert O.distance(auto, f64)["worst"] <= 1e-11 and O.distance(f64, ld)["worst"] <= 1e-11
  for dtype in (np.float64, np.longdouble):
    dg = BO.diagonal(a, b, gamma, cost, w, dtype)
    assert abs(float(dg["value"] - ld["value"])) <= 1e-11 * max(1.0, abs(float(ld["value"])))
    assert float(np.abs(dg["E"] - ld["E"]).max()) <= 1e-11
  # E is a flow from (n,m) to (0,0) inside the band
  M = BO.mask(case[1], case[2], w)
  assert not f64["E"][~M].any() and np.isinf(f64["R"][~M]).all() and np.isfinite(f64["R"][M]).all()
  assert f64["E"][-1, -1] == 1.0 and abs(f64["E"][0, 0] - 1.0) <= 1e-12
  assert not auto["E"][~M].any()


@pytest.mark.parametrize("cost", BO.COSTS)
def test_a_covering_band_is_the_dense_oracle_exactly(cost):
  for index in (1, 2, 3, 4):
    K, Ta, Tb, gamma = cases.CASES[index]
    a, b = cases.inputs(cases.CASES[index])
    w = max(1, min(Ta, Tb) - 1)
    for dtype in (np.float64, np.longdouble):
      x, y = BO.explicit(a, b, gamma, cost, w, dtype), O.explicit(a, b, gamma, cost, dtype)
      for q in ("value", "R", "E", "g_a", "g_b"):
        assert np.array_equal(np.asarray(x[q]), np.asarray(y[q])), (index, q)
      assert np.array_equal(np.asarray(BO.explicit(a, b, gamma, cost, None, dtype)["E"]), np.asarray(y["E"]))
    x, y = BO.autograd(a, b, gamma, cost, w), O.autograd(a, b, gamma, cost)
    for q in ("value", "E", "g_a", "g_b"):
      assert np.array_equal(x[q], y[q]), (index, q)


def test_the_value_grows_as_the_band_narrows_and_tends_to_the_banded_dtw():
  a, b = cases.inputs((16, 37, 41, 1.0))
  dense = float(O.explicit(a, b, 1.0, "l2")["value"])
  v = [float(BO.diagonal(a, b, 1.0, "l2", w, want_e=False)["value"]) for w in (1, 2, 5, 20)]
  assert all(x >= y - 1e-12 for x, y in zip(v, v[1:])) and v[-1] >= dense - 1e-12
  assert BO.dtw(a, b, "l2", None) <= BO.dtw(a, b, "l2", 2) <= BO.dtw(a, b, "l2", 1)
  c = BO.dtw(a, b, "l2", 2)
  soft = float(BO.diagonal(a, b, 1e-3, "l2", 2, want_e=False)["value"])
  assert -1e-9 * c <= c - soft <= 1e-3 * 78 * np.log(3.0) + 1e-9 * c


def test_the_divergence_of_the_oracle():
  """0 at a = b with a zero gradient; non-negative for the squared cost without a band; the autograd and the explicit
  combination agree."""
  a, b = cases.inputs((4, 12, 17, 0.5))
  for cost in BO.COSTS:
    for w in (None, 2):
      same = BO.divergence(a, a, 0.5, cost, w)
      assert same["value"] == 0.0 and float(np.abs(same["g_a"]).max()) <= 1e-12
      ex = BO.divergence(a, b, 0.5, cost, w)
      au = BO.divergence(a, b, 0.5, cost, w, fn=lambda x, y: BO.autograd(x, y, 0.5, cost, w))
      assert abs(float(ex["value"]) - au["value"]) <= 1e-11 * max(1.0, abs(au["value"]))
      assert float(np.abs(ex["g_a"] - au["g_a"]).max()) <= 1e-11 and float(np.abs(ex["g_b"] - au["g_b"]).max()) <= 1e-11
  assert BO.divergence(a, b, 0.5, "sq")["value"] > 0.0


# ------------------------------------------------------------------------------------------------- the C entry points
def test_the_symbols_are_declared_and_bound():
  from waveglow_amd import _lib
  text = open(os.path.join(ROOT, "include", "waveglow_amd.h")).read()
  text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
  for n in NAMES:
    assert re.search(rf"\b{n}\s*\(", text), n
    assert n in _lib.SIGNATURES, n
  fwd, bwd = _lib.SIGNATURES["wg_softdtw_forward"][1], _lib.SIGNATURES["wg_softdtw_backward"][1]
  assert _lib.SIGNATURES["wg_softdtw_banded_forward"][1] == fwd[:-1] + [C.c_int32, C.c_void_p]
  assert _lib.SIGNATURES["wg_softdtw_banded_backward"][1] == bwd[:-1] + [C.c_int32, C.c_void_p]


@pytest.fixture(scope="module")
def lib():
  from waveglow_amd import _lib, build
  build.build_library()
  return _lib.load()


def test_banded_buffer_size(lib):
  assert lib.wg_softdtw_banded_bytes(16, 864, 865, 60) == 26763264 == 16 * 1728 * 121 * 8
  assert lib.wg_softdtw_banded_bytes(1, 1, 1, 1) == 8
  assert lib.wg_softdtw_banded_bytes(3, 5, 60, 7) == 3 * 64 * 5 * 8                      # S = tmax_a under a wide band
  assert lib.wg_softdtw_banded_bytes(2, 4096, 4096, 511) == 2 * 8191 * 1023 * 8
  for bad in ((16, 864, 865, 0), (16, 864, 865, 512), (16, 864, 865, -1), (16, 0, 865, 60), (16, 864, 0, 60),
              (16, 4097, 865, 60), (16, 864, 4097, 60), (0, 864, 865, 60)):
    assert lib.wg_softdtw_banded_bytes(*bad) == 0, bad


def test_banded_entry_points_validate_arguments_without_a_gpu(lib):
  """Every refusal comes before any device work: the pointers below are host memory that no kernel may touch."""
  dummy = (C.c_char * 64)()
  p = C.addressof(dummy)

  def forward(fa=p, value=p, gamma=1.0, cost=0, B=1, K=4, ta=5, tb=6, band=2):
    return lib.wg_softdtw_banded_forward(fa, p, p, p, gamma, cost, value, p, B, K, ta, tb, band, None)

  def backward(fa=p, r=p, gv=p, e=p, ga=p, gb=p, gamma=1.0, cost=0, B=1, K=4, ta=5, tb=6, band=2):
    return lib.wg_softdtw_banded_backward(fa, p, p, p, gamma, cost, r, gv, e, ga, gb, B, K, ta, tb, band, None)

  for call in (forward, backward):
    assert call(fa=None) == -1 and b"null" in lib.wg_last_error()
    for kw, word in ((dict(band=0), b"band"), (dict(band=512), b"band"), (dict(band=-3), b"band"), (dict(K=129), b"K"),
                     (dict(ta=4097), b"tmax"), (dict(tb=0), b"tmax"), (dict(gamma=0.0), b"gamma"), (dict(cost=2), b"cost")):
      assert call(**kw) == -1, kw
      assert word in lib.wg_last_error(), (kw, lib.wg_last_error())
  assert forward(value=None) == -1 and backward(r=None) == -1
  assert backward(gv=None) == -1 and b"g_value" in lib.wg_last_error()
  assert backward(gv=None, e=None, ga=None, gb=None) == 0          # nothing asked for: no device work, no error


# --------------------------------------------------------------------------------------------------- the Python layer
class OnGpu(torch.Tensor):
  """A host tensor that says it is on a GPU: what the refusals see, with no device behind it."""
  device = torch.device("cuda:0")


def test_python_layer_refuses_a_bad_band_before_the_tensor_checks():
  import waveglow_amd
  from waveglow_amd import _lib, softdtw
  assert waveglow_amd.soft_dtw_divergence is softdtw.soft_dtw_divergence
  x = torch.zeros((2, 4, 9))                              # a CPU tensor: the band is refused first, with its own message
  for fn in (softdtw.soft_dtw, softdtw.soft_dtw_alignment, softdtw.soft_dtw_divergence):
    for bad in (0, 512, -1, True, False, 3.0, "3", [3], np.float32(2)):
      with pytest.raises(_lib.WgError, match="band"):
        fn(x, None, x, None, band=bad)
    for good in (None, 1, 511):                           # accepted: the refusal is the tensor's
      with pytest.raises(_lib.WgError, match="feat_a"):
        fn(x, None, x, None, band=good)
    with pytest.raises(TypeError):                        # keyword-only
      fn(x, None, x, None, 1.0, "l2", 3)
  g = torch.zeros((2, 4, 9)).as_subclass(OnGpu)
  for call in (lambda: softdtw.soft_dtw_divergence(g, None, x, None), lambda: softdtw.soft_dtw_divergence(g, [9, 10], g, None),
               lambda: softdtw.soft_dtw_divergence(g, None, g, None, gamma=0.0),
               lambda: softdtw.soft_dtw_divergence(g, None, g, None, cost="l1")):
    with pytest.raises(_lib.WgError):
      call()
  for bad in (0, 512, True, 2.0):
    with pytest.raises(_lib.WgError, match="band"):
      softdtw.SoftDTWLoss(band=bad)
    with pytest.raises(_lib.WgError, match="band"):
      softdtw.r_bytes(1, 5, 6, bad)
  crit = softdtw.SoftDTWLoss(band=60, divergence=True)
  assert (crit.band, crit.divergence) == (60, True)
  plain = softdtw.SoftDTWLoss()
  assert (plain.band, plain.divergence) == (None, False)


def test_bytes_kept_with_a_band_and_with_the_divergence(lib):
  from waveglow_amd import softdtw
  assert softdtw.r_bytes(16, 864, 865, 60) == 26763264 and softdtw.r_bytes(16, 864, 865, band=None) == 16 * 1728 * 864 * 8
  feats = 16 * (864 + 865) * (4 * 16 + 8 * 80)
  assert softdtw.SoftDTWLoss(band=60).workspace_bytes(16, 864, 865) == 26763264 + feats
  # the divergence: 3 B pairs at the common length 865, R and fp32 features; the fp64 mels are those of the B utterances
  want = 48 * 1729 * 121 * 8 + 4 * 48 * 16 * 2 * 865 + 8 * 16 * 80 * (864 + 865)
  assert softdtw.SoftDTWLoss(band=60, divergence=True).workspace_bytes(16, 864, 865) == want
  want = 6 * 39 * 20 * 8 + 4 * 6 * 40 * 40
  assert softdtw.SoftDTWLoss(features="mel", divergence=True).workspace_bytes(2, 10, 20, n_mel=40) == want
  assert softdtw.SoftDTWLoss(band=3, divergence=True).workspace_bytes(1, 4097, 10) == 0
