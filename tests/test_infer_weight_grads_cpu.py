"""CPU: yardsticks of ``infer_differentiable(weight_grads=True)`` (tests/test_gpu_infer_weight_grads.py), pinned in fp64.

``x = g(z, mel; theta)`` is synthesis (oracle.torch_oracle.infer_ref), ``f`` the training forward (forward_ref).
``f(g(z, mel; theta), mel; theta) = sigma P z`` holds for EVERY theta, so its derivative with respect to theta vanishes:
``J_fx J_g,theta + J_f,theta = 0``.  For any u, with ``a = J_fx^T u``:  ``J_g,theta^T a = - J_f,theta^T u``  for every parameter
tensor, where the right side is the gradient of ``(z * u).sum()`` alone (no log_s, no logdet term).  That is the full-size
yardstick of the GPU test; here it is checked with the oracle on case c64, dense and weight-normed.

Also: the closed form of the inverse 1x1's weight gradient the kernel implements, the refusals that need no GPU, and the
C ABI of the new entry points.
"""
import ctypes as C
import os
import re

import pytest
import torch

from _cases import Case
from test_infer_grads_cpu import _F64, _plain
from waveglow_amd import _lib, build, synthetic
from waveglow_amd._lib import WgError
from waveglow_amd.model import WaveGlow

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
IDENTITY_TOL_F64 = 1e-9


def _dense_from(leaves):
  """{470-key dense name: tensor} from leaves in either form (weight norm recomposed as the parametrization does)."""
  v1, v0 = "parametrizations.weight.original1", "parametrizations.weight.original0"
  dense = {}
  for k, v in leaves.items():
    if k.endswith(v1):
      dense[k[:-len(v1)] + "weight"] = torch._weight_norm(v, leaves[k[:-len(v1)] + v0], 0)
    elif not k.endswith(v0):
      dense[k] = v
  for k in list(dense):
    if k.startswith("convinv."):
      dense[k] = dense[k].as_subclass(_F64)       # infer_ref inverts through W.float(): stays fp64
  return dense


@pytest.mark.parametrize("normed", [False, True])
def test_weight_gradient_identity_fp64(normed):
  from oracle import torch_oracle as O
  c = Case("c64")
  cfg = c.oracle_cfg()
  sd = synthetic.to_weightnorm_form(c.sd) if normed else c.sd
  leaves = {k: v.double().requires_grad_(True) for k, v in sd.items()}
  w = _dense_from(leaves)
  mel, zi = c.mel.double(), c.z_init.double()
  ze = {k: v.double() for k, v in c.z_early.items()}
  x = _plain(O.infer_ref(w, mel, zi, ze, c.sigma, cfg))
  u = torch.randn(x.shape[0], cfg.n_group, x.shape[1] // cfg.n_group, generator=torch.Generator().manual_seed(3),
                  dtype=torch.float64)
  names = list(leaves)
  # a = J_fx^T u and the right side J_f,theta^T u at x = g(z, mel; theta)
  x0 = x.detach().requires_grad_(True)
  z, _, _ = O.forward_ref(w, mel, x0, cfg)
  gs = torch.autograd.grad((_plain(z) * u).sum(), [x0] + [leaves[n] for n in names], retain_graph=True)
  a, rhs = gs[0], gs[1:]
  lhs = torch.autograd.grad(x, [leaves[n] for n in names], grad_outputs=a)
  worst = 0.0
  for n, l, r in zip(names, lhs, rhs):
    l, r = _plain(l), _plain(r)
    assert float(r.norm()) > 0.0, n
    e = float((l + r).norm() / r.norm())
    worst = max(worst, e)
    assert e <= IDENTITY_TOL_F64, (n, e)
  print(f"normed={normed}: {len(names)} tensors, worst relative L2 {worst:.3e}")


@pytest.mark.parametrize("n", [4, 6, 8])
def test_inverse_1x1_weight_gradient_closed_form(n):
  """w = W^-1 u per row, g = d w:  d W = - sum_rows (W^-T g) (x) w   (what inv_dw1x1_kernel sums)."""
  gen = torch.Generator().manual_seed(20 + n)
  W = (torch.linalg.qr(torch.randn(n, n, generator=gen, dtype=torch.float64))[0]
       + 0.1 * torch.randn(n, n, generator=gen, dtype=torch.float64)).requires_grad_(True)
  U = torch.randn(37, n, generator=gen, dtype=torch.float64)          # rows of u
  G = torch.randn(37, n, generator=gen, dtype=torch.float64)          # rows of g
  Winv = torch.linalg.inv(W)
  w_rows = U @ Winv.t()
  (ref,) = torch.autograd.grad((w_rows * G).sum(), W)
  gv = G @ Winv.detach()                                              # rows of W^-T g
  closed = -(gv.t() @ w_rows.detach())
  assert float((closed - ref).norm() / ref.norm()) <= 1e-12


def test_cpu_tensors_and_trainable_parameters_raise():
  c = Case("c64")
  model = WaveGlow.remove_weightnorm(WaveGlow(c.hp))
  model.load_state_dict(c.sd)
  ze = [c.z_early[k] for k in sorted(c.z_early, reverse=True)]
  # weight_grads=True with CPU tensors: no fallback
  with pytest.raises(WgError):
    model.infer_differentiable(c.mel.clone(), c.sigma, z_init=c.z_init, z_early=ze, weight_grads=True)
  model.requires_grad_(False)
  with pytest.raises(WgError):
    model.infer_differentiable(c.mel.clone().requires_grad_(True), c.sigma, weight_grads=True)
  # weight_grads=False with a trainable parameter still raises (CPU tensors raise before that, on any device)
  model.requires_grad_(True)
  with pytest.raises(WgError):
    model.infer_differentiable(c.mel.clone(), c.sigma, z_init=c.z_init, z_early=ze)
  with pytest.raises(TypeError):
    model.infer_differentiable(c.mel.clone(), c.sigma, c.z_init, ze, True)      # keyword-only


def _header_decl(name):
  text = open(os.path.join(ROOT, "include", "waveglow_amd.h")).read()
  text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
  m = re.search(r"\b(\w[\w \*]*?)\b" + name + r"\s*\(([^;]*?)\)\s*;", text, flags=re.S)
  assert m, name
  return m.group(1).strip(), [a.strip() for a in m.group(2).split(",")]


_KINDS = {C.c_float: "float", C.c_int32: "int32_t", C.c_size_t: "size_t"}      # (c_int32 is c_int where int has 32 bits)


@pytest.mark.parametrize("name", ["wg_train_workspace_bytes", "wg_train_forward", "wg_train_backward", "wg_train_infer_forward",
                                  "wg_train_infer_backward"])
def test_header_and_binding_agree_argument_by_argument(name):
  """Return type and every argument of the five training calls: pointer / float / int32_t / size_t in the header is the same
  kind, at the same place, in _lib.SIGNATURES -- a binding left at another arity or order does not pass."""
  ret, args = _header_decl(name)
  res, argtypes = _lib.SIGNATURES[name]
  assert (ret, res) in (("int", C.c_int), ("size_t", C.c_size_t))
  assert ["ptr" if "*" in a else a.split()[0] for a in args] == [_KINDS.get(t, "ptr") for t in argtypes]
  want_len = {"wg_train_workspace_bytes": 5, "wg_train_forward": 14, "wg_train_backward": 18, "wg_train_infer_forward": 16,
              "wg_train_infer_backward": 17}[name]
  assert len(args) == want_len


def test_abi_of_the_new_entry_points():
  build.build_library()
  lib = _lib.load()
  ret, args = _header_decl("wg_train_infer_backward")
  assert ret == "int"
  kinds = []
  for a in args:
    if "*" in a:
      kinds.append("ptr")
    else:
      kinds.append(a.split()[0])
  want = ["ptr", "ptr", "ptr", "ptr", "float", "float", "ptr", "ptr", "ptr", "int32_t", "int32_t", "int32_t", "ptr", "ptr",
          "size_t", "int32_t", "ptr"]
  assert kinds == want
  res, argtypes = _lib.SIGNATURES["wg_train_infer_backward"]
  assert res is C.c_int and hasattr(lib, "wg_train_infer_backward")
  ctk = {C.c_float: "float", C.c_int32: "int32_t", C.c_size_t: "size_t"}
  assert [ctk.get(t, "ptr") for t in argtypes] == want
  # wg_train_weights: winv appended, every earlier member where it was
  names = [n for n, _ in _lib.WgTrainWeights._fields_]
  assert names[-1] == "winv" and names[-2] == "wupt" and names.index("w1x1") == 14
  assert C.sizeof(_lib.WgTrainWeights) == 17 * C.sizeof(C.c_void_p)
  assert _lib.WgTrainWeights.winv.offset == 16 * C.sizeof(C.c_void_p)
  text = open(os.path.join(ROOT, "include", "waveglow_amd.h")).read()
  body = text[text.index("typedef struct wg_train_weights {"):text.index("} wg_train_weights;")]
  body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
  members = re.findall(r"(\w+);", body)
  assert members == names
  # argument checks run before any device work
  cfg = _lib.WgConfig(80, 12, 8, 4, 2, 8, 256, 3, 1024, 256)
  h = C.c_void_p()
  assert lib.wg_create(C.byref(cfg), 0, C.byref(h)) == 0
  dummy = (C.c_char * 64)()
  d = C.addressof(dummy)
  w = _lib.WgTrainWeights()
  assert lib.wg_train_infer_backward(h, C.byref(w), None, None, 1.0, 1.0, None, None, None, 0, 1, 8, None, d, 64, 0, None) == -1
  assert b"null argument" in lib.wg_last_error()
  assert lib.wg_train_infer_backward(h, C.byref(w), None, d, 0.0, 1.0, None, None, None, 0, 1, 8, None, d, 64, 0, None) == -1
  assert b"scale" in lib.wg_last_error()
  # wg_train_prepare: a winv array with a null entry is refused
  nulls = (C.c_void_p * 12)()
  full = _lib.WgTrainWeights(*([d] * 16), C.cast(nulls, C.c_void_p))
  params = (C.c_void_p * 686)(*[d] * 686)
  assert lib.wg_train_prepare(h, params, 1, C.byref(full), d, 64, None) == -1
  assert b"winv" in lib.wg_last_error()
  lib.wg_destroy(h)
