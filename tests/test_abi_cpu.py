"""CPU-side checks of the drop-in boundary: the C-ABI library loads and exports every symbol that
include/waveglow_amd.h declares; host-only entry points (no GPU needed) behave."""
import ctypes as C
import os
import re

import pytest

from waveglow_amd import _lib, build

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))


@pytest.fixture(scope="module")
def lib():
  build.build_library()
  return _lib.load()


def header_symbols():
  text = open(os.path.join(ROOT, "include", "waveglow_amd.h")).read()
  text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
  return sorted(set(re.findall(r"\b(wg_[a-z_]+)\s*\(", text)))


def test_header_symbols_all_exported_and_bound(lib):
  syms = header_symbols()
  assert len(syms) >= 14
  for s in syms:
    assert hasattr(lib, s), s
    assert s in _lib.SIGNATURES, f"{s} declared in the header but not bound in _lib.SIGNATURES"
  assert sorted(_lib.SIGNATURES) == syms
  # one entry point per call: no suffixed variant of a name, and the natural-order packing entry is gone everywhere
  assert not [s for s in syms if re.search(r"_(ex|flags|flows|params|ragged)$", s)]
  text = open(os.path.join(ROOT, "include", "waveglow_amd.h")).read()
  for gone in ("wg_train_" + n for n in ("pack", "plain")):
    assert gone not in text and gone not in _lib.SIGNATURES and not hasattr(lib, gone), gone
  # the per-utterance lengths are a nullable pointer of the one call, and `saved` an argument of wg_stftloss_forward
  twins = ("wg_infer", "wg_forward", "wg_train_infer_forward", "wg_train_infer_backward", "wg_stft_denoise", "wg_stft_mel",
           "wg_stft_mel_forward_saved", "wg_stft_mel_backward", "wg_stftloss_forward", "wg_stftloss_forward_saved",
           "wg_stftloss_backward")
  removed = [n + "_ragged" for n in twins] + ["wg_stftloss_forward_saved"]
  assert len(removed) == 12
  for gone in removed:
    assert not re.search(rf"\b{gone}\b", text) and gone not in _lib.SIGNATURES and not hasattr(lib, gone), gone


def _struct_listing(name):
  """Member names of the ctypes Structure `name` as the condensed binding in INTEGRATION.md lists them."""
  text = open(os.path.join(ROOT, "INTEGRATION.md")).read()
  code = "\n".join(re.findall(r"```python\n(.*?)```", text, flags=re.S))
  assert code.count(f"class {name}(C.Structure)") == 1, name
  # the _fields_ statement: from its first line to the next class statement or blank line
  m = re.search(rf"class {name}\(C\.Structure\).*?(_fields_ = .*?)\n(?:class |\s*\n)", code, flags=re.S)
  assert m, name
  return re.findall(r'"(\w+)"', re.sub(r"#[^\n]*", "", m.group(1)))


@pytest.mark.parametrize("name", ["WgTrainWeights", "WgTrainGrads"])
def test_integration_guide_lists_the_structs_as_bound(name):
  """The struct a reader binds from INTEGRATION.md has every member of the library's struct, in order: one that is short
  of the tail members makes wg_train_prepare and the backward read past its end."""
  assert _struct_listing(name) == [n for n, _ in getattr(_lib, name)._fields_]


def test_create_validates_configuration(lib):
  h = C.c_void_p()
  bad = _lib.WgConfig(80, 12, 8, 4, 2, 8, 16, 3, 1024, 256)       # n_channels=16
  assert lib.wg_create(C.byref(bad), 0, C.byref(h)) == -1
  assert b"n_channels" in lib.wg_last_error()
  bad = _lib.WgConfig(80, 12, 4, 4, 2, 8, 256, 3, 1024, 256)      # n_group=4
  assert lib.wg_create(C.byref(bad), 0, C.byref(h)) == -1
  ok = _lib.WgConfig(80, 12, 8, 4, 2, 8, 256, 3, 1024, 256)
  assert lib.wg_create(C.byref(ok), 0, C.byref(h)) == 0
  # 2 upsample + 12 * (1 convinv + 6 + 8*4) tensors = 470 keys of the weight-norm-removed state_dict
  assert lib.wg_num_expected_tensors(h) == 470
  assert lib.wg_expected_tensor_name(h, 0) == b"upsample.weight"
  # algorithmic MACs per group-timestep, SURVEY.md section 8(d): 81 235 408 @ C=256
  assert int(lib.wg_macs_per_group_step(h)) == 81235408
  # workspace sizing is pure host arithmetic
  assert lib.wg_infer_workspace_bytes(h, 16, 864) > 16 * 27648 * (2 * 256 * 2 + 64)   # two x planes + Z + OUT
  assert lib.wg_infer_workspace_bytes(h, 0, 864) == 0
  # infer before finalize -> state error, not a crash
  import ctypes
  buf = ctypes.create_string_buffer(64)
  rc = lib.wg_infer(h, buf, None, buf, None, 0, 1.0, buf, 1, 1, 0, buf, 64, None)
  assert rc == -2
  # unknown tensor name rejected
  import numpy as np
  arr = np.zeros(4, dtype=np.float32)
  shp = (C.c_int64 * 1)(4)
  assert lib.wg_set_tensor(h, b"nope.weight", arr.ctypes.data, shp, 1) == -1
  assert lib.wg_destroy(h) == 0


def test_macs_c512(lib):
  h = C.c_void_p()
  cfg = _lib.WgConfig(80, 12, 8, 4, 2, 8, 512, 3, 1024, 256)
  assert lib.wg_create(C.byref(cfg), 0, C.byref(h)) == 0
  assert int(lib.wg_macs_per_group_step(h)) == 261355984
  lib.wg_destroy(h)


def test_train_entry_points_validate_arguments_without_a_gpu():
  """wg_train_* argument checks run before any device work: null members and bad geometry are reported, not crashed on."""
  import ctypes as C
  from waveglow_amd import _lib
  lib = _lib.load()
  cfg = _lib.WgConfig(80, 12, 8, 4, 2, 8, 256, 3, 1024, 256)
  h = C.c_void_p()
  assert lib.wg_create(C.byref(cfg), 0, C.byref(h)) == 0
  assert lib.wg_train_workspace_bytes(h, 32, 63, 16000, 0) > 10 * 2 ** 30       # saved activations of configs[3]
  assert lib.wg_train_workspace_bytes(h, 32, 63, 16001, 0) == 0                   # not a multiple of n_group
  assert lib.wg_train_workspace_bytes(h, 32, 10, 16000, 0) == 0                   # upsampled mel shorter than audio
  w = _lib.WgTrainWeights()
  dummy = (C.c_char * 64)()
  ls = (C.c_void_p * 12)(*[C.addressof(dummy)] * 12)
  rc = lib.wg_train_forward(h, C.byref(w), C.addressof(dummy), C.addressof(dummy), C.addressof(dummy), ls, 1, 8, 2048, 0,
                            C.addressof(dummy), 1 << 40, 0, None)
  assert rc == -1 and b"null member" in lib.wg_last_error()
  # the backward's own checks, before any geometry: the loss scale, then (grads may be null) the required pointers
  d = C.addressof(dummy)
  g = _lib.WgTrainGrads()
  for grads in (C.byref(g), None):
    assert lib.wg_train_backward(h, C.byref(w), grads, d, ls, C.c_float(0.0), d, None, None, 1, 8, 2048, d, 1 << 40, 11, 0, 0,
                                 None) == -1
    assert b"scale" in lib.wg_last_error()
    assert lib.wg_train_backward(h, C.byref(w), grads, d, ls, C.c_float(1.0), None, None, None, 1, 8, 2048, d, 1 << 40, 11, 0,
                                 0, None) == -1
    assert b"null argument" in lib.wg_last_error()
  lib.wg_destroy(h)


FLOW_CALLS = ("wg_infer", "wg_forward", "wg_train_forward", "wg_train_backward", "wg_train_infer_forward",
              "wg_train_infer_backward", "wg_train_prepare", "wg_train_param_grads", "wg_train_workspace_bytes")
PACKING_CHECKER = ("pos_perm", "_PERM_CACHE", "_perms", "_Perms", "_PERM_PLAN", "to_pos_order", "_dense_stack", "_shape_runs",
                   "pack_weights", "to_fragments", "K_TANH_SCALE", "K_SIGM_SCALE", "wn_forward_fragments", "plain_fragments",
                   "packed_grads")


def _package_text():
  import glob
  files = sorted(glob.glob(os.path.join(ROOT, "waveglow_amd", "*.py")))
  assert len(files) >= 25
  return {os.path.basename(f): open(f).read() for f in files}


@pytest.mark.parametrize("name", FLOW_CALLS)
def test_every_flow_entry_point_has_one_python_call_site(name):
  """Each call of the C ABI that the flow itself stands on is written once in the package, comments and docstrings
  included: a second caller is a second copy of the plumbing around it (sizes, pointer arrays, stream, error check)."""
  sites = [(f, m.start()) for f, text in _package_text().items() for m in re.finditer(rf"\b{name}\(", text)]
  assert len(sites) == 1, sites


def test_the_packing_checker_is_not_in_the_package():
  """The torch restatement of the library's weight packing is test code (tests/_packing.py): none of its names is left
  in the package, and the tests' module needs nothing from the binding."""
  for f, text in _package_text().items():
    for name in PACKING_CHECKER:
      assert not re.search(rf"(?<![A-Za-z0-9_]){name}(?![A-Za-z0-9_])", text), (f, name)
  packing = open(os.path.join(ROOT, "tests", "_packing.py")).read()
  for name in PACKING_CHECKER[:-1]:
    assert re.search(rf"^(def|class) {name}\b|^{name}\b", packing, flags=re.M), name
  assert "waveglow_amd" not in re.sub(r'""".*?"""', "", packing, flags=re.S)


def test_parameter_of_another_size_is_refused_by_name(lib):
  """canonical_params holds every parameter to the element count the library will read and write for it
  (wg_train_param_numel), before the dtype / device checks and before anything is launched: on a handle-only engine
  (no GPU) a model whose flow-1 ``end`` conv has 2 output rows instead of 2 h = 8 is refused by name."""
  import importlib
  import torch
  from waveglow_amd import synthetic
  train = importlib.import_module("waveglow_amd.train")      # the package also exports a function of this name
  from waveglow_amd.hparams import HParams
  from waveglow_amd.model import WaveGlow, _Engine
  hp = HParams(n_channels=64, n_layers=4, n_flows=4, n_early_every=2)
  model = WaveGlow(hp)
  model.load_state_dict(synthetic.to_weightnorm_form(synthetic.make_state_dict(hp, seed=3)))
  eng = _Engine(hp, torch.device("cuda", 0))
  with pytest.raises(_lib.WgError, match="the GPU"):          # sizes agree: the next check (CPU tensors) speaks
    train.canonical_params(model, eng)
  names, numels = eng.cache[("train_params", True)]
  assert numels[names.index("WN.1.end.weight")] == 512 and numels == [dict(model.named_parameters())[n].numel() for n in names]
  model.WN[1].end = torch.nn.Conv1d(64, 2, 1)                 # 128 elements where flow 1 (h = 4) has 8 x 64
  with pytest.raises(_lib.WgError, match=r"WN\.1\.end\.weight.*128.*512"):
    train.canonical_params(model, eng)
  assert eng._train_pool == []
