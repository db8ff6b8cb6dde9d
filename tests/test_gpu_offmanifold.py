"""GPU: the weight-norm plumbing with g != ||v|| in every row, and the device 1x1 inverse on its own.

Every other GPU test of the training direction builds its model with ``synthetic.to_weightnorm_form`` (g = ||v||): the row
scale s = g / ||v|| that csrc/train_prep.hip computes and pack_kernel, wes_fold_kernel, end_grad_kernel, small_prep_kernel and
wn_grad_kernel apply is 1 there, and a wrong index into the scale arrays or a missing ``s`` is invisible.  Here the same
models are reparametrised (tests/_offmanifold.py: v / u, sign(u) g, |u| in [1/4, 4], 1/8 of the rows negative): the dense
weights, and with them the forward, the loss and every reference and bound, stay; s = u.  (g, v) gradients are compared in
the on-manifold metric (``to_on_metric``), where GRAD_TOL applies as it stands.  tests/test_offmanifold_cpu.py shows on the
oracle alone that faults of this kind pass on the manifold and miss GRAD_TOL by more than 10 x off it.

Measured on the MI355X: DESIGN.md section 4.
"""
import ctypes as C
import importlib

import pytest
import torch

import test_gpu_infer_weight_grads as WGT
import test_gpu_recompute as RC
from _cases import Case, oracle_cfg_from_hp, rms
from _offmanifold import check, dense_of, floor_only_names, oracle_infer_grads, raw_worst, reparametrise, to_on_metric
from _prepare import check_prepare_matches_torch_packing
from test_gpu_train import FWD_TOL, _gpu_step
from waveglow_amd import _lib, synthetic
from waveglow_amd.hparams import HParams
from waveglow_amd.model import WaveGlow

T = importlib.import_module("waveglow_amd.train")      # the package also exports a function of this name

pytestmark = pytest.mark.gpu

EARLY = dict(n_early_every=1, n_early_size=2)          # 4 flows: c_k = 8, 6, 4, 2, start rows of length 4, 3, 2, 1


@pytest.fixture(autouse=True)
def _poisoned_gradient_buffers(monkeypatch):
  """Gradient buffers start from NaN: an entry the library never writes makes ``model.grad_finite`` false."""
  monkeypatch.setenv("WG_TRAIN_POISON_GRADS", "1")


@pytest.mark.parametrize("channels", [64, 256, 512])
def test_prepare_matches_torch_packing_off_manifold(channels):
  """The assertions of test_gpu_train.py::test_prepare_matches_torch_packing on the reparametrised model, all four
  ``start`` row lengths.  The dense values are those of the on-manifold model, so its last-place tolerance applies."""
  hp = HParams(n_channels=channels, n_layers=3, n_flows=4, **EARLY)
  sd_off, _ = reparametrise(synthetic.to_weightnorm_form(synthetic.make_state_dict(hp, seed=21)), seed=1)
  check_prepare_matches_torch_packing(hp, sd_off, True)


# name: (hparams, B, T, crop, weight seed)
STEPS = {
    # start rows of length 4, 3, 2, 1
    "c64_h4321": (dict(n_channels=64, n_layers=3, n_flows=4, **EARLY), 2, 9, 40, 5),
    # in_layers rows of 768 elements: exactly the one-pass limit 64 * kKeep of wn_grad_kernel
    "c256_rows768": (dict(n_channels=256, n_layers=3, n_flows=2, **EARLY), 2, 9, 40, 4),
    # rows of 1536: the two-pass form
    "c512_rows1536": (dict(n_channels=512, n_layers=2, n_flows=2, **EARLY), 2, 7, 24, 13),
    # cond_layer rows of 256
    "c64_mel32": (dict(n_channels=64, n_layers=2, n_flows=3, n_early_every=2, n_mel_channels=32), 3, 8, 40, 21),
}


@pytest.mark.parametrize("name", list(STEPS))
def test_train_step_off_manifold(name):
  """One training step of the reparametrised model against oracle.grads_ref / forward_ref on the same state dict, and
  against the on-manifold model's step on the GPU (the two relations; the two packings round v * s and w separately, so
  fp16 fragments may differ in the last place: no bit equality)."""
  from oracle import torch_oracle as O
  over, B, Tn, crop, wseed = STEPS[name]
  hp = HParams(**over)
  sd_on = synthetic.to_weightnorm_form(synthetic.make_state_dict(hp, seed=wseed))
  sd_off, U = reparametrise(sd_on, seed=1)
  mel = synthetic.make_mel(B, Tn, n_mel=hp.n_mel_channels, seed=1234 + B + Tn)
  wav = torch.rand(B, 256 * Tn - crop, generator=torch.Generator().manual_seed(99 + Tn)) * 0.6 - 0.3
  floor = floor_only_names(sd_on)
  assert (len(floor) == 1) == (name == "c64_h4321")
  cfg = oracle_cfg_from_hp(hp)
  loss_ref, g_ref = O.grads_ref(sd_off, mel, wav, cfg, 1.0)
  with torch.no_grad():
    z_ref, ls_ref, ld_ref = O.forward_ref(dense_of(sd_off), mel, wav, cfg)
  loss, y, grads = _gpu_step(hp, sd_off, mel, wav)
  loss_on, y_on, grads_on = _gpu_step(hp, sd_on, mel, wav)
  print(f"{name}: loss gpu {loss:.6f} (on the manifold {loss_on:.6f}) oracle {float(loss_ref):.6f}")
  raw, raw_name = raw_worst(grads, g_ref, skip=floor)
  print(f"{name}: untransformed gradients, worst rel {raw:.3e} ({raw_name})")
  # forward outputs
  z, log_s, log_det = y
  ez = rms(z.detach().cpu() - z_ref)
  print(f"{name}: z rms err {ez:.3e}; to the on-manifold run {rms(z.detach() - y_on[0].detach()):.3e}")
  assert abs(loss - float(loss_ref)) <= 2e-3 * max(1.0, abs(float(loss_ref)))
  assert ez <= FWD_TOL
  for a, b in zip(log_s, ls_ref):
    assert rms(a.detach().cpu() - b) <= FWD_TOL
  for a, b in zip(log_det, ld_ref):
    assert abs(float(a.detach()) - float(b)) <= 1e-3 * max(1.0, abs(float(b)))
  # every gradient against the oracle, (g, v) pairs in the on-manifold metric
  got = to_on_metric(grads, U)
  worst = check(got, to_on_metric(g_ref, U), f"{name} vs oracle", floor_only=floor)
  # the on-manifold run is held to the same bound (a figure beyond GRAD_TOL above and not here: a defect in how s is
  # applied); its oracle gradients are those of the reparametrised model in the on-manifold metric, to 4e-7
  # (tests/test_offmanifold_cpu.py)
  worst_on = check(grads_on, to_on_metric(g_ref, U), f"{name} on the manifold vs oracle", floor_only=floor)
  # the two relations between the two GPU runs (the length-1 rows are zero on both sides, each held to the floor above)
  rel = check(got, {n: g for n, g in grads_on.items() if n not in floor}, f"{name} vs the on-manifold run")
  print(f"{name}: worst per-tensor rel, on-manifold metric: {worst:.3e} (on-manifold run {worst_on:.3e}, between the runs {rel:.3e})")
  assert rms(z.detach() - y_on[0].detach()) <= FWD_TOL
  for a, b in zip(log_s, y_on[1]):
    assert rms(a.detach() - b.detach()) <= FWD_TOL


def test_recompute_off_manifold_equals_full_save():
  """The assertion of test_gpu_recompute.py::test_trainable_c64_equal_to_full_save on the reparametrised model."""
  over = dict(n_channels=64, n_layers=4, n_flows=6, n_early_every=2)
  hp, sd_on, mel, wav = RC._setup(over, 2, 12, 5)
  sd_off, _ = reparametrise(sd_on, seed=1)
  out_f, g_f = RC._train_step(hp, sd_off, mel, wav, False)
  out_r, g_r = RC._train_step(hp, sd_off, mel, wav, True)
  RC._check_modes(out_r, g_r, out_f, g_f, "c64 off the manifold")


def _synthesis(c, sd, r):
  """test_gpu_infer_weight_grads.py: _run for a given weight-normed state dict."""
  model = WaveGlow(c.hp)
  model.load_state_dict(sd)
  model = model.to("cuda:0").train()
  mel, zi, ze = WGT._inputs(c)
  audio = model.infer_differentiable(mel, c.sigma, z_init=zi, z_early=ze, weight_grads=True)
  assert audio.requires_grad and audio.grad_fn is not None
  (audio * r.cuda()).sum().backward()
  torch.cuda.synchronize()
  assert bool(model.grad_finite), "an entry of a (NaN-poisoned) gradient buffer was left unwritten"
  grads = {n: p.grad.detach().float().cpu() for n, p in model.named_parameters()}
  return audio.detach().cpu(), grads, mel.grad.cpu(), zi.grad.cpu(), [z.grad.cpu() for z in ze]


def test_synthesis_weight_grads_off_manifold():
  """infer_differentiable(weight_grads=True) on the reparametrised c64 model: the reference's audio for the weight-normed
  checkpoint (the dense weights are the same), every parameter and input gradient against CPU autograd through
  oracle.infer_ref on the reparametrised leaves."""
  c = Case("c64")
  sd_on = synthetic.to_weightnorm_form(c.sd)
  sd_off, U = reparametrise(sd_on, seed=1)
  r = WGT._r(c)
  _, o_par, o_mel, o_zi, o_ze = oracle_infer_grads(sd_off, c, r)
  audio, grads, g_mel, g_zi, g_ze = _synthesis(c, sd_off, r)
  ref = torch.from_numpy(c.npz["audio_from_weightnorm_ckpt"])
  err = rms(audio - ref)
  print(f"synthesis off the manifold: audio rms err {err:.3e}")
  assert audio.shape == ref.shape and err <= WGT.RMS_TOL
  assert set(grads) == set(o_par)
  floor = floor_only_names(sd_on)
  raw, raw_name = raw_worst(grads, o_par, skip=floor)
  print(f"synthesis: untransformed gradients, worst rel {raw:.3e} ({raw_name})")
  got = to_on_metric(grads, U)
  worst = check(got, to_on_metric(o_par, U), "synthesis vs oracle", floor_only=floor, tol=WGT.GRAD_TOL)
  for what, g, o in [("d mel", g_mel, o_mel), ("d z_init", g_zi, o_zi)] + \
                    [(f"d z_early[{i}]", z, o) for i, (z, o) in enumerate(zip(g_ze, o_ze))]:
    assert g.shape == o.shape, what
    e = WGT._rel(g, o)
    print(f"synthesis {what}: rel {e:.3e}")
    assert e <= WGT.GRAD_TOL, what
  # the on-manifold model's run on the GPU: the two relations
  _, grads_on, _, _, _ = _synthesis(c, sd_on, r)
  rel = check(got, {n: g for n, g in grads_on.items() if n not in floor}, "synthesis vs the on-manifold run", tol=WGT.GRAD_TOL)
  print(f"synthesis: worst per-tensor rel, on-manifold metric: {worst:.3e} (between the runs {rel:.3e})")


# ---------------------------------------------------------------- the device inverse (train_prep.hip: inv1x1_kernel)
def _matrix(kind, c):
  """fp64 [c, c].  "shift": a cyclic-shift permutation times diag(0.5 .. 2): the diagonal is all zero, partial pivoting has
  to exchange rows at every column.  "cond1e4": Q diag(1 .. 1e4) Q2^T from a fixed seed.  "negdet": the same with two rows
  swapped (negative determinant)."""
  f64 = torch.float64
  if kind == "shift":
    d = torch.logspace(torch.log10(torch.tensor(0.5, dtype=f64)), torch.log10(torch.tensor(2.0, dtype=f64)), c, dtype=f64)
    return torch.roll(torch.eye(c, dtype=f64), 1, dims=1) @ torch.diag(d)
  g = torch.Generator().manual_seed(100 + c)
  q1 = torch.linalg.qr(torch.randn(c, c, generator=g, dtype=f64))[0]
  q2 = torch.linalg.qr(torch.randn(c, c, generator=g, dtype=f64))[0]
  w = q1 @ torch.diag(torch.logspace(0, 4, c, dtype=f64)) @ q2.t()
  if float(torch.linalg.det(w)) < 0:
    w = -w if c % 2 else w @ torch.diag(torch.tensor([-1.0] + [1.0] * (c - 1), dtype=f64))      # det > 0 before the swap
  if kind == "negdet":
    w = w[[1, 0] + list(range(2, c))]
  return w


@pytest.mark.parametrize("kind", ["shift", "cond1e4", "negdet"])
def test_device_inverse_elementwise(kind):
  """W_k^-1 as wg_train_prepare writes it (fp64 Gauss-Jordan with partial pivoting on the c_k x c_k corner of an 8 x 8
  identity, c_k = 8, 6, 4, 2) against torch.linalg.inv in fp64 rounded to fp32, entry by entry.  Bound per entry: one fp32
  ulp of the entry (two correctly rounded values of nearly the same number) + 2^-28 max|W^-1| (fp64 elimination at
  condition 1e4 errs by ~1e-12 max|W^-1|, 3.7e-9 is far above it; an fp32 elimination or a missing pivot misses it by 1e-4
  or more).  Prepare only: no forward runs (for "negdet" the reference's logdet is nan).  The 64-float row of each flow is
  NaN before the call and must still be NaN beyond c_k^2."""
  hp = HParams(n_channels=64, n_layers=2, n_flows=4, **EARLY)
  model = WaveGlow(hp)
  model.load_state_dict(synthetic.to_weightnorm_form(synthetic.make_state_dict(hp, seed=7)))
  model = model.to("cuda:0").train()
  flow_c = model.flow_channels()
  assert flow_c == [8, 6, 4, 2]
  refs = []
  with torch.no_grad():
    for k, c in enumerate(flow_c):
      w32 = _matrix(kind, c).float()
      if kind == "shift":
        assert float(w32.diagonal().abs().max()) == 0.0
      assert (float(torch.linalg.det(w32.double())) < 0) == (kind == "negdet" or (kind == "shift" and c % 2 == 0))
      model.convinv[k].conv.weight.copy_(w32.view(c, c, 1))
      refs.append(torch.linalg.inv(w32.double()).float())
    eng = model._get_engine(torch.device("cuda:0"), need_weights=False)
    _names, tensors, wn = T.canonical_params(model, eng)
    stream = torch.cuda.current_stream().cuda_stream
    w = T._Weights(model, tensors, wn, flow_c, eng, stream, want_winv=True)
    torch.cuda.synchronize()
    first = w._winv.clone()
    w._winv.fill_(float("nan"))
    _lib.check(eng.lib.wg_train_prepare(eng.handle, w.params, w.wn, C.byref(w.struct), T._ptr(w.aux), w.aux.numel(),
                                        C.c_void_p(stream)))
    torch.cuda.synchronize()
    rows = w._winv.cpu()
  worst_ulp = worst_abs = 0.0
  for k, c in enumerate(flow_c):
    got, ref = rows[k, :c * c].view(c, c), refs[k]
    assert torch.equal(first[k, :c * c].cpu().view(c, c), got), k
    assert bool(torch.isnan(rows[k, c * c:]).all()), f"flow {k}: written beyond c_k^2"
    assert bool(torch.isfinite(got).all()), k
    ulp = torch.nextafter(ref.abs(), torch.tensor(float("inf"))) - ref.abs()
    diff = (got - ref).abs()
    bound = ulp + 2.0 ** -28 * float(ref.abs().max())
    worst_ulp = max(worst_ulp, float((diff / ulp).max()))
    worst_abs = max(worst_abs, float(diff.max()) / float(ref.abs().max()))
    assert bool((diff <= bound).all()), (k, c, float((diff / bound).max()))
  print(f"winv {kind}: worst entry difference {worst_ulp:.2f} ulp of the entry, {worst_abs:.2e} of max|W^-1|")
