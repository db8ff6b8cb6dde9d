"""Inference and the no-grad forward at the top of the accepted size range (tests/_envelope.py, DESIGN.md sections 2 and 8).

Between the largest geometry any other test runs (32 x 80x4000: Rp = 128 256) and the size check (Rp <= 1 048 448) byte
offsets inside a 64-channel plane pass 2^31 and come within 128 rows of 2^32.  The property that pins a result there needs
no reference of that size: an utterance's result does not depend on the batch it is in (the ragged contract, bit for bit),
so every utterance of a large batch must equal its result in a slice of 256 utterances (Rp = 16 384, where the reference
fixtures pin the kernels) -- every one of them: rows are phase-major, each utterance has columns in every phase block.
Models are synthetic, shallow (4 flows) and fully dilated (8 layers: the (p +- 128) phase wrap against a large Rp).

Every large case prints its wall time and peak device memory; it skips only when the device has less memory free than
the library's own workspace figure plus the case's tensors."""
import ctypes as C
import gc
import os
import time

import pytest
import torch

import _envelope as E
from test_gpu_parity import ROUND_TRIP_TOL, build_model
from waveglow_amd import _lib, synthetic
from waveglow_amd.hparams import HParams
from waveglow_amd.model import WaveGlowLoss

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
SLICE = 256          # utterances per reference call of the wide shapes
SIGMA = 0.8


def _hp(channels):
  return HParams(n_channels=channels, n_layers=8, n_flows=4, n_early_every=2)


def _release(model):
  """Drop the engine's cached workspace (tens of GB after a large case) and hand the memory back to the device."""
  if model is not None and model._engine is not None:
    model._engine._ws.clear()
  torch.cuda.empty_cache()


@pytest.fixture(scope="module")
def pool():
  """Models by (channels, WG_FORCE_BN) and the results the forward / loss cases share.  The engine caches its last
  workspace: after the large cases the models are deleted and the cache emptied, so that the rest of the suite does not
  run with 40 GB held on the card."""
  p = {"models": {}, "shared": {}}
  yield p
  for m in p["models"].values():
    _release(m)
  p["models"].clear()
  p["shared"].clear()
  torch.cuda.empty_cache()


def _model(pool, channels, force_bn=None):
  key = (channels, force_bn)
  if key not in pool["models"]:
    old = os.environ.get("WG_FORCE_BN")
    if force_bn:
      os.environ["WG_FORCE_BN"] = force_bn          # read by wg_create: the engine is created below, inside the setting
    else:
      os.environ.pop("WG_FORCE_BN", None)
    try:
      hp = _hp(channels)
      m = build_model(hp, synthetic.make_state_dict(hp, seed=6), device=DEV)
      m._get_engine(torch.device(DEV))
    finally:
      if old is None:
        os.environ.pop("WG_FORCE_BN", None)
      else:
        os.environ["WG_FORCE_BN"] = old
    pool["models"][key] = m
  return pool["models"][key]


def _inputs(B, T, dtype, seed, frames=None):
  """mel / z_init / z_early drawn on the device; with ``frames`` the slack behind every utterance is garbage that must not
  matter (mel 3.0, noise 7.0), as in test_ragged_batch_equals_batch_of_one_calls."""
  g = torch.Generator(device=DEV).manual_seed(seed)
  mel = (torch.randn(B, 80, T, device=DEV, generator=g) * 2 - 5).clamp_(-11.5, 2.0).to(dtype)
  z_init = torch.randn(B, 6, 32 * T, device=DEV, generator=g).to(dtype)
  z_early = torch.randn(B, 2, 32 * T, device=DEV, generator=g).to(dtype)
  if frames is not None:
    fr = frames.to(DEV)
    mel.masked_fill_(torch.arange(T, device=DEV)[None, None, :] >= fr[:, None, None], 3.0)
    behind = torch.arange(32 * T, device=DEV)[None, None, :] >= 32 * fr[:, None, None]
    z_init.masked_fill_(behind, 7.0)
    z_early.masked_fill_(behind, 7.0)
  return mel, z_init, z_early


def _wide_frames(B, T, seed):
  """Frame counts from [1, T], every fourth utterance at T."""
  g = torch.Generator().manual_seed(seed)
  fr = torch.randint(1, T + 1, (B,), generator=g, dtype=torch.int32)
  fr[::4] = T
  return fr


def _need_or_skip(model, B, T, tensor_bytes, forward=False):
  eng = model._get_engine(torch.device(DEV))
  _release(model)
  ws = eng.lib.wg_forward_workspace_bytes(eng.handle, B, T, 256 * T) if forward else eng.lib.wg_infer_workspace_bytes(eng.handle, B, T)
  assert ws > 0
  need = ws + tensor_bytes
  free, _ = torch.cuda.mem_get_info(torch.device(DEV))
  if free < need:
    pytest.skip(f"needs {need / 2**30:.1f} GiB (workspace {ws / 2**30:.1f} + tensors {tensor_bytes / 2**30:.1f}), {free / 2**30:.1f} GiB free")
  return need


class _Clock:
  def __init__(self, label):
    self.label = label

  def __enter__(self):
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    self.t0 = time.perf_counter()
    return self

  def __exit__(self, *exc):
    torch.cuda.synchronize()
    print(f"\nenvelope case {self.label}: {time.perf_counter() - self.t0:.2f} s, peak "
          f"{torch.cuda.max_memory_allocated() / 2**30:.2f} GiB allocated")


def _zero_behind(out, frames_dev):
  """True when every sample behind 256 * frames[b] is zero."""
  behind = torch.arange(out.shape[1], device=out.device)[None, :] >= 256 * frames_dev[:, None].long()
  return not bool((out.masked_fill(~behind, 0) != 0).any())


def _run_wide(model, name, dtype, ragged, seed=11):
  """The large call, then the same call on slices of 256 consecutive utterances, compared on the device one slice at a
  time: every utterance bit for bit, zero behind its end, everything finite.  Returns (mel, audio) of the large call."""
  s = E.SHAPES[name]
  B, T = s.B, s.T
  esz = torch.finfo(dtype).bits // 8
  tensor_bytes = B * (80 * T + 8 * 32 * T) * (esz + 4) + 2 * B * 256 * T * esz      # inputs (+ their fp32 draws), audio, a slice's worth
  _need_or_skip(model, B, T, tensor_bytes)
  frames = _wide_frames(B, T, seed) if ragged else None
  mel, z_init, z_early = _inputs(B, T, dtype, seed, frames)
  fr_dev = frames.to(DEV) if ragged else None
  with torch.no_grad():
    out = model.infer_with_noise(mel, z_init, [z_early], SIGMA, frames=fr_dev)
    torch.cuda.synchronize()
    assert out.shape == (B, 256 * T) and out.dtype == dtype
    assert bool(torch.isfinite(out).all())
    bad = []
    for lo in range(0, B, SLICE):
      hi = min(lo + SLICE, B)
      ref = model.infer_with_noise(mel[lo:hi], z_init[lo:hi], [z_early[lo:hi]], SIGMA,
                                   frames=fr_dev[lo:hi] if ragged else None)
      if not torch.equal(out[lo:hi], ref):
        bad += [lo + int(b) for b in torch.nonzero((out[lo:hi] != ref).any(1)).flatten()[:8]]
      if ragged and not _zero_behind(out[lo:hi], fr_dev[lo:hi]):
        bad.append(-lo - 1)
      del ref
    assert not bad, f"{name}: utterances that differ from their slice call (negative: slice with samples behind an end): {bad[:32]}"
  del z_init, z_early
  return mel, out


WIDE_CASES = [
  # channels, shape, dtype, WG_FORCE_BN
  (64, "wide_cross", torch.float16, None),
  (64, "wide_top", torch.float16, None),
  (64, "wide_top", torch.float32, None),
  (64, "wide_top", torch.float16, "64"),
  (128, "wide_cross", torch.float16, None),
  (256, "wide_cross", torch.float16, None),
  (256, "wide_cross", torch.float16, "64"),
  (256, "wide_top", torch.float16, None),
  (512, "wide_cross", torch.float16, None),
]


@pytest.mark.parametrize("channels,name,dtype,force_bn", WIDE_CASES,
                         ids=[f"c{c}-{n}-{str(d).split('.')[1]}-bn{b or 'auto'}" for c, n, d, b in WIDE_CASES])
def test_wide_ragged_batch_equals_slices_of_256(pool, channels, name, dtype, force_bn):
  """wg_infer with frame counts on 8 193 / 16 382 utterances of up to 56 frames: every utterance equals, bit for bit, its
  result in a call on its slice of 256 utterances, and is zero behind its own end."""
  model = _model(pool, channels, force_bn)
  try:
    with _Clock(f"infer ragged c{channels} {name} {dtype} bn={force_bn or 'auto'}"):
      _run_wide(model, name, dtype, ragged=True)
  finally:
    _release(model)


def _dense_wide_top(pool):
  """(mel, audio) of the dense 64-channel wide_top call, checked against its slices; shared with the forward and loss cases."""
  sh = pool["shared"]
  if "dense" not in sh:
    model = _model(pool, 64)
    try:
      with _Clock("infer dense c64 wide_top torch.float16"):
        sh["dense"] = _run_wide(model, "wide_top", torch.float16, ragged=False, seed=12)
    finally:
      _release(model)
  return sh["dense"]


def test_wide_top_dense_batch_equals_slices_of_256(pool):
  """frames=None on both sides (wg_infer): the last accepted batch, 16 382 x 56 frames, against its slices."""
  mel, audio = _dense_wide_top(pool)
  assert audio.shape == (E.SHAPES["wide_top"].B, 256 * E.SHAPES["wide_top"].T)


def _rt_err(z, z_early, z_init, sigma):
  want = sigma * torch.cat([z_early, z_init], 1).float()
  return float((z.float() - want).double().pow(2).mean().sqrt())


@pytest.mark.parametrize("channels,name", [(64, "long_cross"), (64, "long_top"), (256, "long_top")])
def test_long_ragged_batch_equals_batch_of_one_calls(pool, channels, name):
  """Four utterances of 37, 864, 4000 and T frames in rows b * Fp with Fp in the hundreds of thousands: each equals its
  batch-of-one call bit for bit and is zero behind its end.  The batch-of-one call of the longest (Rp = 131 200 / 262 144)
  is itself beyond the pinned sizes, so its audio also goes through forward(), which must return the injected noise within
  the round-trip bound of tests/test_gpu_parity.py."""
  s = E.SHAPES[name]
  B, T = s.B, s.T
  dtype = torch.float16
  model = _model(pool, channels)
  try:
    with _Clock(f"infer ragged c{channels} {name} {dtype}"):
      _need_or_skip(model, B, T, B * (80 * T + 8 * 32 * T) * 6 + 2 * B * 256 * T * 2 + 32 * T * (8 + 14) * 6)
      frames = torch.tensor(E.LONG_FRAMES(T), dtype=torch.int32)
      mel, z_init, z_early = _inputs(B, T, dtype, 13, frames)
      with torch.no_grad():
        out = model.infer_with_noise(mel, z_init, [z_early], SIGMA, frames=frames.to(DEV))
        torch.cuda.synchronize()
        assert out.shape == (B, 256 * T) and bool(torch.isfinite(out).all())
        assert _zero_behind(out, frames.to(DEV))
        for b, f in enumerate(E.LONG_FRAMES(T)):
          one = model.infer_with_noise(mel[b:b + 1, :, :f].contiguous(), z_init[b:b + 1, :, :32 * f].contiguous(),
                                       [z_early[b:b + 1, :, :32 * f].contiguous()], SIGMA)
          assert torch.equal(out[b, :256 * f], one[0]), (name, b)
        # utterance 3's batch-of-one audio back through the flow
        z, log_s, _ = model((mel[3:4], one))
        err = _rt_err(z, z_early[3:4], z_init[3:4], SIGMA)
        print(f"\n{name} c{channels}: round trip of utterance 3 (1 x {T} frames), rms err {err:.3e}")
        assert err <= ROUND_TRIP_TOL[dtype]
        del z, log_s, one
      if channels == 64 and name == "long_top":
        pool["shared"]["long"] = (mel, out)
  finally:
    _release(model)


# ---------------------------------------------------------------------------------------------- no-grad forward
@pytest.mark.parametrize("force_bn", ["64", "128"])
@pytest.mark.parametrize("channels", [64, 256])
@pytest.mark.parametrize("T", [5, 37])
def test_forward_rows_do_not_depend_on_the_batch(pool, T, channels, force_bn):
  """wg_forward at small size: z and every log_s of a batch of 6 equal, bit for bit, those of two calls on 3 utterances
  each (the property the large forward cases rest on); log_det_W = B * L * logdet(W) scales with the batch exactly."""
  model = _model(pool, channels, force_bn)
  g = torch.Generator(device=DEV).manual_seed(21 + T)
  B, S = 6, 256 * T - 24                       # L = 32 T - 3: the last frame is partial
  mel = (torch.randn(B, 80, T, device=DEV, generator=g) * 2 - 5).clamp_(-11.5, 2.0).half()
  audio = (torch.rand(B, S, device=DEV, generator=g) * 0.6 - 0.3).half()
  with torch.no_grad():
    z, log_s, log_det = model((mel, audio))
    assert bool(torch.isfinite(z).all())
    for lo in (0, 3):
      z1, ls1, ld1 = model((mel[lo:lo + 3], audio[lo:lo + 3]))
      assert torch.equal(z[lo:lo + 3], z1), lo
      for k in range(len(log_s)):
        assert torch.equal(log_s[k][lo:lo + 3], ls1[k]), (lo, k)
      for k in range(len(log_det)):
        assert float(log_det[k]) == 2.0 * float(ld1[k])     # B L logdet rounded to fp32: a factor of two is exact


def _forward_vs_slices(model, mel, audio, step):
  """forward on the whole batch against forward on slices of `step` utterances: z and every log_s bit for bit.  log_det_W
  is B * L * logdet(W_k) rounded to fp32 once per call, so the slices' values cannot be compared bit for bit with the
  large call's (B differs).  Every value carries one fp32 rounding (2^-24 relative) and all slices have the same sign, so
  the fp64 sum of the slices and the large call's value are each within 2^-24 of the exact figure: they must agree to
  2^-22 relative (twice the sum of the two roundings).  Returns the large call's outputs."""
  B = mel.shape[0]
  with torch.no_grad():
    z, log_s, log_det = model((mel, audio))
    torch.cuda.synchronize()
    assert bool(torch.isfinite(z).all()) and all(bool(torch.isfinite(t).all()) for t in log_s)
    ld_sum = [0.0] * len(log_det)
    bad = []
    for lo in range(0, B, step):
      hi = min(lo + step, B)
      z1, ls1, ld1 = model((mel[lo:hi], audio[lo:hi]))
      if not torch.equal(z[lo:hi], z1):
        bad.append(("z", lo))
      for k in range(len(log_s)):
        if not torch.equal(log_s[k][lo:hi], ls1[k]):
          bad.append((f"log_s[{k}]", lo))
      for k in range(len(ld1)):
        ld_sum[k] += float(ld1[k])
      del z1, ls1
    assert not bad, bad[:16]
    for k in range(len(log_det)):
      assert abs(float(log_det[k]) - ld_sum[k]) <= 2.0 ** -22 * abs(ld_sum[k]), (k, float(log_det[k]), ld_sum[k])
  return z, log_s, log_det


def _forward_wide_top(pool):
  sh = pool["shared"]
  if "fwd" not in sh:
    mel, audio = _dense_wide_top(pool)
    model = _model(pool, 64)
    B, T = mel.shape[0], mel.shape[2]
    try:
      with _Clock("forward c64 wide_top torch.float16"):
        _need_or_skip(model, B, T, B * 32 * T * (8 + 14) * 6 * 2, forward=True)
        sh["fwd"] = _forward_vs_slices(model, mel, audio, SLICE)
    finally:
      _release(model)
  return sh["fwd"]


def test_forward_wide_top_equals_slices_of_256(pool):
  """wg_forward on the audio of the dense 16 382-utterance call: z and every log_s equal the slice calls bit for bit."""
  z, log_s, log_det = _forward_wide_top(pool)
  assert z.shape == (E.SHAPES["wide_top"].B, 8, 32 * E.SHAPES["wide_top"].T)


def test_forward_long_top_equals_batch_of_one_calls(pool):
  """wg_forward on 4 x 262 104 frames (the audio of the long_top inference case) against its four batch-of-one calls."""
  if "long" not in pool["shared"]:
    pytest.fail("the 64-channel long_top inference case did not leave its audio (it runs first in this module)")
  mel, audio = pool["shared"].pop("long")
  model = _model(pool, 64)
  B, T = mel.shape[0], mel.shape[2]
  try:
    with _Clock("forward c64 long_top torch.float16"):
      _need_or_skip(model, B, T, B * 32 * T * (8 + 14) * 6 * 2, forward=True)
      _forward_vs_slices(model, mel, audio, 1)
  finally:
    _release(model)


def test_loss_at_scale_matches_fp64(pool):
  """WaveGlowLoss(1.0) on the forward outputs of wide_top (235 M elements of z) against the same formula in fp64 torch on
  the same z, log_s, log_det_W (train.py:31-45)."""
  z, log_s, log_det = _forward_wide_top(pool)
  with _Clock("loss c64 wide_top"):
    with torch.no_grad():
      loss = float(WaveGlowLoss(1.0)((z, log_s, log_det)))
      total = float(z.double().pow(2).sum()) / 2.0
      for t in log_s:
        total -= float(t.double().sum())
      for t in log_det:
        total -= float(t.double())
      ref = total / z.numel()
  print(f"\nloss at scale: {loss:.6f}, fp64 {ref:.6f}")
  assert abs(loss - ref) <= 2e-3 * max(1.0, abs(ref))


# ---------------------------------------------------------------------------------------------- refusals
def _small_call(model):
  mel, z_init, z_early = _inputs(3, 9, torch.float16, 31)
  with torch.no_grad():
    audio = model.infer_with_noise(mel, z_init, [z_early], SIGMA)
    z, _, _ = model((mel, audio))
  torch.cuda.synchronize()
  return audio, z


@pytest.mark.parametrize("direction", ["infer", "forward"])
@pytest.mark.parametrize("name", E.REFUSED)
def test_first_refused_shapes_raise_before_anything_is_allocated(pool, name, direction):
  """One utterance / one 128-row step past the last accepted geometry: WgError that names the limit, no allocation (not
  even a transient one: the peak stays where the level was), no launch, and the device gives the same bits afterwards."""
  s = E.SHAPES[name]
  B, T = s.B, s.T
  model = _model(pool, 64)
  eng = model._get_engine(torch.device(DEV))
  before = _small_call(model)
  _release(model)
  mel = torch.zeros(B, 80, T, dtype=torch.float16, device=DEV)
  if direction == "infer":
    args = (mel, torch.zeros(B, 6, 32 * T, dtype=torch.float16, device=DEV), [torch.zeros(B, 2, 32 * T, dtype=torch.float16, device=DEV)], SIGMA)
    call = lambda: model.infer_with_noise(*args)
  else:
    audio = torch.zeros(B, 256 * T, dtype=torch.float16, device=DEV)
    call = lambda: model((mel, audio))
  # Tensors that earlier tests left in reference cycles (a caught exception's traceback holds its frame's locals) are
  # freed whenever the collector next runs -- inside the call below, for instance, which would lower the level under the
  # measurement.  Collect them first, so that the level can only move through the call itself.
  gc.collect()
  torch.cuda.synchronize()
  torch.cuda.reset_peak_memory_stats()
  level = torch.cuda.memory_allocated()
  with torch.no_grad(), pytest.raises(_lib.WgError) as ei:
    call()
  msg = str(ei.value)
  del ei                                          # the traceback refers to this frame: no cycle is left behind
  assert "batch too large" in msg and str(E.MAX_RP) in msg and "4 GiB" in msg, msg
  assert torch.cuda.memory_allocated() == level and torch.cuda.max_memory_allocated() == level
  assert not eng._ws
  # the C entry points themselves: range before workspace size, nothing launched
  ws = torch.zeros(256, dtype=torch.uint8, device=DEV)
  stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
  if direction == "infer":
    ze = (C.c_void_p * 1)(args[2][0].data_ptr())
    rc = eng.lib.wg_infer(eng.handle, mel.data_ptr(), None, args[1].data_ptr(), ze, 1, SIGMA, ws.data_ptr(), B, T,
                          _lib.WG_F16, ws.data_ptr(), ws.numel(), stream)
  else:
    ls = (C.c_void_p * 4)(*[ws.data_ptr()] * 4)
    ld = (C.c_float * 4)()
    rc = eng.lib.wg_forward(eng.handle, mel.data_ptr(), None, audio.data_ptr(), ws.data_ptr(), ls, ld, B, T, 256 * T, _lib.WG_F16,
                            ws.data_ptr(), ws.numel(), stream)
  assert rc != 0 and b"batch too large" in eng.lib.wg_last_error()
  assert eng.lib.wg_infer_workspace_bytes(eng.handle, B, T) == 0
  assert eng.lib.wg_forward_workspace_bytes(eng.handle, B, T, 256 * T) == 0
  torch.cuda.synchronize()
  assert not bool(ws.any())
  del mel, call
  after = _small_call(model)
  assert torch.equal(before[0], after[0]) and torch.equal(before[1], after[1])
  _release(model)
