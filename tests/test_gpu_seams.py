"""GPU: every direction of the flow path held to PER-COLUMN bounds at utterance edges and tile seams (tests/_seams.py).

The other comparisons with an oracle are one norm over a whole tensor, in which a kernel that is wrong in the first or last
column of an utterance, in the frames on either side of a tile seam, or in a dilated tap that reads a guard row is diluted
by all the columns that are right (tests/test_seams_cpu.py puts that on record with planted faults).  The planes are
polyphase, so a tile of the WN layer kernel or of the plane GEMM is 64 or 128 ROWS (frames, guard rows included) of one
phase block.  The edge cases (seam_c64, seam_c256: 288 columns, dilation 128 inside the utterance) lie in ONE tile and
pin the utterance ends and the taps into guard rows in every direction; the tile cases (tile64_*, tile128_*: B 4 x T 10
and B 8 x T 9) put row 64 / row 128 of the phase blocks on a frame in the middle of an utterance and run the directions
under a cotangent on the two frames on either side of that seam.  Every quantity with a time axis is compared column by
column against the fp64 oracle on the inputs the kernel received,

  max over (b, j) of || got[b, :, j] - ref[b, :, j] || / rms column norm of ref  <=  3 x yardstick,

the yardstick being the same figure for the fp16-operand emulation of the documented design (three input draws x three
dithered realisations of the roundings, computed here on the CPU and cached per case).  Parameter gradients keep the
whole-tensor statistic and are made sensitive by cotangents that are non-zero at the utterance ends, around column 128
(interior columns), or on the two frames at a tile seam only.  Every test prints, per quantity, the device's worst column, where it is, the yardstick and the
ratio; DESIGN.md section 4c has the measured ratios.
"""
import pytest
import torch

import _seams as S
import test_gpu_infer_grads as IG
import test_gpu_infer_weight_grads as WGT
from _cases import _check
from test_gpu_parity import build_model, gpu_infer
from waveglow_amd.model import WaveGlow, WaveGlowLoss

pytestmark = pytest.mark.gpu

BN = ["128", "64"]                                   # WG_FORCE_BN: both tile widths of the WN layer kernel
# (WG_TRAIN_CT, WG_TRAIN_MT) of test_gpu_train.test_train_step_every_tile_width: the launcher's own choice, and the narrowest
# plane-GEMM tile (64 columns, 128-row groups)
PLANE_TILES = [None, ("2", "1")]
SYNTH_FORMS = [("seam_c64", True), ("seam_c64", False), ("seam_c256", True)]      # (case, weight-norm form)


@pytest.fixture(autouse=True)
def _poisoned_gradient_buffers(monkeypatch):
  """Gradient buffers start from NaN: an entry the library never writes makes grad_finite false."""
  monkeypatch.setenv("WG_TRAIN_POISON_GRADS", "1")


def _tiles(monkeypatch, bn, plane=None):
  monkeypatch.setenv("WG_FORCE_BN", bn)
  if plane is not None:
    monkeypatch.setenv("WG_TRAIN_CT", plane[0])
    monkeypatch.setenv("WG_TRAIN_MT", plane[1])


def _hold(got, ref, yard, what, only=None):
  miss = S.check(got, ref, yard, what, only=only)
  assert not miss, f"{what}: beyond 3 x yardstick (ratio to the yardstick, quantity, position): {miss[:8]}"


def _values(q):
  return q == "z" or q.startswith("log_s.")


# ------------------------------------------------------------------ inference
@pytest.mark.parametrize("bn", BN)
@pytest.mark.parametrize("name", S.IDS)
def test_infer_fp32(name, bn, monkeypatch):
  _tiles(monkeypatch, bn)
  c = S._case(name, "inv")
  out = gpu_infer(build_model(c.hp, c.sd), c.mel, c.z_init, c.z_early, c.sigma)
  _hold({"audio": out}, S.oracle(name, "inv", False, "values"), S.yardstick(name, "inv", False, "values"),
        f"{name} bn{bn} infer fp32")


@pytest.mark.parametrize("bn", BN)
@pytest.mark.parametrize("name", S.IDS)
def test_infer_fp16_io(name, bn, monkeypatch):
  """fp16 I/O against the oracle on the fp16-rounded mel and noise.  The fp16 rounding of the output itself (up to 2^-11 of
  a column's own norm) is inside the figure and not inside the fp32 yardstick: measured 0.91 / 1.19 of it on seam_c64 /
  seam_c256, against 0.48 / 0.64 at fp32 I/O."""
  _tiles(monkeypatch, bn)
  c = S._case(name, "inv")
  out = gpu_infer(build_model(c.hp, c.sd), c.mel, c.z_init, c.z_early, c.sigma, torch.float16)
  _hold({"audio": out}, S.oracle(name, "inv", False, "values", io16=True), S.yardstick(name, "inv", False, "values"),
        f"{name} bn{bn} infer fp16 io")


# ------------------------------------------------------------------ forward and the training step
@pytest.mark.parametrize("bn", BN)
@pytest.mark.parametrize("name", S.IDS)
def test_forward_no_grad(name, bn, monkeypatch):
  """The no-grad forward: z and every log_s."""
  _tiles(monkeypatch, bn)
  c = S._case(name, "fwd")
  model = build_model(c.hp, c.sd, normed=True)
  with torch.no_grad():
    z, log_s, _ = model((c.mel.cuda(), c.wav.cuda()))
  torch.cuda.synchronize()
  got = {"z": z}
  got.update({f"log_s.{k}": t for k, t in enumerate(log_s)})
  assert len(got) == 1 + c.hp.n_flows
  _hold(got, S.oracle(name, "fwd", True, "loss"), S.yardstick(name, "fwd", True, "loss"), f"{name} bn{bn} forward",
        only=_values)


def _train(c, where):
  """One training forward and a backward on the weight-normed model: of WaveGlowLoss ("loss"), or of sum(z u) for a
  cotangent u on z through plain autograd on the module's output.  For a cotangent the loss scale of the gradient planes
  is set explicitly (the automatic one assumes the mean loss over all samples) -- before the forward, which is where the
  module reads it."""
  model = WaveGlow(c.hp)
  model.load_state_dict(c.sdn)
  model = model.to("cuda:0").train()
  model.zero_grad()
  if where != "loss":
    model.grad_scale = c.grad_scale()
  mel, wav = c.mel.cuda().requires_grad_(True), c.wav.cuda().requires_grad_(True)
  y = model((mel, wav))
  if where == "loss":
    WaveGlowLoss(1.0)(y, None).backward()
  else:
    (y[0] * c.cotangent(where).cuda()).sum().backward()
  torch.cuda.synchronize()
  assert bool(model.grad_finite), "an entry of a (NaN-poisoned) gradient buffer was left unwritten, or a plane overflowed"
  got = {"z": y[0].detach(), "d mel": mel.grad, "d audio": wav.grad}
  got.update({f"log_s.{k}": t.detach() for k, t in enumerate(y[1])})
  got.update({f"p/{n}": p.grad.detach().float().cpu() for n, p in model.named_parameters()})
  return got


@pytest.mark.parametrize("plane", PLANE_TILES, ids=["auto", "ct2mt1"])
@pytest.mark.parametrize("bn", BN)
@pytest.mark.parametrize("name", S.IDS)
def test_train_step(name, bn, plane, monkeypatch):
  """WaveGlowLoss on the weight-normed model: z, every log_s, d mel and d audio per column; the parameter gradients as
  test_gpu_train.py checks them (GRAD_TOL, whole tensor)."""
  _tiles(monkeypatch, bn, plane)
  c = S._case(name, "fwd")
  got = _train(c, "loss")
  ref = S.oracle(name, "fwd", True, "loss")
  what = f"{name} bn{bn} plane {plane} train step"
  _hold(got, ref, S.yardstick(name, "fwd", True, "loss"), what, only=lambda q: not q.startswith("p/"))
  params = {q[2:]: t for q, t in ref.items() if q.startswith("p/")}
  assert set(params) == {q[2:] for q in got if q.startswith("p/")}
  _check({n: got[f"p/{n}"] for n in params}, params, what)


@pytest.mark.parametrize("plane", PLANE_TILES, ids=["auto", "ct2mt1"])
@pytest.mark.parametrize("bn", BN)
@pytest.mark.parametrize("where", ["edge", "col128"])
@pytest.mark.parametrize("name", S.IDS)
def test_train_direction_under_local_cotangent(name, where, bn, plane, monkeypatch):
  """The backward of sum(z u), u non-zero on the first and last 32 columns of every utterance ("edge") or on the 32 columns
  on each side of column 128 ("col128"): every parameter gradient within 3 x its whole-tensor yardstick under that cotangent,
  d audio and d mel per column."""
  _tiles(monkeypatch, bn, plane)
  c = S._case(name, "fwd")
  got = _train(c, where)
  ref = S.oracle(name, "fwd", True, where)
  assert {q for q in ref if q.startswith("p/")} == {q for q in got if q.startswith("p/")}
  _hold(got, ref, S.yardstick(name, "fwd", True, where), f"{name} bn{bn} plane {plane} training direction, {where} cotangent")


# ------------------------------------------------------------------ gradients through synthesis
def _synth_got(audio, g_mel, g_zi, g_ze):
  got = {"audio": audio, "d mel": g_mel, "d z_init": g_zi}
  got.update({f"d z_early.{i}": g for i, g in enumerate(g_ze)})
  return got


@pytest.mark.parametrize("bn", BN)
@pytest.mark.parametrize("where", ["edge", "col128"])
@pytest.mark.parametrize("name,normed", SYNTH_FORMS)
def test_infer_differentiable_frozen(name, normed, where, bn, monkeypatch):
  """The backward of sum(audio r), r non-zero on the first and last 256 samples ("edge") or on the 256 samples on each side
  of sample 8 x 128 ("col128"): audio, d mel, d z_init and every d z_early per column."""
  _tiles(monkeypatch, bn)
  c = S._case(name, "inv")
  model = IG._frozen(c.hp, c.sd, normed)
  mel, zi, ze = IG._inputs(c)
  audio = model.infer_differentiable(mel, c.sigma, z_init=zi, z_early=ze)
  (audio * c.cotangent(where).cuda()).sum().backward()
  torch.cuda.synchronize()
  assert bool(model.grad_finite), "a gradient plane overflowed at the automatic loss scale"
  ref = {q: t for q, t in S.oracle(name, "inv", normed, where).items() if not q.startswith("p/")}
  assert len(ref) == 3 + len(ze)
  _hold(_synth_got(audio.detach(), mel.grad, zi.grad, [z.grad for z in ze]), ref, S.yardstick(name, "inv", normed, where),
        f"{name} normed={normed} bn{bn} infer_differentiable frozen, {where} cotangent")
  assert all(p.grad is None for p in model.parameters())


@pytest.mark.parametrize("bn", BN)
@pytest.mark.parametrize("where", ["edge", "col128"])
@pytest.mark.parametrize("name,normed", SYNTH_FORMS)
def test_infer_differentiable_weight_grads(name, normed, where, bn, monkeypatch):
  """weight_grads=True under the same cotangents: the column quantities of the frozen call, and every parameter gradient
  within 3 x its whole-tensor yardstick under that cotangent."""
  _tiles(monkeypatch, bn)
  c = S._case(name, "inv")
  audio, grads, g_mel, g_zi, g_ze, _ = WGT._run(c, normed, c.cotangent(where))
  got = _synth_got(audio, g_mel, g_zi, g_ze)
  got.update({f"p/{n}": g for n, g in grads.items()})
  ref = S.oracle(name, "inv", normed, where)
  assert {q for q in ref if q.startswith("p/")} == {f"p/{n}" for n in grads}
  _hold(got, ref, S.yardstick(name, "inv", normed, where),
        f"{name} normed={normed} bn{bn} infer_differentiable weight_grads, {where} cotangent")


# ------------------------------------------------------------------ a tile seam inside an utterance
def _seam_note(c, bn):
  row, b, f = c.tile_seam()
  return f"{c.name} bn{bn} (row {row}: frames {f - 1} | {f} of utterance {b})"


@pytest.mark.parametrize("bn", BN)
@pytest.mark.parametrize("name", S.TILE_IDS)
def test_tile_seam_infer(name, bn, monkeypatch):
  """infer_with_noise with row 64 / 128 of the phase blocks on a frame inside an utterance: the audio per column (its
  yardstick does not depend on the cotangent; it is taken from the case's synthesis yardstick)."""
  _tiles(monkeypatch, bn)
  c = S._case(name, "inv")
  out = gpu_infer(build_model(c.hp, c.sd, normed=True), c.mel, c.z_init, c.z_early, c.sigma)
  _hold({"audio": out}, S.oracle(name, "inv", True, "seam"), S.yardstick(name, "inv", True, "seam"),
        _seam_note(c, bn) + " infer fp32", only=lambda q: q == "audio")


@pytest.mark.parametrize("bn", BN)
@pytest.mark.parametrize("name", S.TILE_IDS)
def test_tile_seam_forward(name, bn, monkeypatch):
  """The no-grad forward at the same cases: z and every log_s per column."""
  _tiles(monkeypatch, bn)
  c = S._case(name, "fwd")
  with torch.no_grad():
    z, log_s, _ = build_model(c.hp, c.sd, normed=True)((c.mel.cuda(), c.wav.cuda()))
  torch.cuda.synchronize()
  got = {"z": z}
  got.update({f"log_s.{k}": t for k, t in enumerate(log_s)})
  _hold(got, S.oracle(name, "fwd", True, "seam"), S.yardstick(name, "fwd", True, "seam"), _seam_note(c, bn) + " forward",
        only=_values)


@pytest.mark.parametrize("plane", PLANE_TILES, ids=["auto", "ct2mt1"])
@pytest.mark.parametrize("bn", BN)
@pytest.mark.parametrize("name", S.TILE_IDS)
def test_tile_seam_training_direction(name, bn, plane, monkeypatch):
  """The backward of sum(z u), u non-zero on the two frames on either side of the seam only: z, every log_s, d mel and
  d audio per column, every parameter gradient within 3 x its whole-tensor yardstick under that cotangent."""
  _tiles(monkeypatch, bn, plane)
  c = S._case(name, "fwd")
  _hold(_train(c, "seam"), S.oracle(name, "fwd", True, "seam"), S.yardstick(name, "fwd", True, "seam"),
        _seam_note(c, bn) + f" plane {plane} training direction, seam cotangent")


@pytest.mark.parametrize("bn", BN)
@pytest.mark.parametrize("name", S.TILE_IDS)
def test_tile_seam_infer_differentiable(name, bn, monkeypatch):
  """weight_grads=True on the weight-normed model under a cotangent on the 512 samples of the two frames at the seam: audio,
  d mel, d z_init, every d z_early per column, the parameter gradients whole-tensor."""
  _tiles(monkeypatch, bn)
  c = S._case(name, "inv")
  audio, grads, g_mel, g_zi, g_ze, _ = WGT._run(c, True, c.cotangent("seam"))
  got = _synth_got(audio, g_mel, g_zi, g_ze)
  got.update({f"p/{n}": g for n, g in grads.items()})
  _hold(got, S.oracle(name, "inv", True, "seam"), S.yardstick(name, "inv", True, "seam"),
        _seam_note(c, bn) + " infer_differentiable weight_grads, seam cotangent")
