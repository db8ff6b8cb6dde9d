"""GPU: every direction of the flow path held to PER-COLUMN bounds at utterance edges and tile seams (tests/_seams.py).

The other comparisons with an oracle are one norm over a whole tensor, in which a kernel that is wrong in the first or last
column of an utterance, in the frames on either side of a tile seam, or in a dilated tap that reads a guard row is diluted
by all the columns that are right (tests/test_seams_cpu.py puts that on record with planted faults).  The planes are
polyphase, so a tile of the WN layer kernel or of the plane GEMM is 64 or 128 ROWS (frames, guard rows included) of one
phase block.  The edge cases (seam_c64, seam_c256: 288 columns, dilation 128 inside the utterance) lie in ONE tile and
pin the utterance ends and the taps into guard rows in every direction; the tile cases (tile64_*, tile128_*: B 4 x T 10
and B 8 x T 9) put row 64 / row 128 of the phase blocks on a frame in the middle of an utterance and run the directions
under a cotangent on the two frames on either side of that seam.  The far end of the accepted depth: seam_l10_c64,
seam_l10_c256 and seam_l9_c128 (B 1 x T 18, 576 columns, 16 and 8 guard frames, ONE tile) move real data through the taps of
dilation 256 and 512 in every direction, under the "edge" cotangent and under "reach" (the columns whose deep taps land on
the utterance's first and last column); seam_c128 and seam_c512 run the other two channel counts at the 8-layer edge shape;
tile_l10_* (B 2 x T 52) have rows 64 and 128 inside an utterance with real frames under the 16-row taps on both sides;
first64_* (B 4 x T 12) have row 64 on frame 0 of utterance 3.  WG_FORCE_BN takes the tile widths the channel count has: at
512 channels the kernels have 64-wide tiles only, the variable is ignored at 128 and every test of seam_c512 runs once.
Every quantity with a time axis is compared column by
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
from waveglow_amd._lib import WgError
from waveglow_amd.model import WaveGlow, WaveGlowLoss

pytestmark = pytest.mark.gpu

# WG_FORCE_BN: S.tile_widths -- both tile widths of the WN layer kernel up to 256 channels, the one there is at 512
# (WG_TRAIN_CT, WG_TRAIN_MT) of test_gpu_train.test_train_step_every_tile_width: the launcher's own choice, and the narrowest
# plane-GEMM tile (64 columns, 128-row groups)
PLANE_TILES = [None, ("2", "1")]
# (case, weight-norm form): the new cases in both forms
SYNTH_FORMS = [("seam_c64", True), ("seam_c64", False), ("seam_c256", True)] + \
              [(n, normed) for n in S.DEEP_IDS + S.WIDE_IDS for normed in (True, False)]
PLANE_IDS = ["auto", "ct2mt1"]


def _grid(names, where=False, planes=False, forms=False):
  """pytest.params (name[, normed][, where], bn[, plane]) with the ids that stacked parametrize decorators gave the first
  cases: every tile width the case's channel count has, every local cotangent of the case."""
  out = []
  for item in names:
    name, normed = item if forms else (item, None)
    for w in (S.cotangents(name) if where else [None]):
      for bn in S.tile_widths(S.CASES[name][0]["n_channels"]):
        for plane, pid in (zip(PLANE_TILES, PLANE_IDS) if planes else [(None, None)]):
          vals = [v for v, on in ((name, True), (normed, forms), (w, where), (bn, True), (plane, planes)) if on]
          ids = [str(v) for v, on in ((name, True), (normed, forms), (w, where), (bn, True), (pid, planes)) if on]
          out.append(pytest.param(*vals, id="-".join(ids)))
  return out


@pytest.fixture(autouse=True)
def _poisoned_gradient_buffers(monkeypatch):
  """Gradient buffers start from NaN: an entry the library never writes makes grad_finite false."""
  monkeypatch.setenv("WG_TRAIN_POISON_GRADS", "1")


def _tiles(monkeypatch, bn, plane=None):
  monkeypatch.setenv("WG_FORCE_BN", bn)
  if plane is not None:
    monkeypatch.setenv("WG_TRAIN_CT", plane[0])
    monkeypatch.setenv("WG_TRAIN_MT", plane[1])


def _hold(got, ref, yard, what, only=None, case=None):
  miss = S.check(got, ref, yard, what, only=only, case=case)
  assert not miss, f"{what}: beyond 3 x yardstick (ratio to the yardstick, quantity, position): {miss[:8]}"


def _values(q):
  return q == "z" or q.startswith("log_s.")


# ------------------------------------------------------------------ inference
@pytest.mark.parametrize("name,bn", _grid(S.EDGE_IDS))
def test_infer_fp32(name, bn, monkeypatch):
  _tiles(monkeypatch, bn)
  c = S._case(name, "inv")
  out = gpu_infer(build_model(c.hp, c.sd), c.mel, c.z_init, c.z_early, c.sigma)
  _hold({"audio": out}, S.oracle(name, "inv", False, "values"), S.yardstick(name, "inv", False, "values"),
        f"{name} bn{bn} infer fp32", case=c)


@pytest.mark.parametrize("name,bn", _grid(S.EDGE_IDS))
def test_infer_fp16_io(name, bn, monkeypatch):
  """fp16 I/O against the oracle on the fp16-rounded mel and noise.  The fp16 rounding of the output itself (up to 2^-11 of
  a column's own norm) is inside the figure and not inside the fp32 yardstick: measured 0.91 / 1.19 of it on seam_c64 /
  seam_c256, against 0.48 / 0.64 at fp32 I/O."""
  _tiles(monkeypatch, bn)
  c = S._case(name, "inv")
  out = gpu_infer(build_model(c.hp, c.sd), c.mel, c.z_init, c.z_early, c.sigma, torch.float16)
  _hold({"audio": out}, S.oracle(name, "inv", False, "values", io16=True), S.yardstick(name, "inv", False, "values"),
        f"{name} bn{bn} infer fp16 io", case=c)


# ------------------------------------------------------------------ forward and the training step
@pytest.mark.parametrize("name,bn", _grid(S.EDGE_IDS))
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
        only=_values, case=c)


def _train(c, where, recompute=False):
  """One training forward and a backward on the weight-normed model: of WaveGlowLoss ("loss"), or of sum(z u) for a
  cotangent u on z through plain autograd on the module's output.  For a cotangent the loss scale of the gradient planes
  is set explicitly (the automatic one assumes the mean loss over all samples) -- before the forward, which is where the
  module reads it."""
  model = WaveGlow(c.hp)
  model.load_state_dict(c.sdn)
  model = model.to("cuda:0").train()
  model.recompute_activations = recompute
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


@pytest.mark.parametrize("name,bn,plane", _grid(S.EDGE_IDS, planes=True))
def test_train_step(name, bn, plane, monkeypatch):
  """WaveGlowLoss on the weight-normed model: z, every log_s, d mel and d audio per column; the parameter gradients as
  test_gpu_train.py checks them (GRAD_TOL, whole tensor)."""
  _tiles(monkeypatch, bn, plane)
  _hold_train_step(S._case(name, "fwd"), _train(S._case(name, "fwd"), "loss"), f"{name} bn{bn} plane {plane} train step")


def _hold_train_step(c, got, what):
  ref = S.oracle(c.name, "fwd", True, "loss")
  _hold(got, ref, S.yardstick(c.name, "fwd", True, "loss"), what, only=lambda q: not q.startswith("p/"), case=c)
  params = {q[2:]: t for q, t in ref.items() if q.startswith("p/")}
  assert set(params) == {q[2:] for q in got if q.startswith("p/")}
  _check({n: got[f"p/{n}"] for n in params}, params, what)


@pytest.mark.parametrize("bn", S.tile_widths(64))
def test_train_step_recompute(bn, monkeypatch):
  """The training step of seam_l10_c64 with activation recomputation (``model.recompute_activations``): the backward
  re-runs the layers of dilation 256 and 512 from the saved flow inputs; held to the bounds of test_train_step."""
  _tiles(monkeypatch, bn)
  c = S._case("seam_l10_c64", "fwd")
  _hold_train_step(c, _train(c, "loss", recompute=True), f"seam_l10_c64 bn{bn} train step, recompute mode")


@pytest.mark.parametrize("name,where,bn,plane", _grid(S.EDGE_IDS, where=True, planes=True))
def test_train_direction_under_local_cotangent(name, where, bn, plane, monkeypatch):
  """The backward of sum(z u), u non-zero on the first and last 32 columns of every utterance ("edge"), on the 32 columns
  on each side of column 128 ("col128"), or on the 32 columns on each side of the columns whose taps of dilation 64 and up
  land on the utterance's first and last column ("reach": the cases with 9 and 10 layers and with 128 and 512 channels; under
  "edge" the transposed taps of dilation 256 and 512 carry nothing to those columns): every parameter gradient within 3 x its whole-tensor yardstick under that cotangent,
  d audio and d mel per column."""
  _tiles(monkeypatch, bn, plane)
  c = S._case(name, "fwd")
  got = _train(c, where)
  ref = S.oracle(name, "fwd", True, where)
  assert {q for q in ref if q.startswith("p/")} == {q for q in got if q.startswith("p/")}
  _hold(got, ref, S.yardstick(name, "fwd", True, where), f"{name} bn{bn} plane {plane} training direction, {where} cotangent",
        case=c)


# ------------------------------------------------------------------ gradients through synthesis
def _synth_got(audio, g_mel, g_zi, g_ze):
  got = {"audio": audio, "d mel": g_mel, "d z_init": g_zi}
  got.update({f"d z_early.{i}": g for i, g in enumerate(g_ze)})
  return got


@pytest.mark.parametrize("name,normed,where,bn", _grid(SYNTH_FORMS, where=True, forms=True))
def test_infer_differentiable_frozen(name, normed, where, bn, monkeypatch):
  """The backward of sum(audio r), r non-zero on the first and last 256 samples ("edge"), on the 256 samples on each side
  of sample 8 x 128 ("col128"), or on the samples of the "reach" columns (tests/_seams.py): audio, d mel, d z_init and every d z_early per column."""
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
        f"{name} normed={normed} bn{bn} infer_differentiable frozen, {where} cotangent", case=c)
  assert all(p.grad is None for p in model.parameters())


@pytest.mark.parametrize("name,normed,where,bn", _grid(SYNTH_FORMS, where=True, forms=True))
def test_infer_differentiable_weight_grads(name, normed, where, bn, monkeypatch):
  """weight_grads=True under the same cotangents: the column quantities of the frozen call, and every parameter gradient
  within 3 x its whole-tensor yardstick under that cotangent.  A channel count that the weight-gradient path itself refuses
  (a WgError that names n_channels) is skipped on that refusal; no case is left out by a list."""
  _tiles(monkeypatch, bn)
  c = S._case(name, "inv")
  try:
    audio, grads, g_mel, g_zi, g_ze, _ = WGT._run(c, normed, c.cotangent(where))
  except WgError as e:
    if "n_channels" not in str(e):
      raise
    pytest.skip(f"refused by the library: {e}")
  got = _synth_got(audio, g_mel, g_zi, g_ze)
  got.update({f"p/{n}": g for n, g in grads.items()})
  ref = S.oracle(name, "inv", normed, where)
  assert {q for q in ref if q.startswith("p/")} == {f"p/{n}" for n in grads}
  _hold(got, ref, S.yardstick(name, "inv", normed, where),
        f"{name} normed={normed} bn{bn} infer_differentiable weight_grads, {where} cotangent", case=c)


# ------------------------------------------------------------------ a tile seam inside an utterance
SEAM_IDS = S.TILE_IDS + S.FIRST_IDS


def _seam_note(c, bn):
  if c.name in S.FIRST_IDS:
    row, b = c.first_seam()
    return f"{c.name} bn{bn} (row {row}: frame 0 of utterance {b} behind its own guard rows)"
  seams = "; ".join(f"row {row}: frames {f - 1} | {f} of utterance {b}" for row, b, f in c.tile_seams())
  return f"{c.name} bn{bn} ({seams})"


def _local(name):
  """The cotangent of a case of this section: "seam", or "first" for a seam on an utterance's first frame."""
  return S.cotangents(name)[0]


@pytest.mark.parametrize("name,bn", _grid(SEAM_IDS))
def test_tile_seam_infer(name, bn, monkeypatch):
  """infer_with_noise with row 64 / 128 of the phase blocks on a frame inside an utterance: the audio per column (its
  yardstick does not depend on the cotangent; it is taken from the case's synthesis yardstick)."""
  _tiles(monkeypatch, bn)
  c = S._case(name, "inv")
  out = gpu_infer(build_model(c.hp, c.sd, normed=True), c.mel, c.z_init, c.z_early, c.sigma)
  _hold({"audio": out}, S.oracle(name, "inv", True, _local(name)), S.yardstick(name, "inv", True, _local(name)),
        _seam_note(c, bn) + " infer fp32", only=lambda q: q == "audio", case=c)


@pytest.mark.parametrize("name,bn", _grid(SEAM_IDS))
def test_tile_seam_forward(name, bn, monkeypatch):
  """The no-grad forward at the same cases: z and every log_s per column."""
  _tiles(monkeypatch, bn)
  c = S._case(name, "fwd")
  with torch.no_grad():
    z, log_s, _ = build_model(c.hp, c.sd, normed=True)((c.mel.cuda(), c.wav.cuda()))
  torch.cuda.synchronize()
  got = {"z": z}
  got.update({f"log_s.{k}": t for k, t in enumerate(log_s)})
  _hold(got, S.oracle(name, "fwd", True, _local(name)), S.yardstick(name, "fwd", True, _local(name)),
        _seam_note(c, bn) + " forward", only=_values, case=c)


@pytest.mark.parametrize("name,bn,plane", _grid(SEAM_IDS, planes=True))
def test_tile_seam_training_direction(name, bn, plane, monkeypatch):
  """The backward of sum(z u), u non-zero on the two frames on either side of the seam only: z, every log_s, d mel and
  d audio per column, every parameter gradient within 3 x its whole-tensor yardstick under that cotangent."""
  _tiles(monkeypatch, bn, plane)
  c = S._case(name, "fwd")
  _hold(_train(c, _local(name)), S.oracle(name, "fwd", True, _local(name)), S.yardstick(name, "fwd", True, _local(name)),
        _seam_note(c, bn) + f" plane {plane} training direction, {_local(name)} cotangent", case=c)


@pytest.mark.parametrize("name,bn", _grid(SEAM_IDS))
def test_tile_seam_infer_differentiable(name, bn, monkeypatch):
  """weight_grads=True on the weight-normed model under a cotangent on the 512 samples of the two frames at the seam: audio,
  d mel, d z_init, every d z_early per column, the parameter gradients whole-tensor."""
  _tiles(monkeypatch, bn)
  c = S._case(name, "inv")
  audio, grads, g_mel, g_zi, g_ze, _ = WGT._run(c, True, c.cotangent(_local(name)))
  got = _synth_got(audio, g_mel, g_zi, g_ze)
  got.update({f"p/{n}": g for n, g in grads.items()})
  _hold(got, S.oracle(name, "inv", True, _local(name)), S.yardstick(name, "inv", True, _local(name)),
        _seam_note(c, bn) + f" infer_differentiable weight_grads, {_local(name)} cotangent", case=c)
