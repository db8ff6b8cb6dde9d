"""Shared by the hot-weight tests and tests/golden/make_golden_hot.py: weights at the dynamic range of a TRAINED vocoder
(saturated gates, ``log_s`` of several units, 1x1 matrices far from orthogonal), the calibration that makes them, and the
yardstick the GPU tests hold the HIP path to.

``synthetic.make_state_dict`` keeps every gate pre-activation below about 6, ``log_s`` below 0.7 and every ``W_k`` exactly
orthogonal.  Plainly scaling those weights gives a chaotic flow (z reaches 1e11 at 12 flows), so the hot family is
calibrated like actnorm, sequentially and data-dependently, in fp64 on a fixed batch (``calibrate``): per flow, in the
direction under test, ``end.weight`` x s_end, ``in_layers`` / ``cond_layer`` weights x gate, ``W_k`` (or ``W_k^-1``) =
Q diag(logspace(1 .. cond)) Q2^T with its rows rescaled so that the state leaves the 1x1 step with unit channel std, and the
``log_s`` rows of ``end.bias`` shifted so that mean(log_s) = -+ var(log_s) / 2.  The two directions need separate weight
sets: a flow calibrated for analysis is not invertible in practice from a rounded z.

Only the calibrated tensors (``convinv.k.conv.weight``, ``WN.k.end.bias``: a few hundred floats per set) are stored in the
fixture; the rest is ``synthetic.make_state_dict`` times constants, which regenerates bit for bit anywhere.

``emulated`` is the fp64 oracle with the fp16 roundings DESIGN.md sections 2 / 3 document and nothing else: fp16 MFMA
operands (the ``in_layers`` / ``res`` / ``cond_layer`` / ``upsample`` weights, the mel, the ``x`` / ``acts`` / ``spect``
planes), fp16 saved tanh / sigmoid for the gate's derivative, fp16 gradient planes (d x, d pre, d out, d spect) at the loss
scale; the flow state, the accumulation, ``W_end W_skip`` (hi + lo halves) and the 1x1 step are left unrounded.  The gate in
it is plain ``tanh * sigmoid``.  Its error against the fp64 oracle, per case and quantity, is the yardstick.
"""
import os
import zlib

import numpy as np
import torch
import torch.nn.functional as F

import _corners as K
from _cases import oracle_cfg_from_hp
from waveglow_amd import synthetic
from waveglow_amd.hparams import HParams

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
SIGMA = 0.7
CROP = 96
YARD_SEEDS = (0, 1, 2)          # input draws of the yardstick; draw 0 is the fixture's own batch
BOUND_FACTOR = 3.0              # GPU bound = 3 x yardstick
FLOOR = 1e-7                    # the absolute floor of _cases._check
DIRECTIONS = ("fwd", "inv")     # weight sets: calibrated for analysis (forward / training) and for synthesis (infer)

# id: (HParams overrides, B, T, weight seed, {direction: (s_end, cond, gate)})
CASES = {
  "hot_f1": (dict(n_channels=64, n_layers=8, n_flows=1, n_early_every=4), 2, 6, 41,
             {"fwd": (6.0, 20.0, 6.0), "inv": (6.0, 20.0, 6.0)}),
  "hot_f2e": (dict(n_channels=64, n_layers=4, n_flows=2, n_early_every=1, n_early_size=2), 2, 6, 42,
              {"fwd": (6.0, 20.0, 6.0), "inv": (6.0, 20.0, 8.0)}),
  "hot_c256": (dict(n_channels=256, n_layers=8, n_flows=1, n_early_every=4), 1, 5, 43,
               {"fwd": (4.0, 20.0, 6.0), "inv": (5.0, 20.0, 6.0)}),
  "hot_f6": (dict(n_channels=64, n_layers=4, n_flows=6, n_early_every=2), 2, 6, 44,
             {"fwd": (4.2, 8.0, 2.8), "inv": (4.5, 10.0, 2.6)}),
}
IDS = list(CASES)
F6_LIMIT = 0.02                 # hot_f6: emulation yardstick at most 2 % (values: of the signal rms; gradients: relative L2)


# ---------------------------------------------------------------- precision model
class _Q(torch.autograd.Function):
  """x -> fp16(x) when ``fwd``; gradient g -> fp16(g scale) / scale when ``scale`` (else passed through unrounded).
  With a generator ``dither`` the value is moved by up to half an fp16 ulp (uniform, relative) before it is rounded:
  another realisation of the same roundings, for the spread study of test_hot_cpu.py."""

  @staticmethod
  def forward(ctx, x, fwd, scale, dither=None):
    ctx.scale = scale
    if not fwd:
      return x.clone()
    if dither is not None:
      x = x * (1 + (torch.rand(x.shape, generator=dither, dtype=x.dtype) - 0.5) * 2.0 ** -11)
    return x.half().to(x.dtype)

  @staticmethod
  def backward(ctx, g):
    if ctx.scale:
      g = (g * ctx.scale).half().to(g.dtype) / ctx.scale
    return g, None, None, None


class _Gate16(torch.autograd.Function):
  """tanh(a) sigmoid(b) whose derivative is taken from fp16 copies of tanh and sigmoid (the saved planes)."""

  @staticmethod
  def forward(ctx, a, b):
    t, s = torch.tanh(a), torch.sigmoid(b)
    ctx.save_for_backward(t.half().to(a.dtype), s.half().to(a.dtype))
    return t * s

  @staticmethod
  def backward(ctx, g):
    t, s = ctx.saved_tensors
    return g * s * (1 - t * t), g * t * s * (1 - s)


class _LogDet(torch.autograd.Function):
  """logdet W with the gradient W^-T, or with the planted fault ``W`` in its place."""

  @staticmethod
  def forward(ctx, W, fault):
    ctx.save_for_backward(W)
    ctx.fault = fault
    return torch.logdet(W)

  @staticmethod
  def backward(ctx, g):
    W, = ctx.saved_tensors
    return g * (W if ctx.fault else torch.inverse(W).t()), None


class _ConvWgradLast(torch.autograd.Function):
  """A dilated 3-tap conv with exact values and exact data and bias gradients whose WEIGHT gradient omits the term of the
  last column (a weight-gradient kernel whose last slab stops one column short)."""

  @staticmethod
  def forward(ctx, x, w, b, d):
    ctx.save_for_backward(x, w)
    ctx.d = d
    return F.conv1d(x, w, b, dilation=d, padding=d)

  @staticmethod
  def backward(ctx, g):
    x, w = ctx.saved_tensors
    d = ctx.d
    short = torch.cat([g[:, :, :-1], torch.zeros_like(g[:, :, -1:])], 2)
    return (torch.nn.grad.conv1d_input(x.shape, w, g, dilation=d, padding=d),
            torch.nn.grad.conv1d_weight(x, w.shape, short, dilation=d, padding=d), g.sum((0, 2)), None)


class Prec:
  """What is rounded (``r16``: fp16 operands and saved activations; ``gscale``: fp16 gradient planes at that loss scale),
  which fault is planted, and an optional trace of the pre-activations, the ``x`` / ``acts`` planes and ``log_s``.
  Faults: "winv_t" (W^T for W^-1 in synthesis), "logdet_grad" (W for W^-T in the logdet gradient), "no_logdet" (the logdet
  term dropped from the loss), "clamp4" (the tanh argument clamped to +-4: a clamp on a instead of on the exponent),
  "clamp_b4" (the same clamp on the sigmoid's argument), ("leak", k, i) (a batch leak: in layer i of flow k the right-hand
  padding of utterance b holds the first ``d`` columns of utterance b + 1; the last utterance keeps its zeros).
  Column faults of layer i of flow k (``d`` = 2^i; tests/_seams.py): ("drop_col", k, i) (the in-layer's input loses the
  utterance's last column), ("drop_tap", k, i) (the left tap of column ``d``, which reads column 0, is lost),
  ("seam", k, i, c) (at column ``c`` the left tap reads column c - d - 1 instead of c - d: a tile that stages its halo
  one column off), ("wgrad_last", k, i) (backward only: the gradient of ``in_layers.i.weight`` omits the last column's
  term; values and data gradients stay exact)."""

  def __init__(self, r16=False, gscale=None, fault=None, trace=None, dither=None):
    self.r16, self.gscale, self.fault, self.trace, self.dither = r16, gscale, fault, trace, dither

  def weight(self, t):                  # an fp16 MFMA operand whose gradient is accumulated in fp32
    return _Q.apply(t, True, None, self.dither) if self.r16 else t

  def plane(self, t):                   # an fp16 plane in both passes
    return _Q.apply(t, True, self.gscale, self.dither) if self.r16 else t

  def gplane(self, t):                  # fp32 forward (registers / the fp32 OUT rows), an fp16 plane in the backward
    return _Q.apply(t, False, self.gscale) if self.r16 and self.gscale else t

  def gate(self, a, b):
    if self.fault == "clamp4":
      a = a.clamp(-4.0, 4.0)
    elif self.fault == "clamp_b4":      # the same clamp on the sigmoid's argument: sigmoid(-4) = 0.018, not 0
      b = b.clamp(-4.0, 4.0)
    return _Gate16.apply(a, b) if self.r16 else torch.tanh(a) * torch.sigmoid(b)


EXACT = Prec()


def grad_scale(numel):
  """The automatic loss scale: 2^round(log2 N)."""
  return float(2.0 ** round(float(np.log2(numel))))


# ---------------------------------------------------------------- the model, in the dtype of its inputs
def compose(leaves):
  """Weight-norm form -> dense weights, differentiably (g v / ||v||, as oracle.grads_ref); dense keys pass through."""
  v1, v0 = "parametrizations.weight.original1", "parametrizations.weight.original0"
  dense = {}
  for k, v in leaves.items():
    if k.endswith(v1):
      dense[k[:-len(v1)] + "weight"] = torch._weight_norm(v, leaves[k[:-len(v1)] + v0], 0)
    elif not k.endswith(v0):
      dense[k] = v
  return dense


def _leaky_pad(x, d):
  """[B, C, L] -> [B, C, L + 2 d]: zeros on the left; on the right the first ``d`` columns of the NEXT utterance (what a
  tap that runs over missing guard rows would read), zeros behind them and behind the last utterance."""
  n = min(d, x.size(2))
  nxt = torch.cat([x[1:, :, :n], x.new_zeros(1, x.size(1), n)], 0)
  return torch.cat([x.new_zeros(x.size(0), x.size(1), d), x, nxt, x.new_zeros(x.size(0), x.size(1), d - n)], 2)


def _left_tap_shift(x, win, d, fault):
  """What "drop_tap" / "seam" add to the in-layer's output: zero but in one column, where the left tap's term W[..., 0] x[c - d]
  is removed and, for "seam", the term of column c - d - 1 (zero when that is in front of the utterance) put in its place."""
  L = x.size(2)
  c = d if fault[0] == "drop_tap" else fault[3]
  delta = x.new_zeros(x.size(0), win.size(0), L)
  if not d <= c < L:
    return delta
  lost = x[:, :, c - d]
  if fault[0] == "seam":
    lost = lost - (x[:, :, c - d - 1] if c - d - 1 >= 0 else torch.zeros_like(lost))
  onehot = torch.zeros(L, dtype=x.dtype)
  onehot[c] = 1.0
  return -(lost @ win[:, :, 0].t())[:, :, None] * onehot


def _wn(w, k, a0, spect, cfg, P):
  """WN.forward (model.py:115-138) -> [b ; log_s]."""
  C, p = cfg.n_channels, f"WN.{k}."
  x = P.plane(F.conv1d(a0, w[p + "start.weight"], w[p + "start.bias"]))
  cond = F.conv1d(spect, P.weight(w[p + "cond_layer.weight"]), w[p + "cond_layer.bias"])
  output = 0
  for i in range(cfg.n_layers):
    d = 2 ** i
    win, b_in = P.weight(w[p + f"in_layers.{i}.weight"]), w[p + f"in_layers.{i}.bias"]
    fault = P.fault if isinstance(P.fault, tuple) and P.fault[1:3] == (k, i) else (None,)
    if fault[0] == "leak":
      a = F.conv1d(_leaky_pad(x, d), win, b_in, dilation=d)
    elif fault[0] == "drop_col":
      a = F.conv1d(torch.cat([x[:, :, :-1], torch.zeros_like(x[:, :, -1:])], 2), win, b_in, dilation=d, padding=d)
    elif fault[0] == "wgrad_last":
      a = _ConvWgradLast.apply(x, win, b_in, d)
    else:
      a = F.conv1d(x, win, b_in, dilation=d, padding=d)
      if fault[0] in ("drop_tap", "seam"):
        a = a + _left_tap_shift(x, win, d, fault)
    a = P.gplane(a + cond[:, 2 * C * i:2 * C * (i + 1)])
    if P.trace is not None:
      P.trace.setdefault("a", []).append(a[:, :C].detach())
      P.trace.setdefault("b", []).append(a[:, C:].detach())
    acts = P.gate(a[:, :C], a[:, C:])
    acts = _Q.apply(acts, True, None, P.dither) if P.r16 else acts
    if P.trace is not None:             # the two fp16 planes a layer's GEMMs read (rounded when ``r16``)
      P.trace.setdefault("x", []).append(x.detach())
      P.trace.setdefault("acts", []).append(acts.detach())
    wrs, brs = w[p + f"res_skip_layers.{i}.weight"], w[p + f"res_skip_layers.{i}.bias"]
    if i < cfg.n_layers - 1:
      x = P.plane(x + F.conv1d(acts, P.weight(wrs[:C]), brs[:C]))
      output = output + F.conv1d(acts, wrs[C:], brs[C:])
    else:
      output = output + F.conv1d(acts, wrs, brs)
  return P.gplane(F.conv1d(output, w[p + "end.weight"], w[p + "end.bias"]))


def _squeeze(spect, g):
  spect = spect.unfold(2, g, g).permute(0, 2, 1, 3)
  return spect.contiguous().view(spect.size(0), spect.size(1), -1).permute(0, 2, 1)


def _spect(w, mel, cfg, P, n_samples=None):
  up = F.conv_transpose1d(P.plane(mel) if P.r16 else mel, P.weight(w["upsample.weight"]), w["upsample.bias"],
                          stride=cfg.upsample_stride)
  up = up[:, :, :-(cfg.upsample_kernel - cfg.upsample_stride)] if n_samples is None else up[:, :, :n_samples]
  return P.plane(_squeeze(up, cfg.n_group))


def _colmajor(W):
  return W.t().contiguous().t()


def infer(w, mel, z_init, z_early, sigma, cfg, P=EXACT):
  """WaveGlow.infer (model.py:223-274) with injected noise -> [B, 256 T]."""
  spect = _spect(w, mel, cfg, P)
  audio = sigma * z_init
  for k in reversed(range(cfg.n_flows)):
    h = audio.size(1) // 2
    a0, a1 = audio[:, :h], audio[:, h:]
    out = _wn(w, k, a0, spect, cfg, P)
    s, b = out[:, h:], out[:, :h]
    if P.trace is not None:
      P.trace.setdefault("log_s", {})[k] = s.detach()
    audio = torch.cat([a0, (a1 - b) / torch.exp(s)], 1)
    W = w[f"convinv.{k}.conv.weight"].squeeze(-1)
    W_inv = torch.inverse(_colmajor(W))
    if P.fault == "winv_t":             # the VALUE of the transpose; the derivative stays the inverse's
      W_inv = W.t().detach() + (W_inv - W_inv.detach())
    audio = F.conv1d(audio, W_inv[..., None])
    if k % cfg.n_early_every == 0 and k > 0:
      audio = torch.cat((sigma * z_early[k], audio), 1)
  return audio.permute(0, 2, 1).contiguous().view(audio.size(0), -1)


def forward(w, mel, audio, cfg, P=EXACT):
  """WaveGlow.forward (model.py:178-221) -> (z, [log_s], [log_det_W])."""
  spect = _spect(w, mel, cfg, P, audio.size(1))
  audio = audio.unfold(1, cfg.n_group, cfg.n_group).permute(0, 2, 1)
  outs, log_s_list, log_det_list = [], [], []
  for k in range(cfg.n_flows):
    if k % cfg.n_early_every == 0 and k > 0:
      outs.append(audio[:, :cfg.n_early_size])
      audio = audio[:, cfg.n_early_size:]
    W = w[f"convinv.{k}.conv.weight"].squeeze(-1)
    log_det_list.append(audio.size(0) * audio.size(2) * _LogDet.apply(W, P.fault == "logdet_grad"))
    audio = F.conv1d(audio, W[..., None])
    h = audio.size(1) // 2
    a0, a1 = audio[:, :h], audio[:, h:]
    out = _wn(w, k, a0, spect, cfg, P)
    log_s, b = out[:, h:], out[:, :h]
    if P.trace is not None:
      P.trace.setdefault("log_s", {})[k] = log_s.detach()
    log_s_list.append(log_s)
    audio = torch.cat([a0, torch.exp(log_s) * a1 + b], 1)
  outs.append(audio)
  return torch.cat(outs, 1), log_s_list, log_det_list


def loss_fn(z, log_s_list, log_det_list, P=EXACT, sigma=1.0):
  """WaveGlowLoss.forward (train.py:31-45)."""
  total = torch.sum(z * z) / (2 * sigma * sigma) - sum(torch.sum(ls) for ls in log_s_list)
  log_det_total = sum(log_det_list)
  if P.fault == "no_logdet":            # the VALUE of the loss without the term; its gradient stays
    log_det_total = log_det_total - log_det_total.detach()
  total = total - log_det_total
  return total / z.numel()


def _leaves(sd, dtype):
  return {k: v.to(dtype).clone().requires_grad_(True) for k, v in sd.items()}


def run_train(sd, mel, wav, cfg, P=EXACT, dtype=torch.float64, u=None):
  """Forward, loss and one backward on the state dict as given (weight-norm or dense form).  {quantity: tensor}:
  z, log_s.k, log_det (vector), loss, p/<parameter>, d mel, d audio.  With ``u`` the backward is that of sum(z u), a
  cotangent on z alone, instead of the loss's."""
  leaves = _leaves(sd, dtype)
  m, a = mel.to(dtype).clone().requires_grad_(True), wav.to(dtype).clone().requires_grad_(True)
  z, log_s, log_det = forward(compose(leaves), m, a, cfg, P)
  loss = loss_fn(z, log_s, log_det, P)
  names = list(leaves)
  gs = torch.autograd.grad(loss if u is None else (z * u.to(dtype)).sum(), [leaves[n] for n in names] + [m, a])
  out = {"z": z.detach(), "log_det": torch.stack([x.detach() for x in log_det]), "loss": loss.detach().reshape(1)}
  out.update({f"log_s.{k}": ls.detach() for k, ls in enumerate(log_s)})
  out.update({f"p/{n}": g for n, g in zip(names, gs[:len(names)])})
  out["d mel"], out["d audio"] = gs[-2], gs[-1]
  return out


def run_infer(sd, mel, z_init, z_early, sigma, cfg, P=EXACT, dtype=torch.float64, r=None):
  """Synthesis, and with ``r`` the backward of sum(audio r).  {quantity: tensor}: audio, p/<parameter>, d mel, d z_init,
  d z_early.i (i in the order infer_with_noise takes them: descending flow index)."""
  if r is None:
    with torch.no_grad():
      w = compose({k: v.to(dtype) for k, v in sd.items()})
      return {"audio": infer(w, mel.to(dtype), z_init.to(dtype), {k: v.to(dtype) for k, v in z_early.items()}, sigma, cfg, P)}
  leaves = _leaves(sd, dtype)
  m, zi = mel.to(dtype).clone().requires_grad_(True), z_init.to(dtype).clone().requires_grad_(True)
  ze = {k: v.to(dtype).clone().requires_grad_(True) for k, v in z_early.items()}
  keys = sorted(ze, reverse=True)
  audio = infer(compose(leaves), m, zi, ze, sigma, cfg, P)
  names = list(leaves)
  gs = torch.autograd.grad((audio * r.to(dtype)).sum(), [leaves[n] for n in names] + [m, zi] + [ze[k] for k in keys])
  out = {"audio": audio.detach()}
  out.update({f"p/{n}": g for n, g in zip(names, gs[:len(names)])})
  n = len(names)
  out["d mel"], out["d z_init"] = gs[n], gs[n + 1]
  out.update({f"d z_early.{i}": g for i, g in enumerate(gs[n + 2:])})
  return out


def emulated(direction, sd, inputs, cfg, fault=None, r=None, dither=None, u=None):
  """The fp64 oracle with the documented fp16 roundings (module docstring) on ``inputs``: (mel, wav) for "fwd",
  (mel, z_init, z_early) for "inv".  The gradient planes are rounded at the automatic loss scale.  ``dither``: _Q.
  ``u``: the cotangent on z of run_train."""
  if direction == "fwd":
    mel, wav = inputs
    n = wav.size(0) * (wav.size(1) // cfg.n_group) * cfg.n_group
    return run_train(sd, mel, wav, cfg, Prec(True, grad_scale(n), fault, dither=dither), u=u)
  mel, z_init, z_early = inputs
  return run_infer(sd, mel, z_init, z_early, SIGMA, cfg, Prec(True, grad_scale(mel.size(0) * 256 * mel.size(2)), fault, dither=dither), r=r)


def exact(direction, sd, inputs, cfg, fault=None, r=None, dtype=torch.float64, u=None):
  if direction == "fwd":
    return run_train(sd, inputs[0], inputs[1], cfg, Prec(fault=fault), dtype, u=u)
  return run_infer(sd, inputs[0], inputs[1], inputs[2], SIGMA, cfg, Prec(fault=fault), dtype, r=r)


def errors(got, ref):
  """{quantity: (||got - ref||, ||ref||)} in fp64."""
  out = {}
  for name, t in ref.items():
    g = got[name].detach().double().cpu()
    assert g.shape == t.shape, name
    out[name] = (float((g - t.double()).norm()), float(t.double().norm()))
  return out


# ---------------------------------------------------------------- inputs
def make_inputs(name, direction, draw=0):
  """The batch of a case: (mel, wav) or (mel, z_init, z_early).  Draw 0 is seeded as the other fixtures seed theirs (and
  the noise comes from the global CPU RNG in the order the reference's ``infer`` draws it); draws 1, 2 shift the seeds."""
  over, B, T, _, _ = CASES[name]
  return make_inputs_at(HParams(**over), B, T, direction, draw)


def make_inputs_at(hp, B, T, direction, draw=0, crop=CROP):
  """make_inputs for any model and shape (``crop``: samples the waveform is shorter than 256 T)."""
  mel = synthetic.make_mel(B, T, hp.n_mel_channels, seed=1234 + B + T + 1000 * draw)
  if direction == "fwd":
    # a waveform with loud and quiet stretches (Gaussian samples under a log-normal envelope of 64-sample blocks, clipped
    # to +-1) instead of the other fixtures' uniform noise: speech has a high crest factor, and it is the rare loud
    # sample that drives a trained gate deep into saturation while most of the gate stays in its working range
    g = torch.Generator().manual_seed(99 + T + 1000 * draw)
    S = 256 * T - crop
    env = torch.randn(B, (S + 63) // 64, generator=g).repeat_interleave(64, dim=1)[:, :S]
    return mel, (0.05 * torch.randn(B, S, generator=g) * torch.exp(0.6 * env)).clamp(-1.0, 1.0)
  z_init, z_early = K.replay_noise(hp, B, 32 * T, noise_seed(T, draw))
  return mel, z_init, z_early


def noise_seed(T, draw=0):
  return K.noise_seed(T) + 1000 * draw


def cotangent(name):
  """r of the synthesis gradients: the loss is sum(audio r)."""
  _, B, T, _, _ = CASES[name]
  return torch.randn(B, 256 * T, generator=torch.Generator().manual_seed(11)) / (B * 256 * T)


# ---------------------------------------------------------------- the weight family
def base_state_dict(hp, wseed, heat):
  """synthetic.make_state_dict times the fixed multipliers (an fp32 product with a constant: exact IEEE, the same bits
  anywhere); the 1x1 weights and ``end.bias`` are still the synthetic ones."""
  s_end, _, gate = heat
  sd = synthetic.make_state_dict(hp, seed=wseed)
  for key in sd:
    parts = key.split(".")
    if parts[0] == "WN" and parts[-1] == "weight":
      if parts[2] == "end":
        sd[key] = sd[key] * s_end
      elif parts[2] in ("in_layers", "cond_layer"):
        sd[key] = sd[key] * gate
  return sd


def _q2(name, k, c):
  g = torch.Generator().manual_seed(zlib.crc32(f"{name}.q2.{k}".encode()) & 0x7FFFFFFF)
  return torch.linalg.qr(torch.empty(c, c, dtype=torch.float64).normal_(generator=g))[0]


def _spread(Q, Q2, cond, y, target):
  """Q diag(logspace(1 .. cond)) Q2^T with rows rescaled so that every channel of M y has std ``target``; det > 0."""
  c = Q.size(0)
  M = Q @ torch.diag(torch.logspace(0.0, float(np.log10(cond)), c, dtype=torch.float64)) @ Q2.t()
  std = F.conv1d(y, M[..., None]).transpose(0, 1).flatten(1).std(dim=1)
  M = M * (target / std)[:, None]
  if torch.det(M) < 0:
    M[0] = -M[0]
  return M


def calibrate(name, direction):
  """The calibrated state dict (fp32, dense) of a case and direction: module docstring.  Every calibrated tensor is rounded
  to fp32 before the walk goes on, so the statistics are those of the weights that are stored.  Generator only."""
  over, B, T, wseed, heats = CASES[name]
  hp, heat = HParams(**over), heats[direction]
  cfg = oracle_cfg_from_hp(hp)
  sd = base_state_dict(hp, wseed, heat)
  w = {k: v.double() for k, v in sd.items()}
  inputs = make_inputs(name, direction)
  cond = heat[1]

  def put(key, t64):
    sd[key] = t64.float().view(sd[key].shape).contiguous()
    w[key] = sd[key].double()

  def center(k, h, out, sign):
    """Shift the log_s rows of end.bias: mean(log_s) = sign var(log_s) / 2 per row."""
    ls = out[:, h:].transpose(0, 1).flatten(1)
    shift = sign * 0.5 * ls.var(dim=1) - ls.mean(dim=1)
    bias = w[f"WN.{k}.end.bias"].clone()
    bias[h:] += shift
    old = w[f"WN.{k}.end.bias"]
    put(f"WN.{k}.end.bias", bias)
    return out + (w[f"WN.{k}.end.bias"] - old)[None, :, None]

  with torch.no_grad():
    if direction == "fwd":
      mel, wav = (t.double() for t in inputs)
      spect = _spect(w, mel, cfg, EXACT, wav.size(1))
      audio = wav.unfold(1, cfg.n_group, cfg.n_group).permute(0, 2, 1)
      for k in range(cfg.n_flows):
        if k % cfg.n_early_every == 0 and k > 0:
          audio = audio[:, cfg.n_early_size:]
        key = f"convinv.{k}.conv.weight"
        put(key, _spread(w[key].squeeze(-1), _q2(name, k, audio.size(1)), cond, audio, 1.0))
        audio = F.conv1d(audio, w[key])
        h = audio.size(1) // 2
        out = center(k, h, _wn(w, k, audio[:, :h], spect, cfg, EXACT), -1.0)
        audio = torch.cat([audio[:, :h], torch.exp(out[:, h:]) * audio[:, h:] + out[:, :h]], 1)
    else:
      mel, z_init = inputs[0].double(), inputs[1].double()
      spect = _spect(w, mel, cfg, EXACT)
      audio = SIGMA * z_init
      for k in reversed(range(cfg.n_flows)):
        h = audio.size(1) // 2
        out = center(k, h, _wn(w, k, audio[:, :h], spect, cfg, EXACT), +1.0)
        audio = torch.cat([audio[:, :h], (audio[:, h:] - out[:, :h]) / torch.exp(out[:, h:])], 1)
        key = f"convinv.{k}.conv.weight"
        Minv = _spread(w[key].squeeze(-1), _q2(name, k, audio.size(1)), cond, audio, 0.2 if k == 0 else 1.0)
        put(key, torch.inverse(Minv))
        audio = F.conv1d(audio, torch.inverse(w[key].squeeze(-1))[..., None])
        if k % cfg.n_early_every == 0 and k > 0:
          audio = torch.cat((SIGMA * inputs[2][k].double(), audio), 1)
  return sd


def calibrated_keys(hp):
  return [f"convinv.{k}.conv.weight" for k in range(hp.n_flows)] + [f"WN.{k}.end.bias" for k in range(hp.n_flows)]


def fixture_path(name):
  return os.path.join(GOLDEN, f"{name}.npz")


_npz = {}


def fixture(name):
  if name not in _npz:
    _npz[name] = np.load(fixture_path(name), allow_pickle=False)
  return _npz[name]


def hot_state_dict(name, direction):
  """The dense fp32 state dict of a case and direction, rebuilt from the generator, the multipliers and the fixture's
  calibrated tensors; its crc32 must be the one the fixture's generator saw."""
  over, _, _, wseed, heats = CASES[name]
  hp, fx = HParams(**over), fixture(name)
  assert tuple(float(v) for v in fx[f"{direction}/heat"]) == heats[direction] and int(fx["weight_seed"]) == wseed
  sd = base_state_dict(hp, wseed, heats[direction])
  for key in calibrated_keys(hp):
    t = torch.from_numpy(fx[f"{direction}/w/{key}"])
    assert t.shape == sd[key].shape, key
    sd[key] = t
  assert K.weights_crc(sd) == int(fx[f"{direction}/weights_crc32"]), f"{name}/{direction}: the weights changed"
  return sd


class Hot:
  """A case and direction: hp, cfg, sd (dense), sdn (weight-norm form), inputs, and the fixture's records."""

  def __init__(self, name, direction):
    over, self.B, self.T, self.wseed, heats = CASES[name]
    self.name, self.direction, self.heat = name, direction, heats[direction]
    self.hp = HParams(**over)
    self.cfg = oracle_cfg_from_hp(self.hp)
    self.sd = hot_state_dict(name, direction)
    self.sdn = synthetic.to_weightnorm_form(self.sd)
    self.inputs = make_inputs(name, direction)
    self.mel = self.inputs[0]
    if direction == "fwd":
      self.wav = self.inputs[1]
    else:
      self.z_init, self.z_early, self.sigma = self.inputs[1], self.inputs[2], SIGMA
    self.fx = fixture(name)

  def get(self, key):
    return self.fx[f"{self.direction}/{key}"]

  def oracle_cfg(self):
    return self.cfg

  def yard(self, group):
    """{quantity: relative yardstick} of a group: "train" (weight-norm form, one step), "infer" (dense weights, values),
    "synth" (weight-norm form, values and gradients through synthesis)."""
    names = self.get(f"yard/{group}/names")
    vals = self.get(f"yard/{group}/rel")
    return {str(n): float(v) for n, v in zip(names, vals)}


# ---------------------------------------------------------------- what the HIP path is held to
def logdet_bound(ref):
  """log_det_W is not touched by any fp16 rounding (yardstick 0): fp32 LU of an 8x8 matrix, the bound of test_gpu_train."""
  return 1e-3 * max(1.0, abs(ref))


def check(got, ref, yard, what, factor=BOUND_FACTOR, quiet=False, finite=True):
  """Every quantity of ``ref`` (fp64 oracle on the inputs the kernel received) against ``got``:
  ||got - ref|| <= factor * yardstick * ||ref|| + FLOOR, and finite.  Prints error, yardstick and ratio for each; returns
  the list of (ratio, quantity) that miss, worst first, so that a caller can assert on all of them at once.  With
  ``finite=False`` (the planted faults of test_hot_cpu.py) a non-finite entry is a miss instead of an assertion."""
  rows = []
  for q, t in ref.items():
    g = got[q]
    assert g is not None, f"{what}: {q}: missing"
    g = g.detach().double().cpu()
    assert g.shape == t.shape, f"{what}: {q}: shape {tuple(g.shape)} vs {tuple(t.shape)}"
    assert not finite or torch.isfinite(g).all(), f"{what}: {q}: not finite"
    g = torch.nan_to_num(g, nan=float("inf"))
    if q == "log_det":
      for a, b in zip(g.tolist(), t.tolist()):
        assert abs(a - b) <= logdet_bound(b), f"{what}: log_det {a} vs {b}"
      continue
    err, den = float((g - t.double()).norm()), float(t.double().norm())
    bound = factor * yard[q] * den + FLOOR
    rows.append((err / bound, q, err / max(den, 1e-30), yard[q], err <= bound))
  rows.sort(reverse=True)
  if not quiet:
    for ratio, q, rel, y, ok in rows[:10]:
      print(f"{what}: {q}: rel {rel:.3e} yardstick {y:.3e} ratio {rel / max(y, 1e-30):.2f}{'' if ok else '  <-- MISS'}")
  return [(rel / max(y, 1e-30), q) for ratio, q, rel, y, ok in rows if not ok]


# ---------------------------------------------------------------- the regime
def regime(name, direction, sd):
  """Statistics of the fp64 oracle on the case's own batch: the conditions on the INPUTS of the hot tests."""
  over = CASES[name][0]
  cfg = oracle_cfg_from_hp(HParams(**over))
  inputs = make_inputs(name, direction)
  trace = {}
  w = {k: v.double() for k, v in sd.items()}
  with torch.no_grad():
    if direction == "fwd":
      forward(w, inputs[0].double(), inputs[1].double(), cfg, Prec(trace=trace))
    else:
      infer(w, inputs[0].double(), inputs[1].double(), {k: v.double() for k, v in inputs[2].items()}, SIGMA, cfg,
            Prec(trace=trace))
  a, b = torch.cat([t.flatten() for t in trace["a"]]), torch.cat([t.flatten() for t in trace["b"]])
  Ws = [w[f"convinv.{k}.conv.weight"].squeeze(-1) for k in range(cfg.n_flows)]
  return {"a_max": float(a.abs().max()), "b_absmax": float(b.abs().max()), "b_min": float(b.min()),
          "a_gt4": float((a.abs() > 4).double().mean()),
          "log_s_std": [float(trace["log_s"][k].std()) for k in range(cfg.n_flows)],
          "log_s_max": max(float(t.abs().max()) for t in trace["log_s"].values()),
          "cond": [float(torch.linalg.cond(W)) for W in Ws], "logdet": [float(torch.logdet(W)) for W in Ws]}


def assert_regime(st, direction, what):
  """The conditions every hot case meets (the b < -88.7 one is over all inference cases: test_hot_cpu.py)."""
  assert st["a_max"] > 20.8, (what, st["a_max"])                       # beyond the +-60 clamp of the tanh exponent
  if direction == "fwd":
    assert st["b_absmax"] > 41.6, (what, st["b_absmax"])               # beyond the training clamp of the sigmoid exponent
  assert 0.10 <= st["a_gt4"] <= 0.60, (what, st["a_gt4"])
  assert min(st["log_s_std"]) >= 0.7, (what, st["log_s_std"])
  assert st["log_s_max"] >= 3.0, (what, st["log_s_max"])
  assert min(st["cond"]) >= 5.0, (what, st["cond"])
  assert min(abs(v) for v in st["logdet"]) >= 0.1, (what, st["logdet"])


def oracle_agreement(name, direction, sd):
  """Worst relative L2 between the fp32 and the fp64 oracle over every value and gradient of the case."""
  over = CASES[name][0]
  cfg = oracle_cfg_from_hp(HParams(**over))
  inputs = make_inputs(name, direction)
  sdn = synthetic.to_weightnorm_form(sd)
  r = None if direction == "fwd" else cotangent(name)
  e = errors(exact(direction, sdn, inputs, cfg, r=r, dtype=torch.float32), exact(direction, sdn, inputs, cfg, r=r))
  return max((err / max(den, 1e-30), q) for q, (err, den) in e.items()
             if not (q.startswith("p/") and K.structurally_zero(HParams(**over), q[2:])))
