"""CPU: the reparametrised checkpoints of tests/_offmanifold.py (g != ||v|| in every row, dense weights unchanged) against
the oracle alone -- that the family leaves everything but the (g, v) gradients alone, and that it sees what the on-manifold
family (g = ||v||, row scale s = 1) cannot: faults in how the weight-norm row scale is indexed and applied.

(a), (b): invariance in both directions.  (c): each fault is planted into a torch restatement of what the library does with
the row scale -- ``_packing.pack_weights`` (the packing wg_train_prepare is held to) with its weight-norm
evaluation replaced by ``v * s[index]`` and the backward formulas of csrc/train_prep.hip: wn_grad_kernel -- and must change
nothing on the manifold and more than 10 x GRAD_TOL off it.
"""
import pytest
import torch

import _packing as T
from _cases import GRAD_TOL, Case, oracle_cfg_from_hp, rms
from _offmanifold import (FLOOR, V0, V1, check, floor_only_names, oracle_infer_grads, raw_worst, reparametrise,
                          to_on_metric)
from oracle import torch_oracle as O
from waveglow_amd import synthetic
from waveglow_amd.hparams import HParams
from waveglow_amd.model import WaveGlow

INVARIANT_TOL = 1e-5      # the relations between the two parametrisations, relative L2 per tensor (measured 4e-7)
OVER = dict(n_channels=64, n_layers=3, n_flows=4, n_early_every=1, n_early_size=2)      # h_k = 4, 3, 2, 1


def _inputs(B=2, Tn=6):
  hp = HParams(**OVER)
  sd_on = synthetic.to_weightnorm_form(synthetic.make_state_dict(hp, seed=3))
  mel = synthetic.make_mel(B, Tn, seed=5)
  wav = torch.rand(B, 256 * Tn - 32, generator=torch.Generator().manual_seed(6)) * 0.6 - 0.3
  return hp, sd_on, mel, wav


@pytest.fixture(scope="module")
def training_pair():
  """(hp, mel, wav, sd_on, sd_off, U, (loss, grads) of oracle.grads_ref on the manifold, the same off it)."""
  hp, sd_on, mel, wav = _inputs()
  sd_off, U = reparametrise(sd_on, seed=1)
  cfg = oracle_cfg_from_hp(hp)
  return hp, mel, wav, sd_on, sd_off, U, O.grads_ref(sd_on, mel, wav, cfg, 1.0), O.grads_ref(sd_off, mel, wav, cfg, 1.0)


def test_reparametrise_covers_every_module_and_keeps_the_dense_weights():
  hp, sd_on, _, _ = _inputs()
  sd_off, U = reparametrise(sd_on, seed=1)
  assert set(sd_off) == set(sd_on)
  n_mod = hp.n_flows * (2 + 2 * hp.n_layers)
  assert len(U) == n_mod
  dense = synthetic.make_state_dict(hp, seed=3)
  for p, u in U.items():
    assert bool((u < 0).any()) and bool((u.abs() < 0.5).any()) and bool((u.abs() > 2).any()), p
    assert 0.25 * (1 - 1e-6) <= float(u.abs().min()) and float(u.abs().max()) <= 4 * (1 + 1e-6), p
    v, g = sd_off[p + V1], sd_off[p + V0]
    s = g.flatten() / v.flatten(1).norm(dim=1)
    assert float(((s - u) / u).abs().max()) <= 1e-6, p          # the library's row scale is u now
    w = torch._weight_norm(v, g, 0)
    assert float((w - dense[p + "weight"]).abs().max()) <= 4e-7 * float(dense[p + "weight"].abs().max()), p
  # the same seed gives the same draw; another seed another one
  again, _ = reparametrise(sd_on, seed=1)
  assert all(torch.equal(again[k], sd_off[k]) for k in sd_off)
  other, _ = reparametrise(sd_on, seed=2)
  assert not torch.equal(other["WN.0.start." + V1], sd_off["WN.0.start." + V1])
  # to_on_metric leaves everything that is not a (g, v) pair alone
  fake = {k: torch.ones_like(t) for k, t in sd_off.items()}
  back = to_on_metric(fake, U)
  assert all(back[k] is fake[k] for k in fake if not (k.endswith(V0) or k.endswith(V1)))
  assert torch.equal(back["WN.1.cond_layer." + V1].flatten(1)[:, 0], 1.0 / U["WN.1.cond_layer."])


def test_training_direction_is_invariant(training_pair):
  hp, mel, wav, sd_on, sd_off, U, (loss_on, g_on), (loss_off, g_off) = training_pair
  print(f"loss on {float(loss_on):.8f} off {float(loss_off):.8f}")
  assert abs(float(loss_on) - float(loss_off)) <= 1e-6 * max(1.0, abs(float(loss_on)))
  floor = floor_only_names(sd_on)
  assert floor == ("WN.3.start." + V1,)
  worst = check(to_on_metric(g_off, U), g_on, "training", floor_only=floor, tol=INVARIANT_TOL)
  raw, name = raw_worst(g_off, g_on, skip=floor)
  print(f"training: worst relation error {worst:.3e}; untransformed {raw:.3e} ({name})")
  assert raw > 0.5       # the (g, v) gradients themselves are far from the on-manifold ones: d v has ratio u per row
  # the ratio itself, on one module
  p = "WN.0.in_layers.1."
  ratio = (g_off[p + V1] * g_on[p + V1]).flatten(1).sum(1) / g_on[p + V1].flatten(1).pow(2).sum(1)
  assert float(((ratio - U[p]) / U[p]).abs().max()) <= INVARIANT_TOL


def test_synthesis_direction_is_invariant():
  c = Case("c64")
  sd_on = synthetic.to_weightnorm_form(c.sd)
  sd_off, U = reparametrise(sd_on, seed=1)
  r = torch.randn(c.audio.shape, generator=torch.Generator().manual_seed(11)) / c.audio.numel()
  a_on, p_on, mel_on, zi_on, ze_on = oracle_infer_grads(sd_on, c, r)
  a_off, p_off, mel_off, zi_off, ze_off = oracle_infer_grads(sd_off, c, r)
  d = rms(a_off - a_on)
  print(f"synthesis: audio rms difference {d:.3e} (audio rms {rms(a_on):.3e})")
  assert d <= 1e-6 * max(1.0, rms(a_on))
  assert rms(a_off - torch.from_numpy(c.npz["audio_from_weightnorm_ckpt"])) <= 2e-6
  worst = check(to_on_metric(p_off, U), p_on, "synthesis", floor_only=floor_only_names(sd_on), tol=INVARIANT_TOL)
  raw, name = raw_worst(p_off, p_on)
  print(f"synthesis: worst relation error {worst:.3e}; untransformed {raw:.3e} ({name})")
  assert raw > 0.5
  for what, a, b in [("d mel", mel_off, mel_on), ("d z_init", zi_off, zi_on)] + \
                    [(f"d z_early[{i}]", x, y) for i, (x, y) in enumerate(zip(ze_off, ze_on))]:
    assert float((a - b).norm()) <= INVARIANT_TOL * float(b.norm()), what


# ---------------------------------------------------------------- (c) planted faults
FAULTS = ("dv_without_s", "coef_without_s", "s_of_row_minus_1", "cond_s_of_layer_0", "skip_s_of_res_rows")


class _RowScale(torch.autograd.Function):
  """w[r] = v[r] * s[index[r]], s = g / ||v|| (rownorm_kernel, pack_kernel); backward as wn_grad_kernel writes it:
  d v = s dW - s (dW . v) v / ||v||^2, d g = (dW . v) / ||v||.  ``fault`` drops one of the two ``s`` of d v."""

  @staticmethod
  def forward(ctx, v, g, index, fault):
    n = v.flatten(1).norm(dim=1)
    s, inv = g.flatten() / n, 1.0 / n
    ctx.save_for_backward(v, s, inv)
    ctx.fault = fault
    return v * s[index].view(-1, 1, 1)

  @staticmethod
  def backward(ctx, dW):
    v, s, inv = ctx.saved_tensors
    dot = (dW * v).flatten(1).sum(1)
    one = torch.ones_like(s)
    s_dw = one if ctx.fault == "dv_without_s" else s
    s_coef = one if ctx.fault == "coef_without_s" else s
    dv = s_dw.view(-1, 1, 1) * dW - (s_coef * dot * inv * inv).view(-1, 1, 1) * v
    return dv, (dot * inv).view(-1, 1, 1), None, None


def _restated_step(hp, sd, mel, wav, fault, monkeypatch):
  """One training step through pack_weights and a plain-torch evaluation of the packed matrices (natural channel order),
  the weight norm evaluated by _RowScale: (loss, {parameter name: gradient})."""
  model = WaveGlow(hp)
  model.load_state_dict(sd)
  Cc, nl, nf = hp.n_channels, hp.n_layers, hp.n_flows
  kind = {}
  for k in range(nf):
    kind[id(model.WN[k].start)] = "start"
    kind[id(model.WN[k].cond_layer)] = "cond"
    for i in range(nl):
      kind[id(model.WN[k].in_layers[i])] = "in"
      kind[id(model.WN[k].res_skip_layers[i])] = "res_skip"

  def compose(m):
    pw = m.parametrizations.weight
    n = pw.original1.shape[0]
    index = torch.arange(n)
    if fault == "s_of_row_minus_1":
      index = (index - 1) % n
    elif fault == "cond_s_of_layer_0" and kind[id(m)] == "cond":
      index = index % (2 * Cc)
    elif fault == "skip_s_of_res_rows" and kind[id(m)] == "res_skip" and n == 2 * Cc:
      index = torch.cat([index[:Cc], index[:Cc]])              # the fold reads s[j] where it should read s[C + j]
    return _RowScale.apply(pw.original1, pw.original0, index, fault)

  monkeypatch.setattr(T, "_dense_stack", lambda mods: torch.stack([compose(m) for m in mods]))
  w1, b1, w2, b2, wes, wup, bup, start5, out_init, w1x1 = T.pack_weights(model)
  pad = torch.nn.functional.pad
  B, M, Tn = mel.shape
  S = wav.shape[1] - wav.shape[1] % 8
  L, M8 = S // 8, 8 * M
  Q = (L + 31) // 32
  melp = pad(mel, (3, 0))
  taps = torch.stack([pad(melp[:, :, 3 - j:3 - j + Q].transpose(1, 2), (0, 128 - M)) for j in range(4)], 2).reshape(B, Q, 512)
  spect = torch.einsum("pmk,bqk->mbqp", wup, taps).reshape(M8, B, Q * 32)[:, :, :L] + bup[:, None, None]
  audio = wav[:, :S].view(B, L, 8).permute(0, 2, 1)
  outs, log_s, log_det = [], [], []
  for k in range(nf):
    if k % hp.n_early_every == 0 and k > 0:
      outs.append(audio[:, :hp.n_early_size])
      audio = audio[:, hp.n_early_size:]
    c = audio.shape[1]
    h = c // 2
    log_det.append(B * L * torch.logdet(model.convinv[k].conv.weight.squeeze(2)))
    audio = torch.einsum("rc,bcl->brl", w1x1[k, :c, :c], audio)
    a0, a1 = audio[:, :h], audio[:, h:]
    x = torch.einsum("pj,bjl->pbl", start5[k, :h].t(), a0) + start5[k, 4][:, None, None]
    out = out_init[k][:, None, None].expand(8, B, L)
    for i in range(nl):
      fl, d = k * nl + i, 2 ** i
      xp = pad(x, (d, d))
      kin = torch.cat([xp[:, :, 0:L], xp[:, :, d:d + L], xp[:, :, 2 * d:2 * d + L], spect], 0)
      pre = torch.einsum("mk,kbl->mbl", w1[fl], kin) + b1[fl][:, None, None]
      acts = torch.tanh(pre[:Cc]) * torch.sigmoid(pre[Cc:])
      if i < nl - 1:
        x = x + torch.einsum("mk,kbl->mbl", w2[fl], acts) + b2[fl][:, None, None]
      out = out + torch.einsum("mk,kbl->mbl", wes[fl], acts)
    b_, ls = out[:h].permute(1, 0, 2), out[h:2 * h].permute(1, 0, 2)
    audio = torch.cat([a0, torch.exp(ls) * a1 + b_], 1)
    log_s.append(ls)
  outs.append(audio)
  loss = O.loss_ref(torch.cat(outs, 1), log_s, log_det, 1.0)
  names, params = zip(*model.named_parameters())
  return loss.detach(), dict(zip(names, torch.autograd.grad(loss, params)))


def _worst(grads, ref, skip):
  return max((float((grads[n] - r).norm()) / max(float(r.norm()), 1e-12), n) for n, r in ref.items() if n not in skip)


def test_restatement_without_a_fault_is_the_oracle(training_pair, monkeypatch):
  """The restatement that the faults are planted into computes what oracle.grads_ref computes, on and off the manifold."""
  hp, mel, wav, sd_on, sd_off, U, (loss_on, g_on), (loss_off, g_off) = training_pair
  floor = floor_only_names(sd_on)
  for what, sd, loss_ref, g_ref in (("on", sd_on, loss_on, g_on), ("off", sd_off, loss_off, g_off)):
    loss, g = _restated_step(hp, sd, mel, wav, None, monkeypatch)
    assert set(g) == set(g_ref)
    assert abs(float(loss) - float(loss_ref)) <= 1e-6 * max(1.0, abs(float(loss_ref)))
    u = U if what == "off" else {}
    worst = check(to_on_metric(g, u), to_on_metric(g_ref, u), f"restatement {what}", floor_only=floor, tol=INVARIANT_TOL)
    print(f"restatement {what} the manifold: worst {worst:.3e}")


@pytest.mark.parametrize("fault", FAULTS)
def test_planted_fault_is_invisible_on_the_manifold_and_caught_off_it(fault, training_pair, monkeypatch):
  hp, mel, wav, sd_on, sd_off, U, (loss_on, g_on), (loss_off, g_off) = training_pair
  floor = floor_only_names(sd_on)
  # on the manifold: s = 1 in every row, the fault changes nothing
  _, clean = _restated_step(hp, sd_on, mel, wav, None, monkeypatch)
  loss_f, faulty = _restated_step(hp, sd_on, mel, wav, fault, monkeypatch)
  on, on_name = _worst(faulty, clean, floor)
  assert float((faulty[floor[0]] - clean[floor[0]]).norm()) <= FLOOR
  assert abs(float(loss_f) - float(loss_on)) <= 1e-6 * max(1.0, abs(float(loss_on)))
  # off it: the oracle's gradients in the on-manifold metric are the yardstick, as on the GPU
  loss_f, faulty = _restated_step(hp, sd_off, mel, wav, fault, monkeypatch)
  ref = to_on_metric(g_off, U)
  got = to_on_metric(faulty, U)
  off, off_name = _worst(got, ref, floor)
  n_bad = sum(1 for n, r in ref.items() if n not in floor and float((got[n] - r).norm()) > GRAD_TOL * float(r.norm()) + FLOOR)
  print(f"fault {fault}: on the manifold {on:.3e} ({on_name}); off it {off:.3e} ({off_name}), {n_bad} of {len(ref)} tensors "
        f"beyond GRAD_TOL, loss off by {abs(float(loss_f) - float(loss_off)):.3e}")
  assert on <= 1e-6
  assert off > 10 * GRAD_TOL
