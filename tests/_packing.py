"""The library's weight packing (``wg_train_prepare``) written as torch ops, the checker the tests hold it to: natural-order
stacked matrices (``pack_weights``), the kernels' channel-position permutation and the MFMA fragment orders.  Test code only."""
from typing import Tuple

import torch


def pos_perm(n: int) -> torch.Tensor:
  """perm[P] = channel stored at position P (wg_common.h: pos_to_chan) for n channels (n % 32 == 0)."""
  P = torch.arange(n)
  blk, p = P // 32, P % 32
  h, g, i = p // 16, (p // 4) % 4, p % 4
  return blk * 32 + 8 * g + 4 * h + i


_PERM_CACHE: dict = {}


def _perms(Cc: int, M8: int, device) -> "_Perms":
  """Index tensors are built (and copied to the device) once per geometry, not once per step."""
  key = (Cc, M8, str(device))
  if key not in _PERM_CACHE:
    _PERM_CACHE[key] = _Perms(Cc, M8, device)
  return _PERM_CACHE[key]


class _Perms:
  def __init__(self, Cc: int, M8: int, device):
    pc = pos_perm(Cc)
    self.c = pc.to(device)
    self.c2 = torch.cat([pc, Cc + pc]).to(device)
    self.m8 = pos_perm(M8).to(device)
    self.k1 = torch.cat([pc, Cc + pc, 2 * Cc + pc, 3 * Cc + pos_perm(M8)]).to(device)
    self.r32 = pos_perm(32).to(device)
    for name in ("c", "c2", "m8", "k1"):
      setattr(self, "i" + name, torch.argsort(getattr(self, name)))       # inverse permutations (gradients)
    r = torch.arange(32)
    self.c2p = (16 * ((r >> 2) & 1) + 4 * (r >> 3) + (r & 3)).to(device)   # chan_to_pos inside a 32-block


# (tensor index in the packed tuple, dims that carry a channel-position permutation, which permutation)
_PERM_PLAN = ((0, ((1, "c2"), (2, "k1"))), (1, ((1, "c2"),)), (2, ((1, "c"), (2, "c"))), (3, ((1, "c"),)), (4, ((2, "c"),)),
              (5, ((1, "m8"),)), (6, ((0, "m8"),)), (7, ((2, "c"),)))


def to_pos_order(packed, pm: "_Perms", inverse: bool = False):
  """Natural channel order -> the kernels' position-major order (or back, for gradients).  Plain gathers, done
  outside autograd (inside the autograd node): an indexing op under autograd costs a zero-filled full-size tensor and
  an atomic scatter in its backward; the inverse permutation is just another gather."""
  out = list(packed)
  for idx, dims in _PERM_PLAN:
    t = out[idx]
    for dim, name in dims:
      t = t.index_select(dim, getattr(pm, ("i" if inverse else "") + name))
    out[idx] = t
  return out


def _dense_stack(mods) -> torch.Tensor:
  """Dense weights of same-shaped conv modules, stacked [n, out, in, k].  Weight-normed modules (the training case) are
  evaluated with ONE ``torch._weight_norm`` over their concatenated (g, v) -- what the parametrization computes per
  module (rows are normalised independently), in one kernel each way instead of one per module."""
  is_p = torch.nn.utils.parametrize.is_parametrized
  if len(mods) > 1 and all(is_p(m, "weight") for m in mods):
    g = torch.cat([m.parametrizations.weight.original0 for m in mods])
    v = torch.cat([m.parametrizations.weight.original1 for m in mods])
    return torch._weight_norm(v, g, 0).view(len(mods), v.shape[0] // len(mods), *v.shape[1:])
  return torch.stack([m.weight for m in mods])


def _shape_runs(sizes):
  """[(size, [flow indices])] for maximal runs of consecutive flows with equal size (flow order is kept by concatenating
  the runs)."""
  runs = []
  for k, r in enumerate(sizes):
    if runs and runs[-1][0] == r:
      runs[-1][1].append(k)
    else:
      runs.append((r, [k]))
  return runs


def pack_weights(model) -> Tuple[torch.Tensor, ...]:
  """Differentiable packing of the module's parameters into the stacked matrices of wg_train_weights, in NATURAL
  channel order (to_pos_order applies the kernels' permutation).

  Few, LARGE autograd nodes: modules of one shape are gathered across ALL flows and go through one weight-norm
  evaluation (``_dense_stack``), and everything per flow (W_end x W_skip fold, start, 1x1) is a batched op over the
  flow axis -- a per-module formulation costs ~2000 tiny kernels per step (~8 ms of the round-1 step), and every
  per-layer slice of a big tensor costs a zero-filled full-size gradient in its backward."""
  hp = model._hp
  Cc, nl, nf, M, M8 = hp.n_channels, hp.n_layers, model.n_flows, hp.n_mel_channels, hp.n_mel_channels * 8
  pad = torch.nn.functional.pad
  WN = model.WN
  w_in = _dense_stack([WN[k].in_layers[i] for k in range(nf) for i in range(nl)])              # [FL, 2C, C, 3]
  b_in = torch.stack([WN[k].in_layers[i].bias for k in range(nf) for i in range(nl)])          # [FL, 2C]
  w_cond = _dense_stack([WN[k].cond_layer for k in range(nf)]).squeeze(3).reshape(nf * nl, 2 * Cc, M8)
  b_cond = torch.stack([WN[k].cond_layer.bias for k in range(nf)]).reshape(nf * nl, 2 * Cc)
  last_w = _dense_stack([WN[k].res_skip_layers[nl - 1] for k in range(nf)]).squeeze(3)         # [nf, C, C]: all skip rows
  last_b = torch.stack([WN[k].res_skip_layers[nl - 1].bias for k in range(nf)])                # [nf, C]
  if nl > 1:
    rs_w = _dense_stack([WN[k].res_skip_layers[i] for k in range(nf) for i in range(nl - 1)]).squeeze(3)
    rs_w = rs_w.view(nf, nl - 1, 2 * Cc, Cc)
    rs_b = torch.stack([WN[k].res_skip_layers[i].bias for k in range(nf) for i in range(nl - 1)]).view(nf, nl - 1, 2 * Cc)
    w2 = pad(rs_w[:, :, :Cc], (0, 0, 0, 0, 0, 1)).reshape(nf * nl, Cc, Cc)      # model.py:131-134; the last layer has no res rows
    b2 = pad(rs_b[:, :, :Cc], (0, 0, 0, 1)).reshape(nf * nl, Cc)
    w_skips = torch.cat([rs_w[:, :, Cc:], last_w[:, None]], 1)                  # [nf, nl, C, C]   model.py:135-136
    b_skip_sum = rs_b[:, :, Cc:].sum(1) + last_b                                # [nf, C]
  else:
    w2 = torch.zeros_like(last_w)
    b2 = torch.zeros_like(last_b)
    w_skips, b_skip_sum = last_w[:, None], last_b
  # Per-flow small tensors (end, start, 1x1): flows of one shape (h_k changes at the early outputs) are stacked and padded as
  # ONE tensor per shape group -- a per-flow formulation costs ~25 tiny kernels per flow and step each way.
  runs = _shape_runs([WN[k].end.weight.shape[0] for k in range(nf)])
  # WN.end (not weight-normed, 2h_k rows) zero-padded to 8 rows: end(sum_i skip_i) for every flow in one batched GEMM
  w_end8 = torch.cat([pad(torch.stack([WN[k].end.weight.squeeze(2) for k in ks]), (0, 0, 0, 8 - r)) for r, ks in runs])
  b_end8 = torch.cat([pad(torch.stack([WN[k].end.bias for k in ks]), (0, 8 - r)) for r, ks in runs])
  wes = torch.matmul(w_end8[:, None], w_skips).reshape(nf * nl, 8, Cc)           # [nf, nl, 8, C]
  out_init = torch.bmm(w_end8, b_skip_sum[:, :, None]).squeeze(2) + b_end8       # [nf, 8]
  # start conv [C, h_k] (weight norm per shape group), zero-padded to 4 columns, + bias row -> [nf, 5, C]
  start5 = torch.cat([torch.cat([pad(_dense_stack([WN[k].start for k in ks]).squeeze(3), (0, 4 - r // 2)).transpose(1, 2),
                                 torch.stack([WN[k].start.bias for k in ks])[:, None, :]], 1) for r, ks in runs])
  w1x1 = torch.cat([pad(torch.stack([model.convinv[k].conv.weight.squeeze(2) for k in ks]), (0, 8 - r, 0, 8 - r))
                    for r, ks in _shape_runs([model.convinv[k].conv.weight.shape[0] for k in range(nf)])])
  FL = nf * nl
  w_in = w_in.permute(0, 1, 3, 2).reshape(FL, 2 * Cc, 3 * Cc)                    # K = tap-major
  w1 = torch.cat([w_in, w_cond], 2)                                              # [FL, 2C, 3C + M8]
  # "* 1.0": AddBackward hands the SAME gradient tensor to both operands and cat / stack backward only slice it, so
  # in_layers[i].bias.grad and cond_layer.bias.grad would become overlapping views of one buffer (AccumulateGrad
  # installs them without a copy) and the next in-place accumulation would count a gradient twice
  b1 = b_in + b_cond * 1.0
  up = model.upsample.weight                                                     # [M_in, M_out, 1024]
  wup = up.view(M, M, 4, 32, 8).permute(3, 1, 4, 2, 0).reshape(32, M8, 4, M)     # [p][(o,g)][j][i]
  wup = torch.nn.functional.pad(wup, (0, 128 - M)).reshape(32, M8, 512)
  bup = model.upsample.bias.repeat_interleave(8)
  return (w1.contiguous(), b1.contiguous(), w2.contiguous(), b2.contiguous(), wes.contiguous(), wup.contiguous(),
          bup.contiguous(), start5.contiguous(), out_init.contiguous(), w1x1.contiguous())


def to_fragments(mat: torch.Tensor, c2p: torch.Tensor = None) -> torch.Tensor:
  """[..., M, K] (pos,pos) fp16 -> MFMA-fragment order [..., K/64, M/32, 4, 64, 8] (wg_train.h: PGemmArgs::A):
  lane (r, h), element j of sub-step s of block b, K-step t = mat[32b + chan_to_pos(r)][64t + 32h + 8s + j]."""
  *lead, M, K = mat.shape
  if c2p is None:
    r = torch.arange(32)
    c2p = (16 * ((r >> 2) & 1) + 4 * (r >> 3) + (r & 3)).to(mat.device)
  v = mat.reshape(*lead, M // 32, 32, K // 64, 2, 4, 8).index_select(len(lead) + 1, c2p)   # [.., b, r, t, h, s, j]
  n = len(lead)
  return v.permute(*range(n), n + 2, n, n + 4, n + 3, n + 1, n + 5).contiguous()            # [.., t, b, s, h, r, j]


K_TANH_SCALE = 2.8853900817779268     # 2*log2(e): the gate evaluates tanh / sigmoid through exp2 (kernels.hip: gate_act)
K_SIGM_SCALE = -1.4426950408889634    # -log2(e)


def wn_forward_fragments(w1: torch.Tensor, b1: torch.Tensor, w2: torch.Tensor, wes: torch.Tensor, pm: "_Perms", NW: int):
  """Natural-order stacked matrices -> the forward kernel's operands (include/waveglow_amd.h: wg_train_weights a1, a1c,
  b1, a2, es): rows stay in natural channel order, K goes to position order, the gate pre-scale is folded into the
  GEMM-1 rows and bias, and everything is laid out in the WN-layer kernel's MFMA A-fragment order.
  w1 [FL, 2C, 3C + M8], b1 [FL, 2C], w2 [FL, C, C], wes [FL, 8, C] (fp32)."""
  FL, C2, K1 = w1.shape
  Cc = C2 // 2
  MB = Cc // (32 * NW)
  nK = K1 // 64
  scale = torch.cat([torch.full((Cc,), K_TANH_SCALE), torch.full((Cc,), K_SIGM_SCALE)]).to(w1)
  wk = (w1.index_select(2, pm.k1) * scale[None, :, None]).half()                   # K in position order, rows natural
  # rows (gate, w, mb, r), K (ks, u1, k2, hh, j)  ->  [ks, u1, w, (gate, mb) = mt, k2, (hh, r) = lane, j]
  a = wk.reshape(FL, 2, NW, MB, 32, nK, 2, 2, 2, 8).permute(0, 5, 6, 2, 1, 3, 7, 8, 4, 9).contiguous()
  a = a.reshape(FL, nK, 2 * NW * 2 * MB * 2 * 64 * 8)
  n_tap = 3 * Cc // 64
  a1 = a[:, :n_tap].contiguous()
  a1c = a[:, n_tap:].contiguous()
  b1s = (b1 * scale[None, :]).float().contiguous()
  w2k = w2.index_select(2, pm.c).half()                                            # [FL, C rows natural, C pos]
  a2 = w2k.reshape(FL, NW, MB, 32, Cc // 16, 2, 8).permute(0, 1, 2, 4, 5, 3, 6).contiguous()   # [FL, w, mb, k16, hh, r, j]
  wek = wes.index_select(2, pm.c)
  hi = wek.half()
  lo = (wek - hi.float()).half()
  rows16 = torch.cat([hi, lo], 1)                                                  # [FL, 16, C pos]
  es = rows16.reshape(FL, 16, Cc // 32, 4, 8).permute(0, 2, 3, 1, 4).contiguous()  # [FL, s, l4, row, j]: lane = 16 l4 + row
  return a1, a1c, b1s, a2, es


def plain_fragments(mat: torch.Tensor, NW: int) -> torch.Tensor:
  """[FL, M, K] fp16 (rows natural, K already in the order of the planes it multiplies) -> the WN-layer kernel's A-fragment
  order for plain row blocks [FL, K/64, 2, NW, MB, 2, 64, 8] (include/waveglow_amd.h: wat, wbt)."""
  FL, M, K = mat.shape
  MB = M // (32 * NW)
  v = mat.reshape(FL, NW, MB, 32, K // 64, 2, 2, 2, 8)                      # rows (w, mb, r), K (ks, u1, k2, hh, j)
  return v.permute(0, 4, 5, 1, 2, 6, 7, 3, 8).contiguous()                  # [FL, ks, u1, w, mb, k2, hh, r, j]
