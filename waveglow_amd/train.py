"""Training direction: ``WaveGlow.forward`` under autograd on the HIP library.

Reference: src/waveglow/model.py:178-221 (forward), train.py:190-199 (``loss.backward()``; Adam step on the
weight-normed parameters).  Everything that touches a weight, an activation or a gradient runs in the library:

* ``wg_train_prepare``: the module's own parameter tensors (weight-normed (g, v) pairs or dense weights, native layouts)
  -> every operand of the step: weight norm, the ``WN.end`` x skip fold, channel permutations, gate pre-scale, MFMA
  fragment orders (csrc/train_prep.hip, pack_kernel);
* ``wg_train_forward`` / ``wg_train_backward``: upsample, 12 x (1x1 conv, start, 8 x (dilated conv + cond + gate, res,
  skip/end), coupling) with saved fp16 activations, and the whole backward (both dgrads of every layer, every weight
  gradient, coupling / 1x1 / start backward) -- one C call each way;
* ``wg_train_param_grads``: packed gradients -> one gradient per parameter (weight-norm backward, the fold's chain rule) in
  ONE flat buffer; autograd gets views of it.

This file is the binding and nothing else: the autograd node (``_TrainFn``), buffer allocation, the data-parallel
schedule, and what ``_TrainFn`` shares with the synthesis direction's node (waveglow_amd/infer_grad.py) -- the lifecycle
of a node between its forward and its backward (``begin_node`` / ``finish_node``: per-call weights, one pool workspace
behind a guard, the loss scale, the refusals, packed gradients -> parameter gradients) and its parts
(``request_workspace``, ``new_grad``, ``set_grad_finite``, ``param_grad_views``).  What is left to torch is ``logdet`` of
the twelve 1x1 weights (model.py:63) and the optimiser.

There is no fallback: CPU tensors raise.
"""
from __future__ import annotations

import ctypes as C
import math
import os
from typing import List, Tuple

import torch

from . import _lib
from ._args import ptr as _ptr


def canonical_params(model, eng):
  """(names, tensors in the library's canonical order, weight_normed flag) for wg_train_prepare / wg_train_param_grads: the
  module's own parameter tensors, looked up by state_dict key (include/waveglow_amd.h: wg_train_param_name), each held to
  the element count the library will read and write through its bare pointer (wg_train_param_numel) before anything else."""
  wn = torch.nn.utils.parametrize.is_parametrized(model.WN[0].start, "weight")
  key = ("train_params", wn)
  if key not in eng.cache:
    n = eng.lib.wg_train_param_count(eng.handle, int(wn))
    eng.cache[key] = ([eng.lib.wg_train_param_name(eng.handle, int(wn), i).decode() for i in range(n)],
                      [int(eng.lib.wg_train_param_numel(eng.handle, int(wn), i)) for i in range(n)])
  names, numels = eng.cache[key]
  byname = dict(model.named_parameters())
  try:
    tensors = [byname[n] for n in names]
  except KeyError as e:
    raise _lib.WgError(f"parameter {e} missing: the training direction needs every WN module in the same form "
                       "(all weight-normed, or all dense after remove_weightnorm)")
  for n, t, numel in zip(names, tensors, numels):
    if t.numel() != numel:
      raise _lib.WgError(f"parameter {n}: {t.numel()} elements of shape {tuple(t.shape)}, the library reads and writes "
                         f"{numel} for this model")
  for n, t in zip(names, tensors):
    if t.dtype != torch.float32 or not t.is_contiguous() or t.device.type != "cuda":
      raise _lib.WgError(f"parameter {n}: the training direction takes contiguous float32 parameters on the GPU")
  return names, tensors, wn


class _Weights:
  """Device buffers + the ctypes struct handed to the library (kept alive between forward and backward).  Everything in
  them -- fp16 fragment tensors and the small fp32 vectors -- is filled by the library itself from the module's own
  parameter tensors (``wg_train_prepare``: weight norm, the W_end x W_skip fold, permutations, gate pre-scale, fragment
  orders); tests/_packing.py is the same computation written as torch ops, and the tests hold the library to it.
  ``tensors`` (the detached parameters) stay here, so their storage lives as long as the node that holds this object, and
  ``sig`` is their ``(_version, data_ptr())`` when the library read them: ``moved`` tells whether that still holds."""

  def __init__(self, model, tensors, wn: bool, flow_c: List[int], eng, stream, want_wupt: bool = False,
               want_winv: bool = False):
    hp = model._hp
    Cc, nf, nl = hp.n_channels, model.n_flows, hp.n_layers
    M8 = hp.n_mel_channels * 8
    dev = tensors[0].device
    FL = nf * nl
    K1 = 3 * Cc + M8
    h16 = lambda n: torch.empty(n, dtype=torch.float16, device=dev)
    f32 = lambda *shape: torch.empty(*shape, dtype=torch.float32, device=dev)
    n_tap = 3 * Cc // 64
    self.a1, self.a1c = h16(FL * n_tap * 64 * 2 * Cc), h16(FL * (K1 // 64 - n_tap) * 64 * 2 * Cc)
    self.a2, self.es = h16(FL * Cc * Cc), h16(FL * 16 * Cc)
    self.wat, self.wbt = h16(FL * Cc * (Cc + 64)), h16(FL * Cc * 6 * Cc)
    self.wct, self.wup = h16(M8 * FL * 2 * Cc), h16(32 * M8 * 512)
    self.b1, self.b2, self.bup = f32(FL, 2 * Cc), f32(FL, Cc), f32(M8)
    # the transposed upsample of the mel input gradient: packed only for a step that needs d mel
    self.wupt = h16(32 * 4 * M8 * ((hp.n_mel_channels + 31) // 32) * 32) if want_wupt else None
    # per-flow operands as rows of one buffer each
    small = f32(nf, Cc * 4 + Cc + 8 + 64)
    self._small = small
    self.wstart = [small[k, :Cc * (c // 2)] for k, c in enumerate(flow_c)]
    self.bstart = [small[k, 4 * Cc:5 * Cc] for k in range(nf)]
    self.out_init = [small[k, 5 * Cc:5 * Cc + 8] for k in range(nf)]
    self.w1x1 = [small[k, 5 * Cc + 8:5 * Cc + 8 + c * c] for k, c in enumerate(flow_c)]
    arr = lambda ts: (C.c_void_p * nf)(*[t.data_ptr() for t in ts])
    self._arrs = [arr(self.wstart), arr(self.bstart), arr(self.out_init), arr(self.w1x1)]
    # W_k^-1 for synthesis with moving weights (infer_differentiable(weight_grads=True)): inverted by wg_train_prepare
    self.winv = None
    if want_winv:
      self._winv = f32(nf, 64)
      self.winv = [self._winv[k, :c * c] for k, c in enumerate(flow_c)]
      self._arrs.append(arr(self.winv))
    self.struct = _lib.WgTrainWeights(_ptr(self.a1), _ptr(self.a1c), _ptr(self.b1), _ptr(self.a2), _ptr(self.b2), _ptr(self.es),
                                      _ptr(self.wat), _ptr(self.wbt), _ptr(self.wct), _ptr(self.wup), _ptr(self.bup),
                                      C.cast(self._arrs[0], C.c_void_p), C.cast(self._arrs[1], C.c_void_p),
                                      C.cast(self._arrs[2], C.c_void_p), C.cast(self._arrs[3], C.c_void_p),
                                      _ptr(self.wupt) if want_wupt else None,
                                      C.cast(self._arrs[4], C.c_void_p) if want_winv else None)
    self.wn = int(wn)
    ptrs = [t.data_ptr() for t in tensors]
    self.params = (C.c_void_p * len(tensors))(*ptrs)
    self.tensors = tensors
    self.sig = [(t._version, p) for t, p in zip(tensors, ptrs)]
    self.aux = torch.empty(eng.lib.wg_train_prepare_bytes(eng.handle), dtype=torch.uint8, device=dev)
    _lib.check(eng.lib.wg_train_prepare(eng.handle, self.params, self.wn, C.byref(self.struct), _ptr(self.aux),
                                        self.aux.numel(), C.c_void_p(stream)))

  def moved(self, live) -> bool:
    """Whether one of ``live`` -- the parameters ``tensors`` were detached from (a detached tensor shares its parameter's
    version counter, not a storage the parameter is given later) -- was written in place or moved since the library read it."""
    return [(t._version, t.data_ptr()) for t in live] != self.sig


class _SlotGuard:
  """Returns a training workspace to the pool when its autograd graph goes away -- after backward(), or when the
  graph is dropped without one (a loss that is only logged): otherwise every such forward would pin another workspace."""

  _serial = 0

  def __init__(self, slot: dict):
    _SlotGuard._serial += 1
    self.slot, self.token = slot, _SlotGuard._serial
    slot["owner"] = self.token        # a number, not a reference: the guard must die with its graph

  def release(self) -> None:
    if self.slot.get("owner") == self.token:
      self.slot["owner"] = None
      self.slot["busy"] = False          # stream-ordered: the next forward's kernels queue behind pending work

  def __del__(self):
    try:
      self.release()
    except Exception:
      pass


def _ddp_group(model):
  """Process group over which ``backward`` averages gradients itself (``model.ddp_group``; set by
  ``enable_data_parallel``), or None: single process, or the caller reduces with GradientAllReducer."""
  return getattr(model, "ddp_group", None)


def enable_data_parallel(model, group=None, force: bool = False) -> bool:
  """Average gradients inside ``backward``, flow by flow, overlapped with the rest of the backward pass.  Needs an
  initialised ``torch.distributed`` (backend "nccl" = RCCL); returns False (and changes nothing) in a single process
  unless ``force`` (tests of the RCCL path on one GPU)."""
  import torch.distributed as dist
  if not (dist.is_available() and dist.is_initialized()):
    return False
  if dist.get_world_size(group) == 1 and not force:
    return False
  model.ddp_group = group if group is not None else dist.group.WORLD
  return True


def train_workspace_bytes(eng, B: int, n_frames: int, audio_len: int, flags: int) -> int:
  """The library's size of the saved state of one forward of either direction, for the geometry and the wg_train ``flags``;
  its message as a WgError for a geometry it does not take."""
  nbytes = int(eng.lib.wg_train_workspace_bytes(eng.handle, int(B), int(n_frames), int(audio_len), int(flags)))
  if nbytes == 0:
    raise _lib.WgError(eng.lib.wg_last_error().decode())
  return nbytes


def request_workspace(eng, B: int, n_frames: int, audio_len: int, flags: int) -> Tuple[dict, bool]:
  """(slot, fresh) of ``_Engine.train_workspace`` for one forward of either direction: the saved state of its graph, of
  ``train_workspace_bytes``.  The caller hands the slot to a ``_SlotGuard``."""
  return eng.train_workspace(train_workspace_bytes(eng, B, n_frames, audio_len, flags), (B, n_frames, audio_len), flags)


def new_grad(shape, device) -> torch.Tensor:
  """An fp32 gradient tensor the library fills: not cleared -- every entry is written (GradBuffers names the exception) --
  or, under WG_TRAIN_POISON_GRADS=1 (tests), NaN first, so an entry the library leaves out cannot go unnoticed."""
  t = torch.empty(shape, dtype=torch.float32, device=device)
  return t.fill_(float("nan")) if os.environ.get("WG_TRAIN_POISON_GRADS") == "1" else t


def set_grad_finite(model, tensors, scale: float) -> None:
  """Overflow of the fp16 gradient planes (the automatic scale 2^round(log2 N) assumes a loss normalised by N, the
  reference's MEAN loss; another normalisation needs model.grad_scale) or inf / nan inputs: every gradient tensor of a
  backward (None entries aside) is checked, on the device.  model.grad_finite is read by waveglow_amd.training.train()
  before the optimiser step; WG_TRAIN_CHECK_FINITE=1 raises here (one host sync per step).
  (one reduction per tensor: inf / nan anywhere makes a sum non-finite, and 8.6e7 finite fp32 values cannot overflow it)"""
  sums = [t.sum() for t in tensors if t is not None]
  model.grad_finite = torch.isfinite(torch.stack(sums)).all() if len(sums) > 1 else torch.isfinite(sums[0])
  if os.environ.get("WG_TRAIN_CHECK_FINITE") == "1" and not bool(model.grad_finite):
    raise _lib.WgError(nonfinite_message(scale))


def param_grad_views(eng, wts, gstruct, shapes, stream) -> List[torch.Tensor]:
  """Packed gradients (``GradBuffers.struct``) -> one gradient per parameter of ``wts``, in the canonical order: views of
  ONE flat buffer that ``wg_train_param_grads`` fills (weight-norm backward, the fold's chain rule)."""
  sizes = [math.prod(sh) for sh in shapes]
  flat = new_grad(sum(sizes), wts.aux.device)
  _lib.check(eng.lib.wg_train_param_grads(eng.handle, wts.params, wts.wn, C.byref(gstruct), _ptr(wts.aux), wts.aux.numel(),
                                          _ptr(flat), C.c_void_p(stream)))
  return [v.view(sh) for v, sh in zip(flat.split(sizes), shapes)]


class GradBuffers:
  """All gradients of one backward pass in ONE flat fp32 buffer, laid out so that everything that becomes final
  with flow k's backward is contiguous (few, large messages -- xGMI rings are per-link bound):

    [ flow 0 region | flow 1 region | ... | tail ]
    flow region = n_layers records (dw1 | db1 | dw2 | db2 | dwes of one layer) | dstart [5,C] | dout_init [8] | dw1x1 [8,8]
    tail        = dwup [32, M8, 512] | dbup [M8]

  The library writes through strided views (wg_train_grads.layer_stride / flow_stride); ``regions[k]`` is what a
  data-parallel run all-reduces right behind flow k's backward, ``tail`` goes last.  12 + 1 messages per step at the
  reference's 12 flows (25.3 MB per flow, 5.2 MB tail at 256 channels)."""

  def __init__(self, Cc: int, nl: int, nf: int, M8: int, device):
    K1 = 3 * Cc + M8
    sizes = (2 * Cc * K1, 2 * Cc, Cc * Cc, Cc, 8 * Cc)
    self.rec = sum(sizes)
    small = (5 * Cc, 8, 64)
    self.flow_stride = nl * self.rec + sum(small)
    n_tail = 32 * M8 * 512 + M8
    # Not zero-filled (352 MB per step at 256 channels): the library writes every entry except dw2 / db2 of the last
    # layer of each flow (no res rows there, model.py:106-110), which are cleared below.
    self.flat = new_grad(nf * self.flow_stride + n_tail, device)
    self.regions = [self.flat[k * self.flow_stride:(k + 1) * self.flow_stride] for k in range(nf)]
    self.tail = self.flat[nf * self.flow_stride:]
    st = lambda shape, strides, off: self.flat.as_strided(shape, strides, off)
    off, fs, rec = 0, self.flow_stride, self.rec
    self.dw1 = st((nf, nl, 2 * Cc, K1), (fs, rec, K1, 1), off); off += sizes[0]
    self.db1 = st((nf, nl, 2 * Cc), (fs, rec, 1), off); off += sizes[1]
    self.dw2 = st((nf, nl, Cc, Cc), (fs, rec, Cc, 1), off); off += sizes[2]
    self.db2 = st((nf, nl, Cc), (fs, rec, 1), off); off += sizes[3]
    self.dwes = st((nf, nl, 8, Cc), (fs, rec, Cc, 1), off)
    off = nl * rec
    self.dstart = st((nf, 5, Cc), (fs, Cc, 1), off); off += small[0]
    self.dout_init = st((nf, 8), (fs, 1), off); off += small[1]
    self.dw1x1 = st((nf, 8, 8), (fs, 8, 1), off)
    self.dwup = self.tail[:32 * M8 * 512].view(32, M8, 512)
    self.dbup = self.tail[32 * M8 * 512:]
    self.nf = nf
    self.dw2[:, nl - 1].zero_()
    self.db2[:, nl - 1].zero_()

  def struct(self):
    """(wg_train_grads, keep-alive list)."""
    arr = lambda t: (C.c_void_p * self.nf)(*[t[k].data_ptr() for k in range(self.nf)])
    keep = [arr(self.dstart), arr(self.dout_init), arr(self.dw1x1)]
    g = _lib.WgTrainGrads(_ptr(self.dw1), _ptr(self.db1), _ptr(self.dw2), _ptr(self.db2), _ptr(self.dwes),
                          _ptr(self.dwup), _ptr(self.dbup), C.cast(keep[0], C.c_void_p), C.cast(keep[1], C.c_void_p),
                          C.cast(keep[2], C.c_void_p), self.rec, self.flow_stride)
    return g, keep


def flow_backward_schedule(n_flows: int, run_flow, bufs, group=None) -> None:
  """The data-parallel backward schedule, independent of what computes the gradients (so that the CPU tests drive it
  with a stub): flows are processed last to first; as soon as ``run_flow(k)`` has queued flow k's backward its region of
  the flat gradient buffer is final on the stream and goes out as ONE asynchronous all-reduce (RCCL runs on its own
  stream, ordered after the work queued so far), overlapping the backward of flows k-1 .. 0; the tail (upsample
  gradients, final with flow 0) follows; then everything is awaited and divided by the world size -- the reference's
  loss is a mean over the LOCAL batch (train.py:44), so the mean over ranks is the gradient of the concatenated batch.
  ``bufs`` needs ``regions`` (one tensor per flow), ``tail`` and ``flat``.  ``group`` None: no exchange."""
  if group is None:
    for k in reversed(range(n_flows)):
      run_flow(k)
    return
  import torch.distributed as dist
  works = []
  for k in reversed(range(n_flows)):
    run_flow(k)
    works.append(dist.all_reduce(bufs.regions[k], op=dist.ReduceOp.SUM, group=group, async_op=True))
  works.append(dist.all_reduce(bufs.tail, op=dist.ReduceOp.SUM, group=group, async_op=True))
  for wk in works:
    wk.wait()
  world = dist.get_world_size(group)
  if world > 1:
    bufs.flat.mul_(1.0 / world)


def begin_node(ctx, what: str, model, eng, params, wn, flags: int, dims, n_out: int, scale: float, stream,
               want_wupt: bool, want_winv: bool = False):
  """Forward side of the lifecycle the two autograd nodes share (``what`` names the call in their refusals): the per-call
  weights from ``wg_train_prepare``, one pool workspace for ``dims = (B, n_frames, audio_len)`` behind a guard that returns
  it when the graph goes away (also when the node's forward call raises), and on ``ctx`` what the backward side needs: flags,
  parameters, shapes, the loss scale (``scale``, or 2^round(log2 ``n_out``)).  Returns ``(weights, workspace, fresh)``."""
  wts = _Weights(model, [p.detach() for p in params], wn, model.flow_channels(), eng, stream, want_wupt=want_wupt,
                 want_winv=want_winv)
  slot, fresh = request_workspace(eng, *dims, flags)                         # held until this graph's backward has run
  ctx.what, ctx.model, ctx.eng, ctx.wts, ctx.ws, ctx.guard = what, model, eng, wts, slot["ws"], _SlotGuard(slot)
  ctx.dims, ctx.flags, ctx.params, ctx.shapes = dims, flags, params, [t.shape for t in params]
  ctx.scale = float(scale) if scale else float(2.0 ** round(math.log2(n_out)))
  return wts, slot["ws"], fresh


def finish_node(ctx, n_meta: int, need_p, launch, also_stale: bool = False):
  """Backward side.  Refused before any launch: a second backward() of one graph, and weights that moved since the forward
  (written in place, another storage, another engine; ``also_stale``: the node's own reason) -- the saved state belongs to
  the old weights, and ``wg_train_param_grads`` would read the new ones.  ``launch(eng, wts, bufs, grads_ptr, stream)``
  issues the node's own calls (``bufs``: a ``GradBuffers`` when ``need_p`` asks for a parameter gradient, else None) and
  returns its data gradients in input order; raised or not, the workspace goes back to the pool and the saved state goes.
  Returns backward()'s tuple: ``n_meta`` Nones, the data gradients, one gradient (or None) per parameter."""
  model, wts, eng = ctx.model, ctx.wts, ctx.eng
  if wts is None:
    raise _lib.WgError(f"the saved state of this {ctx.what} call is gone: backward() already ran for it "
                       "(retain_graph is not supported)")
  if also_stale or model._engine is not eng or wts.moved(ctx.params):
    ctx.wts = None
    ctx.guard.release()
    raise _lib.WgError(f"the weights changed between {ctx.what} and backward(): the saved state belongs to the old weights")
  hp, dev = model._hp, ctx.ws.device
  stream = torch.cuda.current_stream(dev).cuda_stream
  want_params = any(need_p)
  bufs = GradBuffers(hp.n_channels, hp.n_layers, model.n_flows, hp.n_mel_channels * 8, dev) if want_params else None
  gstruct, _keep = bufs.struct() if want_params else (None, None)
  views = [None] * len(ctx.shapes)
  try:
    data_grads = launch(eng, wts, bufs, C.byref(gstruct) if want_params else None, stream)
    if want_params:
      views = param_grad_views(eng, wts, gstruct, ctx.shapes, stream)
  finally:
    ctx.guard.release()
    ctx.wts = None
  set_grad_finite(model, [bufs.flat if want_params else None, *data_grads], ctx.scale)
  return (None,) * n_meta + (*data_grads, *[v if w else None for v, w in zip(views, need_p)])


class _TrainFn(torch.autograd.Function):
  """Inputs: model, the loss scale, the weight-norm flag, the wg_train flags (``WG_TRAIN_RECOMPUTE``: activation
  recomputation; the backward runs with the flags of its own forward), mel, audio and the module's parameters in the
  library's canonical order (``canonical_params``); outputs (z, log_s...).  backward() returns what
  ``ctx.needs_input_grad`` asks for: d mel / d audio (written by the library into tensors of their own), and one gradient
  per parameter, each a view of ONE flat buffer the library fills -- or, when no parameter needs one (a frozen model used
  as a loss), no parameter gradient at all: the library then runs the data-gradient chain alone
  (include/waveglow_amd.h: wg_train_backward)."""

  N_META = 4      # model, scale, wn, flags

  @staticmethod
  def forward(ctx, model, scale, wn, flags, mel, audio, *params):
    eng = model._get_engine(mel.device, need_weights=False)
    B, M, F_ = mel.shape
    S = audio.shape[1]
    L = S // model.n_group
    if int(eng.lib.wg_wn_waves(model._hp.n_channels)) <= 0:
      raise _lib.WgError(f"n_channels={model._hp.n_channels} unsupported (64, 128, 256, 512)")
    stream = torch.cuda.current_stream(mel.device).cuda_stream
    wts, ws, fresh = begin_node(ctx, "forward", model, eng, params, wn, flags, (B, F_, S), B * model.n_group * L, scale,
                                stream, want_wupt=ctx.needs_input_grad[_TrainFn.N_META])
    z = torch.empty((B, model.n_group, L), dtype=torch.float32, device=mel.device)
    log_s = [torch.empty((B, c // 2, L), dtype=torch.float32, device=mel.device) for c in model.flow_channels()]
    ls = (C.c_void_p * len(log_s))(*[t.data_ptr() for t in log_s])
    _lib.check(eng.lib.wg_train_forward(eng.handle, C.byref(wts.struct), _ptr(mel), _ptr(audio), _ptr(z), ls, B, F_, S,
                                        1 if fresh else 0, _ptr(ws), ws.numel(), flags, C.c_void_p(stream)))
    ctx.audio = audio
    return (z, *log_s)

  @staticmethod
  def backward(ctx, g_z, *g_log_s):
    nm = _TrainFn.N_META
    want_mel, want_audio = ctx.needs_input_grad[nm], ctx.needs_input_grad[nm + 1]

    def launch(eng, wts, bufs, gs_ptr, stream):
      model = ctx.model
      B, F_, S = ctx.dims
      dev, nf = ctx.audio.device, model.n_flows
      g_mel = new_grad((B, model._hp.n_mel_channels, F_), dev) if want_mel else None
      g_audio = new_grad((B, S), dev) if want_audio else None
      gz = g_z.float().contiguous() if g_z is not None else None
      gls = [g.float().contiguous() if g is not None else None for g in g_log_s]
      gl_arr = (C.c_void_p * nf)(*[(g.data_ptr() if g is not None else None) for g in gls])

      def run_flows(hi, lo):
        _lib.check(eng.lib.wg_train_backward(eng.handle, C.byref(wts.struct), gs_ptr, _ptr(gz), gl_arr,
                                             C.c_float(ctx.scale), _ptr(ctx.audio), _ptr(g_mel), _ptr(g_audio), B, F_, S,
                                             _ptr(ctx.ws), ctx.ws.numel(), hi, lo, ctx.flags, C.c_void_p(stream)))
      # input gradients stay local (as under torch DDP); only parameter gradients are averaged over the ranks
      group = _ddp_group(model) if bufs is not None else None
      if group is None:
        run_flows(nf - 1, 0)
      else:
        # Data parallel: the backward pass is cut at flow boundaries and every flow's gradients -- ONE contiguous region
        # of the flat buffer -- are all-reduced right behind it (flow_backward_schedule).  What follows (weight-norm
        # backward, the fold's chain rule: wg_train_param_grads) is linear in these gradients, so averaging here equals
        # averaging the parameter gradients (the logdet term of the 1x1 weights is identical on every rank).
        flow_backward_schedule(nf, lambda k: run_flows(k, k), bufs, group)
      return g_mel, g_audio

    return finish_node(ctx, nm, ctx.needs_input_grad[nm + 2:], launch)


def nonfinite_message(scale: float) -> str:
  return ("non-finite gradients: the fp16 gradient planes overflowed (or the inputs held inf / nan).  The automatic loss "
          "scale assumes the reference's mean-normalised WaveGlowLoss (train.py:43-44); for a differently normalised loss "
          "set model.grad_scale (currently %s) so that scale * |dL/dz| stays below 65504" % (("%g" % scale) if scale else "automatic"))


def train_forward(model, mel: torch.Tensor, audio: torch.Tensor, grad_scale: float = 0.0, recompute: bool = False):
  """(z, [log_s_k], [log_det_W_k]) with an autograd graph back to the module's parameters and to ``mel`` / ``audio``
  (model.py:178-221).  The crop to a multiple of n_group and ``.contiguous()`` are torch ops in front of the autograd
  node: dropped trailing samples get a zero gradient and the input gradients the inputs' own shapes.  ``recompute``:
  activation recomputation (``WG_TRAIN_RECOMPUTE``, ``WaveGlow.recompute_activations``)."""
  if mel.device.type != "cuda":
    raise _lib.WgError("waveglow_amd runs on MI355X only: there is no CPU fallback")
  if mel.dtype != torch.float32 or audio.dtype != torch.float32:
    raise _lib.WgError("the training direction takes float32 mel / audio (reference: fp32 training)")
  B, M, F_ = mel.shape
  S = audio.shape[1]
  assert (F_ - 1) * 256 + 1024 >= S                    # model.py:187
  S = S - S % model.n_group                            # unfold drops the remainder (model.py:191,195)
  audio = audio[:, :S].contiguous()
  mel = mel.contiguous()
  eng = model._get_engine(mel.device, need_weights=False)
  if eng.width != eng.n_channels or eng.mel_width != eng.n_mel:
    raise _lib.WgError(f"n_channels={eng.n_channels}, n_mel_channels={eng.n_mel}: the training direction takes the kernel widths "
                       f"{eng.KERNEL_WIDTHS} and mel counts that are multiples of 16 only (inference and the no-grad forward "
                       "zero-pad the others)")
  _names, tensors, wn = canonical_params(model, eng)
  flags = _lib.WG_TRAIN_RECOMPUTE if recompute else 0
  out = _TrainFn.apply(model, grad_scale, wn, flags, mel, audio, *tensors)
  z, log_s = out[0], list(out[1:])
  L = S // model.n_group
  return z, log_s, _log_det_w(model, B * L)


def _log_det_w(model, n: int) -> List[torch.Tensor]:
  """``batch_size * n_of_groups * torch.logdet(W)`` of every flow (model.py:63) as ONE batched LU: each c_k x c_k matrix
  sits in the top-left corner of an 8 x 8 identity (same pivots, det x 1), so the twelve flows cost the ~20 small
  kernels of one ``logdet`` (forward and backward) instead of twelve times that -- 1.5 ms of launch latency per step at
  config 4.  Returns the reference's list of 0-dim tensors (views of one vector)."""
  ws = [model.convinv[k].conv.weight.squeeze(2) for k in range(model.n_flows)]
  dev = ws[0].device
  ng = model.n_group
  key = (str(dev), tuple(w.shape[0] for w in ws))
  cache = getattr(model, "_logdet_pad", None)
  if cache is None or cache[0] != key:
    base = torch.eye(ng, device=dev).repeat(len(ws), 1, 1)
    idx = torch.cat([(k * ng * ng + torch.arange(c)[:, None] * ng + torch.arange(c)[None, :]).reshape(-1)
                     for k, c in enumerate(key[1])]).to(dev)
    cache = (key, base.reshape(-1), idx)
    model._logdet_pad = cache
  _, base, idx = cache
  padded = base.index_put((idx,), torch.cat([w.reshape(-1) for w in ws])).view(len(ws), ng, ng)
  return list((n * torch.logdet(padded)).unbind(0))
