"""Differentiable synthesis: ``WaveGlow.infer_differentiable`` under autograd on the HIP library.

Reference: src/waveglow/model.py:223-273 (``infer``; the reference ends it with ``.data``, so its output never carries a
graph).  Here the output of the frozen vocoder carries one back to ``mel`` and to the noise, so that a waveform-domain loss
(a multi-resolution STFT loss, a discriminator) can train an acoustic model, or optimise a mel or a noise tensor, through
it.  By default the weights are constants: a parameter that requires grad is refused, never silently dropped.  With
``weight_grads=True`` the graph reaches the vocoder's own parameters as well (fine-tuning WaveGlow on a loss on what it
synthesises): the backward then also runs the training direction's weight-gradient launches, flow by flow, and
``wg_train_param_grads``; the inverse 1x1 matrices come from the per-call weights (inverted on the device by
``wg_train_prepare``), so an optimiser step costs no re-finalisation of the inference engine.

* ``wg_train_infer_forward``: the same 12 WN stacks as the training direction (``wg_train_forward``), in inverse flow
  order, with the training kernels' saved activations and the state that enters every inverse step; the inverse 1x1
  matrices are the fp64-computed ones ``infer`` uses (the engine is finalised with the current weights);
* ``wg_train_infer_backward``: ascending flow order, two row kernels per flow around the training direction's WN
  data-gradient chain, then the d spect GEMM and the transposed upsample for ``d mel``; with ``grads`` also the packed
  weight gradients (``GradBuffers``), among them ``d W_k = - sum (W_k^-T d w) (x) w`` of every inverse 1x1 step.

Both take the per-utterance frame counts of a padded batch (``infer_differentiable(..., frames=)``: int32 [B] on the
device, kept on ``ctx`` for the backward), or none for a dense one.

The node's lifecycle is ``_TrainFn``'s (waveglow_amd/train.py: ``begin_node`` / ``finish_node``): per-call weights from
``wg_train_prepare``, one training workspace per outstanding graph, the fp16 loss scale and ``model.grad_finite``, the
refusal of a second backward() and of weights that moved in between.  Its own: its two library calls, and in the frozen
mode the rule that the inference engine was not re-finalised since.  There is no fallback: CPU tensors raise.
"""
from __future__ import annotations

import ctypes as C
from typing import List

import torch

from . import _args, _lib
from ._args import ptr as _ptr
from .train import _ddp_group, begin_node, canonical_params, finish_node, new_grad


class _InferFn(torch.autograd.Function):
  """Inputs: model, sigma, loss scale (0 = automatic), weight-norm flag, wg_train flags (``WG_TRAIN_RECOMPUTE``: activation
  recomputation, the backward runs with its forward's flags), number of early-noise tensors, the weight-gradient mode, the
  frame counts of a ragged batch (int32 [B] on the device, or None: kept on ``ctx`` for the backward, never differentiated), mel,
  z_init, z_early..., then the module's parameters in the library's canonical order (the library reads them through
  ``wg_train_prepare``; without the weight-gradient mode they are constants: never differentiated).  Output: audio
  [B, 256 T] fp32.  backward() returns only what ``ctx.needs_input_grad`` asks for among mel, z_init, the z_early entries
  and -- in the weight-gradient mode -- the parameters, each parameter gradient a view of ONE flat buffer (as ``_TrainFn``)."""

  N_META = 8      # model, sigma, scale, wn, flags, n_early, wgrads, frames

  @staticmethod
  def forward(ctx, model, sigma, scale, wn, flags, n_early, wgrads, frames, mel, z_init, *rest):
    z_early, params = rest[:n_early], rest[n_early:]
    # frozen: finalised with the current weights, the W^-1 of infer.  Weight-gradient mode: the weights move every step,
    # W^-1 comes with the per-call weights and the inference engine is left alone
    eng = model._get_engine(mel.device, need_weights=not wgrads)
    B, M, T = mel.shape
    S = 256 * T
    stream = _args.stream(mel.device).value     # as an int: _Weights takes it so
    # the automatic scale assumes a loss normalised by the number of samples (|d loss / d audio| ~ 1 / N)
    wts, ws, fresh = begin_node(ctx, "infer_differentiable", model, eng, params, wn, flags, (B, T, S), B * S, scale, stream,
                                want_wupt=ctx.needs_input_grad[_InferFn.N_META], want_winv=wgrads)
    audio = torch.empty((B, S), dtype=torch.float32, device=mel.device)
    ze = (C.c_void_p * max(1, n_early))(*[z.data_ptr() for z in z_early])
    _lib.check(eng.lib.wg_train_infer_forward(eng.handle, C.byref(wts.struct), _ptr(mel), _ptr(z_init), ze, n_early,
                                              float(sigma), _ptr(audio), B, T, _ptr(frames),
                                              1 if fresh else 0, _ptr(ws), ws.numel(), flags, C.c_void_p(stream)))
    ctx.frames, ctx.wgrads, ctx.sigma, ctx.n_early, ctx.n_mel = frames, wgrads, float(sigma), n_early, M
    ctx.sig = eng.signature                     # frozen: the engine whose W^-1 the forward used must still be this one
    ctx.z_shapes = [tuple(z_init.shape)] + [tuple(z.shape) for z in z_early]
    return audio

  @staticmethod
  def backward(ctx, g_audio):
    ne, nm, need = ctx.n_early, _InferFn.N_META, ctx.needs_input_grad
    want_mel, want_zi = need[nm], need[nm + 1]
    want_ze = need[nm + 2:nm + 2 + ne]
    need_p = need[nm + 2 + ne:] if ctx.wgrads else (False,) * len(ctx.shapes)

    def launch(eng, wts, bufs, gs_ptr, stream):      # (no logdet term in this direction)
      B, T, S = ctx.dims
      dev = ctx.ws.device
      g_mel = new_grad((B, ctx.n_mel, T), dev) if want_mel else None
      g_zi = new_grad(ctx.z_shapes[0], dev) if want_zi else None
      g_ze = [new_grad(ctx.z_shapes[1 + i], dev) if w else None for i, w in enumerate(want_ze)]
      ga = g_audio.float().contiguous() if g_audio is not None else torch.zeros((B, S), dtype=torch.float32, device=dev)
      ze = (C.c_void_p * max(1, ne))(*[(g.data_ptr() if g is not None else None) for g in g_ze])
      _lib.check(eng.lib.wg_train_infer_backward(eng.handle, C.byref(wts.struct), gs_ptr, _ptr(ga), C.c_float(ctx.scale),
                                                 C.c_float(ctx.sigma), _ptr(g_mel), _ptr(g_zi), ze, ne, B, T,
                                                 _ptr(ctx.frames), _ptr(ctx.ws), ctx.ws.numel(), ctx.flags,
                                                 C.c_void_p(stream)))
      return (g_mel, g_zi, *g_ze)

    return finish_node(ctx, nm, need_p, launch, also_stale=not ctx.wgrads and ctx.eng.signature != ctx.sig)


def infer_differentiable(model, spect: torch.Tensor, z_init: torch.Tensor, z_early: List[torch.Tensor], sigma: float,
                         grad_scale: float = 0.0, recompute: bool = False, weight_grads: bool = False,
                         frames=None) -> torch.Tensor:
  """``model.infer_with_noise(spect, z_init, z_early, sigma)`` (fp32) with an autograd graph back to ``spect``, ``z_init``
  and every ``z_early[i]`` that requires grad -- and, with ``weight_grads``, to every parameter that requires grad.
  Without grad mode, or when nothing requires grad, exactly ``infer_with_noise`` (nothing is saved).  ``recompute``:
  activation recomputation (``WG_TRAIN_RECOMPUTE``).  ``frames``: per-utterance mel-frame counts of a ragged batch
  (``WaveGlow.infer_differentiable``), None for a dense one."""
  # the counts first: refused for what is wrong with them before any launch and before anything else about the call is
  # looked at.  Host counts are checked where they are and go up only once a graph is certain; device counts are trusted
  fr = fr_host = None
  if frames is not None:
    if spect.dim() != 3:
      raise _lib.WgError(f"infer_differentiable: mel [B, n_mel, T] expected, got {tuple(spect.shape)}")
    on_device = isinstance(frames, torch.Tensor) and frames.device.type != "cpu"
    fr, fr_host = _args.counts("infer_differentiable: frame counts", frames, spect.shape[0], 1, spect.shape[2],
                               device=spect.device if on_device else "cpu", allow_device=True)
  ins = [spect, z_init] + list(z_early)
  for t in ins:
    _args.tensor("infer_differentiable: mel and noise (the training direction's kernels)", t, ndim=3)
  eng = model._get_engine(spect.device, need_weights=False)
  if eng.width != eng.n_channels or eng.mel_width != eng.n_mel or int(eng.lib.wg_wn_waves(eng.n_channels)) <= 0:
    raise _lib.WgError(f"n_channels={eng.n_channels}, n_mel_channels={eng.n_mel}: infer_differentiable runs on the training "
                       f"direction's kernels, which take the widths {eng.KERNEL_WIDTHS} and mel counts that are multiples "
                       "of 16 only (infer / infer_with_noise zero-pad the others)")
  B, M, T = spect.shape
  L = T * 256 // model.n_group
  if tuple(z_init.shape) != (B, model.n_remaining_channels, L):
    raise _lib.WgError(f"z_init: expected shape {(B, model.n_remaining_channels, L)}, got {tuple(z_init.shape)}")
  n_early = model.n_early_flows()
  if len(z_early) != n_early or any(tuple(z.shape) != (B, model.n_early_size, L) for z in z_early):
    raise _lib.WgError(f"z_early: expected {n_early} tensors of shape {(B, model.n_early_size, L)}")
  if weight_grads and _ddp_group(model) is not None:
    raise _lib.WgError("infer_differentiable(weight_grads=True) does not average gradients over a process group "
                       "(enable_data_parallel covers the training direction only): unset model.ddp_group and reduce the "
                       "parameter gradients yourself")
  if not torch.is_grad_enabled():
    return model.infer_with_noise(spect, z_init, z_early, sigma, frames=fr)
  trainable = any(p.requires_grad for p in model.parameters())
  if trainable and not weight_grads:
    raise _lib.WgError("infer_differentiable treats the vocoder's weights as constants and gives no weight gradients: "
                       "freeze the model first (model.requires_grad_(False)) or ask for them (weight_grads=True)")
  if not trainable and not any(t.requires_grad for t in ins):
    return model.infer_with_noise(spect, z_init, z_early, sigma, frames=fr)
  _names, tensors, wn = canonical_params(model, eng)
  ins = [t.contiguous() for t in ins]
  flags = _lib.WG_TRAIN_RECOMPUTE if recompute else 0
  if fr_host is not None:
    fr = fr.to(spect.device)                   # one small copy, nothing synchronises
  elif fr is not None:
    # trusted device counts: one outside [1, T] becomes 0, which the kernels take as an utterance that is all padding
    fr = fr.masked_fill((fr < 1) | (fr > spect.shape[2]), 0)
  return _InferFn.apply(model, float(sigma), float(grad_scale), wn, flags, n_early, bool(weight_grads), fr, *ins, *tensors)
