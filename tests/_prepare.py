"""wg_train_prepare against the same computation written as torch ops: the body shared by
tests/test_gpu_train.py::test_prepare_matches_torch_packing and tests/test_gpu_offmanifold.py."""
import importlib

import torch

import _packing as P
from waveglow_amd.model import WaveGlow

T = importlib.import_module("waveglow_amd.train")      # the package also exports a function of this name


def check_prepare_matches_torch_packing(hp, sd, wn):
  """``sd``: a weight-normed state dict for ``hp``; ``wn`` False: the model is checked after remove_weightnorm.
  wg_train_prepare (the library reads the module's own parameter tensors: weight norm, W_end x W_skip fold, permutations,
  gate pre-scale, fragment orders -- train_prep.hip, pack_kernel) against tests/_packing.py: pack_weights,
  wn_forward_fragments, plain_fragments, to_fragments.  Dense weights: every tensor that is pure data movement is
  bit-identical; with weight norm (and for the fold) the fp32 summation order differs from torch's, so fp16 values may
  differ in the last place."""
  model = WaveGlow(hp)
  model.load_state_dict(sd)
  if not wn:
    model = WaveGlow.remove_weightnorm(model)
  model = model.to("cuda:0").train()
  eng = model._get_engine(torch.device("cuda:0"), need_weights=False)
  NW = int(eng.lib.wg_wn_waves(hp.n_channels))
  with torch.no_grad():
    packed = [t.detach() for t in P.pack_weights(model)]
    names, tensors, is_wn = T.canonical_params(model, eng)
    assert is_wn == wn and len(tensors) == len(list(model.parameters()))
    w = T._Weights(model, tensors, wn, model.flow_channels(), eng, torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    Cc, M8 = hp.n_channels, hp.n_mel_channels * 8
    pm = P._perms(Cc, M8, packed[0].device)
    a1, a1c, b1s, a2, es = P.wn_forward_fragments(packed[0], packed[1], packed[2], packed[4], pm, NW)
    FL = packed[0].shape[0]
    w1h = packed[0].half()
    w1c = w1h[:, :, 3 * Cc:].index_select(1, pm.c2).index_select(2, pm.m8)
    wat_m = torch.cat([packed[2].transpose(1, 2).index_select(2, pm.c),
                       torch.nn.functional.pad(packed[4].half().float(), (0, 0, 0, 56)).transpose(1, 2)], 2)
    want = {"a1": a1, "a1c": a1c, "a2": a2, "es": es,
            "wat": P.plain_fragments(wat_m.half(), NW),
            "wbt": P.plain_fragments(torch.cat([w1h[:, :, t * Cc:(t + 1) * Cc].transpose(1, 2).index_select(2, pm.c2)
                                                for t in range(3)], 2), NW),
            "wct": P.to_fragments(w1c.permute(2, 0, 1).reshape(-1, FL * 2 * Cc), pm.c2p),
            "wup": P.to_fragments(packed[5].index_select(1, pm.m8).half(), pm.c2p)}
    for name, t in want.items():
      got = getattr(w, name)
      assert got.numel() == t.numel(), name
      if not wn and name not in ("es", "wat"):
        assert torch.equal(got.view(-1).view(torch.int16), t.reshape(-1).view(torch.int16)), name
      else:
        g32, t32 = got.view(-1).float(), t.reshape(-1).float()
        if name == "es":      # [FL, s, l4, 16 rows, 8]: rows 0-7 the hi fp16 half, 8-15 the lo half -- their SUM is the value
          g32, t32 = [x.view(FL, Cc // 32, 4, 2, 8, 8).sum(3).reshape(-1) for x in (g32, t32)]
        tol = 1.5e-3 * t32.abs() + 1e-6
        assert bool(((g32 - t32).abs() <= tol).all()), (name, float((g32 - t32).abs().max()))
    assert torch.allclose(w.b1, b1s, rtol=1e-6, atol=1e-7)
    assert torch.allclose(w.b2, packed[3], rtol=1e-6, atol=1e-7)
    assert torch.equal(w.bup, packed[6].index_select(0, pm.m8))
    start5, out_init, w1x1 = packed[7].index_select(2, pm.c), packed[8], packed[9]
    for k, c in enumerate(model.flow_channels()):
      assert torch.allclose(w.wstart[k].view(Cc, c // 2), start5[k, :c // 2].transpose(0, 1), rtol=2e-6, atol=1e-7), k
      assert torch.equal(w.bstart[k], start5[k, 4]), k
      assert torch.allclose(w.out_init[k], out_init[k], rtol=1e-5, atol=1e-6), k
      assert torch.equal(w.w1x1[k].view(c, c), w1x1[k, :c, :c]), k
