"""Streaming synthesis without a GPU: the halo of ``stream_halo`` against the oracle by NaN poisoning (exact and tight),
the chunk planner's properties, and the planner driven end to end on the fp64 oracles -- window crops of mel and noise
as a session slices them, interiors concatenated, against the whole utterance.  The offsets are where this feature can
be wrong without any kernel being wrong."""
import itertools
from unittest import mock

import numpy as np
import pytest
import torch

from _cases import oracle_cfg_from_hp
from oracle import stft_oracle
from oracle.torch_oracle import infer_ref
from waveglow_amd import streaming as S
from waveglow_amd import synthetic
from waveglow_amd.hparams import HParams

SIGMA = 0.8
# (n_layers, T, interior [s, e)); 4 flows, 64 channels, an early output every 2 flows
HALO_CASES = {"4x3": (3, 24, (8, 12)), "4x4": (4, 40, (16, 24))}


def _hp(n_layers):
  return HParams(n_flows=4, n_early_every=2, n_layers=n_layers, n_channels=64)


def _inputs(hp, T, dtype=torch.float32):
  sd = {k: v.to(dtype) for k, v in synthetic.make_state_dict(hp).items()}
  mel = synthetic.make_mel(1, T, hp.n_mel_channels).to(dtype)
  z_init, z_early = synthetic.make_noise(hp, 1, 32 * T)
  return sd, mel, z_init.to(dtype), {k: v.to(dtype) for k, v in z_early.items()}


def _infer(sd, mel, z_init, z_early, hp):
  """``infer_ref`` in the tensors' dtype.  The oracle inverts W in fp32 as the reference does (``W.float().inverse()``);
  an fp64 run keeps the weight's dtype there, nothing else of it calls ``.float()``."""
  with torch.no_grad():
    if mel.dtype == torch.float64:
      with mock.patch.object(torch.Tensor, "float", lambda t: t):
        return infer_ref(sd, mel, z_init, z_early, SIGMA, oracle_cfg_from_hp(hp))
    return infer_ref(sd, mel, z_init, z_early, SIGMA, oracle_cfg_from_hp(hp))


@pytest.fixture(scope="module", params=sorted(HALO_CASES))
def halo_case(request):
  n_layers, T, (s, e) = HALO_CASES[request.param]
  hp = _hp(n_layers)
  sd, mel, z_init, z_early = _inputs(hp, T)
  clean = _infer(sd, mel, z_init, z_early, hp)
  assert bool(torch.isfinite(clean).all())
  return hp, sd, mel, z_init, z_early, T, s, e, clean


def _poisoned(case, mel_lo, mel_hi, col_lo, col_hi):
  """The interior's audio with every mel frame outside [mel_lo, mel_hi) and every noise column outside [col_lo, col_hi)
  set to NaN."""
  hp, sd, mel, z_init, z_early, T, s, e, _ = case
  assert 0 < mel_lo and mel_hi < T and 0 < col_lo and col_hi < 32 * T       # there is something to poison on every side
  m = mel.clone()
  m[:, :, :mel_lo] = float("nan")
  m[:, :, mel_hi:] = float("nan")

  def cut(z):
    z = z.clone()
    z[:, :, :col_lo] = float("nan")
    z[:, :, col_hi:] = float("nan")
    return z
  return _infer(sd, m, cut(z_init), {k: cut(v) for k, v in z_early.items()}, hp)[:, 256 * s:256 * e]


def test_halo_is_exact(halo_case):
  hp, _, _, _, _, _, s, e, clean = halo_case
  ml, mr, R, df = S.stream_halo(hp)
  assert R == hp.n_flows * (2 ** hp.n_layers - 1) and mr == -(-R // 32) and ml == mr + 3 and df == 3
  got = _poisoned(halo_case, s - ml, e + mr, 32 * s - R, 32 * e + R)
  assert bool(torch.isfinite(got).all())
  assert torch.equal(got, clean[:, 256 * s:256 * e])


@pytest.mark.parametrize("short", ["mel_left", "mel_right", "noise_left", "noise_right"])
def test_halo_is_tight(halo_case, short):
  """One mel frame or one noise column less on any side, and NaN reaches the interior."""
  hp, _, _, _, _, _, s, e, _ = halo_case
  ml, mr, R, _ = S.stream_halo(hp)
  d = {k: int(k == short) for k in ("mel_left", "mel_right", "noise_left", "noise_right")}
  got = _poisoned(halo_case, s - ml + d["mel_left"], e + mr - d["mel_right"], 32 * s - R + d["noise_left"],
                  32 * e + R - d["noise_right"])
  assert bool(torch.isnan(got).any())


def test_default_model_halo():
  assert S.stream_halo(HParams()) == (99, 96, 3060, 3)
  assert S.halo_frames(HParams(), True) == (102, 99) and S.halo_frames(HParams(), False) == (99, 96)


# ---------------------------------------------------------------------------------------------- planner properties
T_SET, C_SET = (1, 3, 4, 7, 40, 41), (1, 8, 13, 40, 64)
HALOS = {False: (5, 2), True: (8, 5)}        # the 4 x 4 model's (Hl, Hr): T_SET has utterances shorter and longer than a halo


@pytest.mark.parametrize("denoise", [False, True])
@pytest.mark.parametrize("T,C", list(itertools.product(T_SET, C_SET)))
def test_planner_tiles_the_utterance(T, C, denoise):
  Hl, Hr = HALOS[denoise]
  plans = S.plan_stream(T, C, Hl, Hr, closed=True)
  assert len(plans) == -(-T // C)
  at = 0
  for j, p in enumerate(plans):
    assert p.index == j and p.start_sample == at == 256 * j * C            # exactly once and in order
    assert p.count == 256 * (min((j + 1) * C, T) - j * C) > 0
    at += p.count
    # the window holds the chunk plus the halo, or reaches the utterance's edge
    assert p.w0 == max(0, j * C - Hl) and p.w1 == min(T, (j + 1) * C + Hr)
    assert p.offset == 256 * (j * C - p.w0) and p.offset + p.count <= 256 * (p.w1 - p.w0)
    assert p.w1 - p.w0 <= C + Hl + Hr
    assert p.final == (j == len(plans) - 1)
  assert at == 256 * T


@pytest.mark.parametrize("denoise", [False, True])
@pytest.mark.parametrize("T,C", list(itertools.product(T_SET, C_SET)))
def test_planner_emission_times(T, C, denoise):
  """An open stream emits chunk j exactly when (j + 1) C + Hr frames are there, with the window it has in the closed
  stream unless the utterance's end cuts that one short; close() releases the rest."""
  Hl, Hr = HALOS[denoise]
  closed = S.plan_stream(T, C, Hl, Hr, closed=True)
  for frames in range(T + 1):
    n = S.ready_chunks(frames, C, Hr, closed=False)
    assert n == sum(1 for j in range(len(closed)) if (j + 1) * C + Hr <= frames)
    assert S.plan_chunk(n, frames, C, Hl, Hr, closed=False) is None
    for j in range(n):
      p = S.plan_chunk(j, frames, C, Hl, Hr, closed=False)
      assert (p.w0, p.w1, p.offset, p.count, p.start_sample) == (max(0, j * C - Hl), (j + 1) * C + Hr, closed[j].offset,
                                                                 256 * C, closed[j].start_sample)
      assert not p.final
      if (j + 1) * C + Hr <= T:
        assert p == closed[j]
  assert S.ready_chunks(T, C, Hr, closed=True) == len(closed) and closed[-1].final


# ---------------------------------------------------------------------------------------------- end to end, fp64
@pytest.fixture(scope="module")
def whole64():
  hp, T = _hp(4), 40
  sd, mel, z_init, z_early = _inputs(hp, T, torch.float64)
  raw = _infer(sd, mel, z_init, z_early, hp)
  fwd, inv, wsq = stft_oracle.bases()
  rng = np.random.default_rng(5)
  bias = stft_oracle.bias_spectrum(0.3 * rng.standard_normal((1, 4096)), fwd)
  den = stft_oracle.denoise(raw.numpy(), bias, 0.1, fwd, inv, wsq)
  assert np.abs(den - raw.numpy()).max() > 1e-3 * np.abs(raw.numpy()).max()      # the subtraction changes samples
  return hp, T, sd, mel, z_init, z_early, raw, den, (bias, fwd, inv, wsq)


@pytest.mark.parametrize("denoise", [False, True])
@pytest.mark.parametrize("C", [1, 8, 13, 40, 64])
def test_planned_windows_reproduce_the_whole_utterance(whole64, C, denoise):
  hp, T, sd, mel, z_init, z_early, raw, den, (bias, fwd, inv, wsq) = whole64
  Hl, Hr = S.halo_frames(hp, denoise)
  raws, dens = [], []
  for p in S.plan_stream(T, C, Hl, Hr, closed=True):
    cols = slice(32 * p.w0, 32 * p.w1)
    a = _infer(sd, mel[:, :, p.w0:p.w1], z_init[:, :, cols], {k: v[:, :, cols] for k, v in z_early.items()}, hp)
    raws.append(a[:, p.offset:p.offset + p.count])
    if denoise:
      d = stft_oracle.denoise(a.numpy(), bias, 0.1, fwd, inv, wsq)
      dens.append(d[:, p.offset:p.offset + p.count])
  got = torch.cat(raws, dim=1)
  assert got.shape == raw.shape
  assert float((got - raw).abs().max()) <= 1e-12 * float(raw.abs().max())
  if denoise:
    got = np.concatenate(dens, axis=1)
    assert got.shape == den.shape
    assert np.abs(got - den).max() <= 1e-12 * np.abs(den).max()
