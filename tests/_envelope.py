"""The accepted size range of ``wg_infer`` / ``wg_forward`` in plain Python: a restatement of
``make_geom`` (waveglow_amd/csrc/wg_host.h) and of the one size check in front of it (``kMaxRowsPerPhase``), plus the
named shapes at the top of that range that tests/test_envelope_cpu.py and tests/test_gpu_envelope.py share.

A 64-channel chunk plane of the activation layout holds ``R * 128`` bytes; the call is accepted while that stays below
2^32, i.e. while ``Rp <= 2^20 - 128`` (DESIGN.md sections 2 and 8)."""
from __future__ import annotations

from typing import NamedTuple

PHASES = 32                      # group-timesteps per mel frame (upsample_stride / n_group)
ROW_PAD = 16                     # slack rows in front of / behind every plane
MAX_RP = (1 << 20) - 128         # 1 048 448: the last Rp with R * 128 < 2^32


def guard_frames(n_layers: int) -> int:
  """Zero guard frames each side of an utterance: 4 up to 8 layers, 8 / 16 for 9 / 10."""
  return max(4, (PHASES - 1 + (1 << (n_layers - 1))) // PHASES)


class Geom(NamedTuple):
  B: int
  T: int
  L: int            # group-timesteps per utterance
  Fp: int           # rows per utterance and phase
  Rp: int           # rows per phase block
  R: int            # rows of a plane
  plane_bytes: int  # R * 128: one 64-channel chunk of fp16
  state_elems: int  # B * L * 8: the [B*L][8] flow state / audio

  @property
  def accepted(self) -> bool:
    return self.plane_bytes < (1 << 32)


def geom(B: int, T: int, n_layers: int = 8, L: int | None = None) -> Geom:
  """``make_geom`` for an inference call of B utterances x T mel frames (L = 32 T), or a forward call with L = audio_len / 8."""
  if L is None:
    L = PHASES * T
  F = -(-L // PHASES)
  Fp = F + 2 * guard_frames(n_layers)
  Rp = -(-(B * Fp) // 128) * 128
  R = PHASES * Rp + 2 * ROW_PAD
  return Geom(B, T, L, Fp, Rp, R, R * 128, B * L * 8)


class Shape(NamedTuple):
  B: int
  T: int
  Rp: int           # expected rows per phase block (8 layers, Gf = 4)
  side: str         # "cross": plane bytes just over 2^31; "top": the last accepted; "over": the first refused


SHAPES = {
  "wide_cross": Shape(8193, 56, 524416, "cross"),      # B * Fp = 524 352 rounds up to 524 416: padding rows are part of the case
  "wide_top": Shape(16382, 56, 1048448, "top"),
  "long_cross": Shape(4, 131072, 524416, "cross"),
  "long_top": Shape(4, 262104, 1048448, "top"),
  "wide_over": Shape(16383, 56, 1048576, "over"),
  "long_over": Shape(4, 262136, 1048576, "over"),
}
ACCEPTED = [n for n, s in SHAPES.items() if s.side != "over"]
REFUSED = [n for n, s in SHAPES.items() if s.side == "over"]

LONG_FRAMES = lambda T: [37, 864, 4000, T]      # per-utterance mel frames of the long shapes
