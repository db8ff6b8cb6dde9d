"""The size range of the inference and no-grad-forward calls, without a GPU: tests/_envelope.py restates make_geom; here
its named shapes are placed against 2^31 and 2^32, and the library's own answer (the workspace queries are pure host
arithmetic and return 0 for a call that would be refused) is compared with the restatement at every edge."""
import ctypes as C

import pytest

import _envelope as E
from waveglow_amd import _lib, build


@pytest.mark.parametrize("name", list(E.SHAPES))
def test_named_shapes_lie_where_they_are_meant_to(name):
  s = E.SHAPES[name]
  g = E.geom(s.B, s.T)
  assert g.Fp == s.T + 8 and g.Rp == s.Rp and g.R == 32 * g.Rp + 32
  assert g.state_elems < 2 ** 31                    # the [B*L][8] state never binds: the plane limit does
  if s.side == "cross":
    assert 2 ** 31 < g.plane_bytes < 2 ** 31 + 2 ** 20 and g.accepted      # just over 2^31
  elif s.side == "top":
    assert g.Rp == E.MAX_RP and g.plane_bytes == 2 ** 32 - 520192 and g.accepted
  else:
    assert g.plane_bytes >= 2 ** 32 and not g.accepted
    assert g.Rp == E.MAX_RP + 128                                           # the first refused step


def test_wide_cross_rounds_up_into_padding_rows():
  s = E.SHAPES["wide_cross"]
  assert s.B * (s.T + 8) == 524352 and 524352 % 128 == 64 and E.geom(s.B, s.T).Rp == 524416


def test_refused_shapes_are_the_first_refused():
  w, l = E.SHAPES["wide_over"], E.SHAPES["long_over"]
  assert E.geom(w.B - 1, w.T).accepted and (w.B - 1, w.T) == E.SHAPES["wide_top"][:2]      # one utterance fewer
  assert E.geom(l.B, l.T - 32).accepted and (l.B, l.T - 32) == E.SHAPES["long_top"][:2]    # one 128-row step less
  assert not E.geom(l.B, l.T - 31).accepted                                                 # ... and not a row sooner
  assert not E.geom(w.B, w.T).accepted and not E.geom(l.B, l.T).accepted


@pytest.mark.parametrize("n_layers,guard", [(1, 4), (8, 4), (9, 8), (10, 16)])
def test_guard_frames(n_layers, guard):
  assert E.guard_frames(n_layers) == guard
  assert E.geom(3, 5, n_layers).Fp == 5 + 2 * guard


def _limit_T(B, n_layers):
  """Largest T with B * (T + 2 Gf) <= MAX_RP."""
  return E.MAX_RP // B - 2 * E.guard_frames(n_layers)


@pytest.fixture(scope="module")
def lib():
  build.build_library()
  return _lib.load()


@pytest.mark.parametrize("channels", [64, 128, 256, 512])
@pytest.mark.parametrize("n_layers", [8, 9, 10])
def test_library_refuses_exactly_outside_the_restated_range(lib, channels, n_layers):
  """wg_infer_workspace_bytes / wg_forward_workspace_bytes: a size for the last accepted geometry, 0 and a message that
  names the limit for the first refused one, at every width and guard size -- and the same line as tests/_envelope.py."""
  cfg = _lib.WgConfig(80, 4, 8, 2, 2, n_layers, channels, 3, 1024, 256)
  h = C.c_void_p()
  assert lib.wg_create(C.byref(cfg), 0, C.byref(h)) == 0
  try:
    cases = [(s.B, s.T) for s in E.SHAPES.values()] if n_layers == 8 else []
    for B in (1, 4, 1200, 16382):
      T = _limit_T(B, n_layers)
      cases += [(B, T), (B, T + 1), (B + 1, T)]
    cases += [(2 ** 31 - 1, 1), (1, 2 ** 22), (130150525, 1)]     # far outside: the check itself must not overflow
    for B, T in cases:
      g = E.geom(B, T, n_layers)
      for n in (lib.wg_infer_workspace_bytes(h, B, T), lib.wg_forward_workspace_bytes(h, B, T, 256 * T)):
        if g.accepted:
          # two x planes, the a0 plane, Z and OUT at least
          assert n >= 2 * (channels // 64) * g.plane_bytes + g.plane_bytes + 2 * 4 * g.state_elems, (B, T)
        else:
          assert n == 0, (B, T)
          msg = lib.wg_last_error().decode()
          assert "batch too large" in msg and str(E.MAX_RP) in msg and "4 GiB" in msg, msg
    # forward with one group-timestep per utterance: L = 1, one frame
    B = E.MAX_RP // (1 + 2 * E.guard_frames(n_layers))
    assert lib.wg_forward_workspace_bytes(h, B, 1, 8) > 0
    assert not E.geom(B + 1, 1, n_layers, L=1).accepted and lib.wg_forward_workspace_bytes(h, B + 1, 1, 8) == 0
  finally:
    lib.wg_destroy(h)
