"""CPU: the case table, the inputs, the yardsticks and the sensitivity of the per-cell and per-sample statistics of
tests/_loss_cells.py (the GPU side is tests/test_gpu_loss_cells.py).

The sensitivity test plants five defects into restatement (b) -- no library code involved -- and asserts that the new
statistic exceeds 4 Y for each; for each it prints whether the scalar bound and the per-utterance L2 bound of the existing
loss tests would have caught it, which puts the gap on record.
"""
import ctypes as C

import pytest
import torch

import _loss_cells as L
import _mel_loss_oracle as O
from waveglow_amd import _lib, build

F4 = L.BOUND_FACTOR


@pytest.mark.parametrize("sid", list(L.EXPECT))
def test_case_table_matches_the_geometry_arithmetic(sid):
  g = L.geometry(L.SCALES[sid])
  got = (g["MTf"], g["nbyf"], g["TWf"], g["MTb"], g["nbyb"], g["TWb"], g["lpad"])
  assert got == L.EXPECT[sid], (sid, got)
  n_fft, hop, win, n_mels = L.SCALES[sid]
  assert n_fft % 32 == 0 and 1 <= win <= n_fft and 1 <= n_mels <= n_fft // 2 + 1
  for leg in "fb":
    r = g["m" + leg]
    assert r[0][0] == 0 and r[-1][1] == g["MT" + leg] and all(a[1] == b[0] for a, b in zip(r, r[1:]))
    assert max(m1 - m0 for m0, m1 in r) <= 4 * L.K_TW and L.ceil_div(max(m1 - m0 for m0, m1 in r), 4) == g["TW" + leg]
  if sid == "g544":
    assert g["mf"] == L.G544_RANGES and g["mb"] == L.G544_RANGES
    assert L.owner(8 * 32 - 1, 17, 2) == 0 and L.owner(8 * 32, 17, 2) == 1
  if sid in ("g160", "g544"):
    assert win % 32 != 0 and g["lpad"] > 0
  # the four instances and both uneven deals are reached: a wave without a tile, a repeated tile, an uneven split
  assert {v[2] for v in L.EXPECT.values()} == {1, 2, 3, 4}


@pytest.mark.parametrize("name", list(L.CASES))
def test_frame_counts_and_lengths(name):
  c = L.case(name)
  assert [c.F(i) for i in range(len(c.scales))] == (L.EXPECT_F[name] if name not in L.BANK_CASES else [65])
  for i, s in enumerate(c.scales):
    assert c.F(i) == c.N // s[1] + 1 and c.Fp(i) % L.K_BN == 0 and 0 <= c.Fp(i) - c.F(i) < L.K_BN
  assert all(c.min_len() <= n <= c.N for n in c.lens)
  if name in L.EXPECT_FB:
    assert c.Fb(0) == L.EXPECT_FB[name] and min(c.lens) == c.min_len() and max(c.lens) == c.N
  if name == "full64":
    assert c.F(0) == c.Fp(0) == 64
  if name == "g64":
    assert c.F(0) % 64 == 1                                  # the last tile holds one frame
  if name == "g64r":
    assert c.Fb(0)[1] == 64                                  # fills its first tile, leaves the other two without work


@pytest.fixture(scope="module")
def lib():
  build.build_library()
  return _lib.load()


def test_layout_is_the_librarys(lib):
  """``layout`` (written from the header's text) gives the sizes a planning handle reports."""
  for name in L.CASES:
    c = L.case(name)
    arr = lambda v: (C.c_int32 * len(v))(*v)
    h = C.c_void_p()
    assert lib.wg_melloss_create(len(c.scales), *(arr(col) for col in zip(*c.scales)), None, None, 1e-5, -1, C.byref(h)) == 0
    spec, mel, tail, ns, nm = L.layout(c.scales, c.B, c.N)
    assert lib.wg_melloss_spectra_elems(h, c.B, c.N) == ns and lib.wg_melloss_mels_elems(h, c.B, c.N) == nm, name
    assert tail == nm - 64 and all(at % 64 == 0 for at, _ in spec) and all(ax % 64 == 0 and ay % 64 == 0 for ax, ay, _ in mel)
    ms, mm = L.written_mask(c.scales, c.B, c.N, c.lens)
    assert int(ms.sum()) == sum(s[0] * sum(c.Fb(i)) for i, s in enumerate(c.scales))
    assert int(mm.sum()) == 16 + 2 * sum(s[3] * sum(c.Fb(i)) for i, s in enumerate(c.scales))
    assert lib.wg_melloss_destroy(h) == 0


def test_deinterleave_follows_the_header():
  """Against (b) arranged by hand for g32: row 0 = re of bin 0, row 1 = re of bin 16, rows 2p, 2p + 1 = (re, im) of bin p."""
  c = L.case("g32")
  n_fft, hop, win, _ = c.scales[0]
  x = c.plane_inputs()[0][:1]
  re, im = (t[0] for t in O.spec_unfold(x, n_fft, hop, win, torch.float64))
  rows = torch.stack([re[0], re[16]] + [t[p] for p in range(1, 16) for t in (re, im)])
  assert rows.shape == (32, c.F(0))
  r2, i2 = L.deinterleave(rows)
  im_ref = im.clone()
  im_ref[0] = im_ref[16] = 0.0
  assert torch.equal(r2, re) and torch.equal(i2, im_ref)
  assert torch.equal(L.interleave(re, im), rows)
  assert [L.row_of(0, 0, 32), L.row_of(0, 16, 32), L.row_of(0, 3, 32), L.row_of(1, 3, 32)] == [0, 1, 6, 7]
  assert float(im[0].abs().max()) < 1e-12 and float(im[16].abs().max()) < 1e-12      # what the layout leaves out is zero


@pytest.mark.parametrize("name", list(L.CASES))
def test_inputs_qualify(name):
  """Draw 0 of every gradient comparison of the GPU tests: no fragile cell or bin on the frames that matter; and a local
  difference leaves (a)'s gradient exactly zero outside its support and non-zero inside."""
  c = L.case(name)
  if name in L.BANK_CASES:                                   # mel cells only: they ask nothing of their inputs
    W = c.banks()[0]
    assert (name == "empty256") == bool((W.abs().sum(1) == 0).sum() >= 2) and (name == "dense256") == bool((W < 0).any())
    return
  assert L.qualifies(c, c.seed(0, None))
  if len(c.scales) > 1:
    return
  for where, ivs in c.intervals().items():
    assert L.qualifies(c, c.seed(0, where), where), where
    sup = c.support(where)
    for loss, term in L.LOCAL_TERMS:
      g = L.ref_grad(name, loss, term, where)
      assert not g[~sup].any() and torch.isfinite(g).all(), (where, loss)
      for b, iv in enumerate(ivs):
        if iv is None:
          assert not g[b].any() and not sup[b].any()
        else:
          assert g[b, iv[0]:iv[1]].any() and sup[b, iv[0]:iv[1]].all() and len(c.touching(where)[b]) >= 1
          print(f"{name} {where} {loss} utterance {b}: interval {iv}, frames {c.touching(where)[b].tolist()}, "
                f"{int(sup[b].sum())} samples of support")
  assert "seam64" in c.intervals() or name == "full64"
  assert ("seam128" in c.intervals()) == (name in ("g32", "g64", "g64r"))


@pytest.mark.parametrize("name", list(L.CASES))
def test_yardsticks(name):
  """Finite and positive; (b) in fp64 -- the rounding of the basis to fp32 alone -- at most a quarter of Y (measured 7 to
  30 times below); (b) and (c) in fp32 inside the derived cap (measured: 0.1 % to 10 % of it)."""
  c = L.case(name)
  for i, s in enumerate(c.scales):
    yb, yc, ym = L.yard_rows(name, i, "b"), L.yard_rows(name, i, "c"), L.yard_mels(name, i)
    x = c.plane_inputs()[0]
    ref, cap = L.ref_rows(name, i), L.ref_cap(name, i)
    b64 = L.cell_stat(L.rows_b(s, x, c.lens, torch.float64), ref)[0]
    use = [max(float(((g.double() - r).abs() / k.clamp_min(1e-300)).max()) for g, r, k in zip(fn(s, x, c.lens), ref, cap))
           for fn in (L.rows_b, L.rows_c32)]
    print(f"{name} scale {s}: rows Y (b) {yb:.2e}, (c) {yc:.2e}, (b) in fp64 {b64:.2e}; (b), (c) use {use[0]:.4f}, {use[1]:.4f} "
          f"of the cap; mels Y {ym:.2e}")
    for y in (yb, yc, ym):
      assert 0.0 < y < 1e-3 and y == y
    assert b64 <= yb / 4
    assert max(use) <= 1.0
  if name in L.SINGLE:
    for loss, term in (("mel", "both"), ("stft", "sc")):
      y = L.yard_grad(name, loss, term)
      print(f"{name} {loss} {term}: gradient Y {y:.2e}, (b) per-utterance L2 {L.l2_b32(name, loss, term)}")
      assert 0.0 < y < 1e-2


# ---------------------------------------------------------------- sensitivity
SENS_CASES = ["g64", "g2048"]     # the smallest case with a frame 64 and the largest: the larger, the more the old bounds dilute
BIN, MEL_ROW = 5, 4


def _planted(fault):
  """Restatement (b)'s transform with one defect."""

  def spec(x, n_fft, hop, win, dtype):
    if fault == "reflect":                                  # the right edge reflected about N instead of N - 1
      n = x.shape[1]
      p = torch.arange(L.frames_of(n, hop))[:, None] * hop + torch.arange(n_fft)[None, :] - n_fft // 2
      p = p.abs()
      p = torch.where(p >= n, (2 * n - p).clamp(max=n - 1), p)
      fr = x.to(dtype)[:, p]
    else:
      fr = O.frames_unfold(x, n_fft, hop, dtype)
    if fault == "tap" and fr.shape[1] > 64:                 # one tap dropped in frame 64
      keep = torch.ones(fr.shape[1:], dtype=dtype)
      keep[64, n_fft // 2 + 3] = 0.0
      fr = fr * keep
    if fault == "ola" and fr.requires_grad and fr.shape[1] > 64:      # frame 64 left out of the overlap-add
      keep = torch.ones(fr.shape[1:], dtype=dtype)
      keep[64] = 0.0
      fr.register_hook(lambda g: g * keep)
    re, im = O.spec_of_frames(fr, n_fft, win)
    if fault == "swap":                                     # rows 2p and 2p + 1 exchanged for one bin
      re, im = re.clone(), im.clone()
      re[:, BIN], im[:, BIN] = im[:, BIN].clone(), re[:, BIN].clone()
    return re, im

  return spec


def _short_span(W):
  """Row MEL_ROW's span one bin short."""
  W = W.clone()
  W[MEL_ROW, int(torch.nonzero(W[MEL_ROW]).max())] = 0.0
  return W


@pytest.mark.parametrize("SENS", SENS_CASES)
@pytest.mark.parametrize("fault", ["tap", "reflect", "ola", "swap", "span"])
def test_statistic_sees_planted_defects(fault, SENS):
  c = L.case(SENS)
  s = c.scales[0]
  W = O.bank(s)
  x, y = c.inputs()
  spec = _planted(fault)
  mag = lambda *a: O._root(sum(t ** 2 for t in spec(*a)))                   # noqa: E731
  Wf = _short_span(W) if fault == "span" else W
  # the new statistic
  if fault in ("tap", "reflect", "swap"):
    xs = c.plane_inputs()[0]
    stat, pos = L.cell_stat(L.rows_of(spec, s, xs, c.lens, torch.float32), L.ref_rows(SENS))
    yard, what = L.yard_rows(SENS), "transform rows: " + L.describe_cell(pos, L.geometry(s)["MTf"])
    if fault in ("tap", "swap"):
      assert pos[2] == 64 if fault == "tap" else pos[1] in (2 * BIN, 2 * BIN + 1)
    else:
      assert pos[3] <= 2                                    # within the frames that reach past the end
  elif fault == "span":
    xs = c.plane_inputs()[0]
    stat, pos = L.cell_stat(L.mels_of(O.mag_unfold, s, Wf, xs, c.lens, torch.float32),
                            L.mels_of(O.mag_stft, s, W, xs, c.lens, torch.float64))
    yard, what = L.yard_mels(SENS), "mels: " + L.describe_cell(pos)
    assert pos[1] == MEL_ROW
  else:
    g = O.grad_of(lambda *a, **k: O._loss(mag, *a, **k), x, y, c.scales, banks=[W], clamp=O.CLAMP, factor_log=1.0, factor_lin=1.0,
                  lengths=None, dtype=torch.float32)
    stat, pos = L.sample_stat(g, L.ref_grad(SENS, "mel", "both"), c.lens, s[1])
    yard, what = L.yard_grad(SENS, "mel", "both"), "gradient: " + L.describe_sample(pos)
    assert abs(pos[1] - 64 * s[1]) <= s[0] // 2
  # what the existing bounds see: the scalars under min(max(4 e32, 1e-6), 1e-5), the gradient under max(4 g32, 1e-6) per utterance
  kw = dict(banks=[Wf], clamp=O.CLAMP, factor_log=1.0, factor_lin=1.0, lengths=None, dtype=torch.float32)
  a = [float(v) for v in O.loss_stft(x, y, c.scales, factor_lin=1.0)]
  e32 = [float(v) for v in O.loss_unfold(x, y, c.scales, factor_lin=1.0, dtype=torch.float32)]
  bad = [float(v) for v in O._loss(mag, x, y, c.scales, **kw)]
  scalar = any(abs(g - r) / abs(r) > min(max(F4 * abs(e - r) / abs(r), 1e-6), 1e-5) for g, r, e in zip(bad, a, e32))
  gbad = O.grad_of(lambda *a, **k: O._loss(mag, *a, **k), x, y, c.scales, **kw)
  l2 = L.l2_per_utterance(gbad, L.ref_grad(SENS, "mel", "both"), c.lens)
  l2_caught = any(e > max(F4 * g32, L.L2_FLOOR) for e, g32 in zip(l2, L.l2_b32(SENS, "mel", "both")))
  print(f"{SENS} {fault}: statistic {stat:.3e} against 4 Y = {F4 * yard:.3e} ({stat / yard:.0f} Y) at {what}; the scalar bound would "
        f"{'' if scalar else 'NOT '}have caught it (worst relative error {max(abs(g - r) / abs(r) for g, r in zip(bad, a)):.1e}), the "
        f"per-utterance L2 bound would {'' if l2_caught else 'NOT '}have (worst {max(l2):.1e})")
  assert stat > F4 * yard
