"""GPU: the device-resident training data path (waveglow_amd/device_data.py).  wg_data_gather against its numpy
restatement without a tolerance, the batched mel call against single calls, DeviceBatchLoader against
DataLoader(MelLoader) batch by batch, and train(device_dataset=True) against train()."""
import ctypes as C
import random
from pathlib import Path

import numpy as np
import pytest
import torch
from scipy.io.wavfile import write as write_wav

from _device_data_ref import gather_ref

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
SR = 22050


# ---------------------------------------------------------------- 1. the gather kernel
POOL_LENS = [1031, 520, 519, 4097, 1]
# (utterance, start): start 0, odd starts, the last valid start, a short utterance, one of exactly the segment, the
# first and the last utterance of the pool (whose row ends on the pool's last element)
VALID = {520: [(0, 0), (0, 1), (0, 256), (0, 511), (1, 0), (2, 0), (3, 0), (3, 1001), (3, 3577), (4, 0)],
         4096: [(3, 0), (3, 1), (0, 0), (1, 0), (2, 0), (4, 0)]}
# one row per kind: utterance below / above the range, negative start, start behind the last valid one of a long, an
# exact and a short utterance
INVALID = {520: [(-1, 0), (5, 0), (0, -1), (0, 512), (1, 1), (2, 1), (4, 1)],
           4096: [(-1, 0), (5, 0), (3, -1), (3, 2), (0, 1)]}


def _pool(dtype):
  rng = np.random.default_rng(11)
  if dtype == np.int16:
    wavs = [rng.integers(-32768, 32768, size=n, dtype=np.int64).astype(np.int16) for n in POOL_LENS]
    lo, hi = -32768, 32767
  else:
    wavs = [rng.uniform(-1.0, 1.0, size=n).astype(np.float32) for n in POOL_LENS]
    lo, hi = -1.0, 1.0
  wavs[0][[0, 1, 1030]] = (lo, hi, hi)
  wavs[1][[0, 519]] = (hi, lo)
  wavs[3][[1, 4096]] = (hi, lo)
  wavs[4][0] = lo
  return np.concatenate(wavs), np.concatenate([[0], np.cumsum(POOL_LENS)]).astype(np.int64)


def _gather(pool, offsets, picks, seg, status_init=0, with_status=True):
  from waveglow_amd import _lib
  lib = _lib.load()
  code = _lib.WG_PCM_I16 if pool.dtype == np.int16 else _lib.WG_PCM_F32
  d_pool, d_off = torch.from_numpy(pool).to(DEV), torch.from_numpy(offsets).to(DEV)
  d_picks = torch.tensor(picks, dtype=torch.int32).reshape(-1, 2).to(DEV)
  out = torch.full((len(picks), seg), float("nan"), dtype=torch.float32, device=DEV)
  status = torch.full((1,), status_init, dtype=torch.int32, device=DEV)
  stream = torch.cuda.current_stream(DEV).cuda_stream
  _lib.check(lib.wg_data_gather(d_pool.data_ptr(), code, pool.size, d_off.data_ptr(), len(offsets) - 1,
                                d_picks.data_ptr(), out.data_ptr(), status.data_ptr() if with_status else None,
                                len(picks), seg, C.c_void_p(stream)))
  torch.cuda.synchronize()
  return out.cpu().numpy(), int(status.item())


def _same_bits(a, b):
  return a.shape == b.shape and np.array_equal(a.view(np.int32), b.view(np.int32))


@pytest.mark.parametrize("dtype", [np.int16, np.float32], ids=["int16", "fp32"])
@pytest.mark.parametrize("seg", [520, 4096])
def test_gather_is_its_numpy_restatement_bit_for_bit(dtype, seg):
  pool, offsets = _pool(dtype)
  valid, invalid = VALID[seg], INVALID[seg]
  # valid picks only: status stays 0
  ref, ref_status = gather_ref(pool, offsets, valid, seg)
  out, status = _gather(pool, offsets, valid, seg)
  assert ref_status == 0 and status == 0
  assert _same_bits(out, ref)
  ext = (-1.0, 32767 / 32768) if dtype == np.int16 else (-1.0, 1.0)
  assert out.min() == ext[0] and out.max() == ext[1]
  # valid and invalid rows interleaved: the invalid ones are zero, the others untouched by them, status 1
  mixed = [p for pair in zip(invalid, valid) for p in pair] + invalid[len(valid):] + valid[len(invalid):]
  ref, ref_status = gather_ref(pool, offsets, mixed, seg)
  out, status = _gather(pool, offsets, mixed, seg)
  assert ref_status == 1 and status == 1
  assert _same_bits(out, ref)
  for b, p in enumerate(mixed):
    if p in invalid:
      assert not out[b].any()
  # every kind of invalid pick sets the flag on its own; without a status pointer the rows are still zero
  for p in invalid:
    out, status = _gather(pool, offsets, [p], seg)
    assert status == 1 and not out.any(), p
  out, status = _gather(pool, offsets, invalid, seg, status_init=7, with_status=False)
  assert status == 7 and not out.any()


# ---------------------------------------------------------------- 2. one batched mel call for B single ones
def test_batched_mel_is_the_single_calls_bit_for_bit():
  from waveglow_amd.hparams import HParams
  from waveglow_amd.taco_stft import TacotronSTFT
  st = TacotronSTFT(HParams(), DEV)
  x = torch.from_numpy(np.random.default_rng(2).uniform(-0.9, 0.9, size=(3, 4096)).astype(np.float32)).to(DEV)
  x[1, 1000:] = 0.0                                                  # a zero-padded row, as a short utterance gives
  batched = st._mel(x)
  assert batched.shape == (3, 80, 17)
  for b in range(3):
    assert torch.equal(batched[b], st._mel(x[b:b + 1].contiguous())[0]), b


# ---------------------------------------------------------------- 3. loader equality
SEG = 4096
TRAIN_LENS = [6001, 4096, 3000, 9000, 5001, 4097, 7000]              # one exactly the segment, one shorter
VAL_LENS = [4500, 700, 8000]


def _write_folder(folder: Path, lens, seed, float_at=None):
  folder.mkdir(parents=True, exist_ok=True)
  rng = np.random.default_rng(seed)
  for i, n in enumerate(lens):
    data = rng.integers(-32768, 32768, size=n, dtype=np.int64).astype(np.int16)
    if i == float_at:
      data = (data.astype(np.float32) / np.float32(40000))           # an fp32 wav: forces the fp32 pool
    write_wav(folder / f"utt_{i}.wav", SR, data)


def _hp():
  from waveglow_amd.hparams import HParams
  return HParams(batch_size=2, segment_length=SEG)


def _cpu(batch):
  return tuple(t.cpu() for t in batch)


def _legacy_walk(trn, val, interleave):
  """Two epochs of the legacy loaders: [(mel, audio), ...] on the host.  ``interleave``: a full validation pass after
  every second train batch, the order train() gives; otherwise ``trn`` alone (``val`` is None)."""
  out = []
  for _ in range(2):
    for k, batch in enumerate(trn):
      out.append(_cpu(batch))
      if interleave and k % 2 == 1:
        out.extend(_cpu(b) for b in val)
  return out


@pytest.fixture(scope="module", params=["int16", "fp32"])
def folders(request, tmp_path_factory):
  """Wav folders of one variant and the legacy loaders' batches over them, computed once."""
  from waveglow_amd.training import load_dataset, prepare_trainloader, prepare_valloader
  root = tmp_path_factory.mktemp(f"wavs_{request.param}")
  _write_folder(root / "trn", TRAIN_LENS, 21, float_at=2 if request.param == "fp32" else None)
  _write_folder(root / "val", VAL_LENS, 22)
  trn, val = load_dataset(root / "trn"), load_dataset(root / "val")
  hp = _hp()
  legacy = {
    "drop": _legacy_walk(prepare_trainloader(hp, trn, DEV), None, False),
    "keep": _legacy_walk(prepare_valloader(hp, trn, DEV), None, False),
  }
  trn_loader = prepare_trainloader(hp, trn, DEV)                      # train first, validation second, as train() does
  legacy["train_order"] = _legacy_walk(trn_loader, prepare_valloader(hp, val, DEV), True)
  return dict(variant=request.param, trn=trn, val=val, legacy=legacy)


def _assert_same(ours, legacy):
  assert len(ours) == len(legacy)
  for k, ((mel, audio), (mel_l, audio_l)) in enumerate(zip(ours, legacy)):
    assert mel.dtype == audio.dtype == torch.float32
    assert audio.shape == audio_l.shape and mel.shape == mel_l.shape == (audio.shape[0], 80, SEG // 256 + 1), k
    assert torch.equal(audio, audio_l), k
    assert torch.equal(mel, mel_l), k


@pytest.mark.parametrize("prefetch", [False, True], ids=["plain", "prefetch"])
def test_loader_yields_the_legacy_batches(folders, prefetch):
  from waveglow_amd.device_data import DeviceBatchLoader
  loader = DeviceBatchLoader(folders["trn"], _hp(), DEV, drop_last=True)
  assert loader.pool.is_int16 == (folders["variant"] == "int16")
  assert len(loader) == 3
  ours = []
  for epoch in range(2):
    for k, batch in loader.epoch():
      assert batch[0].device.type == "cuda" and batch[1].device.type == "cuda"
      if prefetch and not (epoch == 1 and k == 2):                    # across the epoch boundary, not past the last one
        loader.prefetch()
      ours.append(_cpu(batch))
  loader.check_status(sync=True)
  _assert_same(ours, folders["legacy"]["drop"])


def test_loader_without_drop_last_ends_on_the_partial_batch(folders):
  from waveglow_amd.device_data import DeviceBatchLoader
  loader = DeviceBatchLoader(folders["trn"], _hp(), DEV, drop_last=False)
  assert len(loader) == 4
  ours = [_cpu(b) for _ in range(2) for b in loader]
  assert ours[3][1].shape == (1, SEG)
  loader.check_status(sync=True)
  _assert_same(ours, folders["legacy"]["keep"])


def test_loaders_in_the_order_of_train(folders):
  """Train and validation loaders interleaved as train() runs them, prefetching wherever no validation pass follows."""
  from waveglow_amd.device_data import DeviceBatchLoader
  trn = DeviceBatchLoader(folders["trn"], _hp(), DEV, drop_last=True)
  val = DeviceBatchLoader(folders["val"], _hp(), DEV, drop_last=False)
  ours = []
  for epoch in range(2):
    for k, batch in trn.epoch():
      ours.append(_cpu(batch))
      if k % 2 == 1:
        ours.extend(_cpu(b) for b in val)
      elif not (epoch == 1 and k == 2):
        trn.prefetch()
  trn.check_status(sync=True)
  val.check_status(sync=True)
  _assert_same(ours, folders["legacy"]["train_order"])


def test_a_bad_pick_raises_where_the_status_is_read(folders):
  from waveglow_amd._lib import WgError
  from waveglow_amd.device_data import DeviceBatchLoader
  loader = DeviceBatchLoader(folders["trn"], _hp(), DEV, drop_last=True)
  loader.check_status(sync=True)
  mel, audio = loader._enqueue([(0, 0), (len(TRAIN_LENS), 0)])
  assert not audio[1].any()
  with pytest.raises(WgError):
    loader.check_status(sync=True)


# ---------------------------------------------------------------- 4. train(device_dataset=True) against train()
CUSTOM = {"n_channels": "64", "n_layers": "3", "n_flows": "4", "n_early_every": "2", "batch_size": "2",
          "segment_length": "4096", "epochs": "2", "iters_per_checkpoint": "2", "learning_rate": "0.001"}


def _bound(legacy, again):
  """Per step: max(4 fp32 ulps of the legacy loss, 2 x |legacy - second legacy run|)."""
  return [max(4 * float(np.spacing(np.float32(abs(a)))), 2 * abs(a - b)) for a, b in zip(legacy, again)]


@pytest.fixture(scope="module")
def runs(tmp_path_factory):
  """The legacy path twice and the device path once over the same folders, each with its own checkpoint folder; then a
  resume from iteration 4 (the middle of an epoch: one batch is skipped) for each."""
  from waveglow_amd.checkpoint import CheckpointWaveglow
  from waveglow_amd.training import get_all_checkpoint_iterations, get_pytorch_filename, load_dataset, train
  root = tmp_path_factory.mktemp("train_ab")
  rng = np.random.default_rng(1)
  for name, n in (("trn", 6), ("val", 2)):
    (root / name).mkdir()
    for i in range(n):
      write_wav(root / name / f"random_audio_{i + 1}.wav", SR,
                np.int16(rng.uniform(-1.0, 1.0, size=int(0.6 * SR)) * 32767))
  trn, val = load_dataset(root / "trn"), load_dataset(root / "val")
  res = {}
  for name, flag in (("legacy", False), ("again", False), ("device", True)):
    ckp = root / f"ckp_{name}"
    losses = train(dict(CUSTOM), None, trn, val, ckp, None, None, DEV, device_dataset=flag)
    its = get_all_checkpoint_iterations(ckp)
    ck = CheckpointWaveglow.load(ckp / get_pytorch_filename(4), DEV)
    more = train(None, None, trn, val, root / f"ckp_{name}_resumed", ck, None, DEV, device_dataset=flag)
    res[name] = dict(losses=losses, its=its, more=more,
                     more_its=get_all_checkpoint_iterations(root / f"ckp_{name}_resumed"))
  return res


def test_train_on_the_device_dataset_is_the_legacy_training(runs):
  legacy, again, device = runs["legacy"], runs["again"], runs["device"]
  assert len(legacy["losses"]) == len(device["losses"]) == 6
  assert device["its"] == legacy["its"] == [1, 2, 3, 4, 6]
  bound = _bound(legacy["losses"], again["losses"])
  for k, (a, b, d, tol) in enumerate(zip(legacy["losses"], again["losses"], device["losses"], bound)):
    print(f"step {k + 1}: legacy {a!r} again {b!r} device {d!r} |device - legacy| {abs(d - a):.3e} bound {tol:.3e}")
  for k, (a, d, tol) in enumerate(zip(legacy["losses"], device["losses"], bound)):
    assert abs(d - a) <= tol, (k, a, d, tol)


def test_resumed_training_on_the_device_dataset_continues_like_the_legacy_one(runs):
  legacy, again, device = runs["legacy"], runs["again"], runs["device"]
  assert len(legacy["more"]) == len(device["more"]) == 2              # iterations 5 and 6: batch 0 of the epoch is skipped
  assert device["more_its"] == legacy["more_its"] == [6]
  bound = _bound(legacy["more"], again["more"])
  for k, (a, b, d, tol) in enumerate(zip(legacy["more"], again["more"], device["more"], bound)):
    print(f"step {k + 5}: legacy {a!r} again {b!r} device {d!r} |device - legacy| {abs(d - a):.3e} bound {tol:.3e}")
  for k, (a, d, tol) in enumerate(zip(legacy["more"], device["more"], bound)):
    assert abs(d - a) <= tol, (k, a, d, tol)
