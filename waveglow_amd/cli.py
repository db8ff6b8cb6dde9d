"""``waveglow-cli synthesize`` with the reference's flags and file conventions
(src/waveglow_cli/inference_v2.py:53-130, helper.py:8-22, defaults.py:9-10), plus real batching (the reference's
commented-out ``--batch-size``, inference_v2.py:64) and per-rank sharding of the file list under torch.distributed.run.

  python -m waveglow_amd.cli synthesize CHECKPOINT FOLDER [--sigma S] [--denoiser-strength D] [--device cuda:0]
         [--custom-hparams a=1,b=2] [--custom-seed N] [-out DIR] [-o] [--batch-size B] [--output-sampling-rate R]
         --output-sampling-rate: the synthesis is resampled to R Hz on the device (waveglow_amd/resample.py)
  python -m waveglow_amd.cli synthesize-wav CHECKPOINT FOLDER [same flags]   wav -> mel (HIP front-end) -> wav
         (src/waveglow_cli/inference_wav.py:74-130; copy synthesis)  [--resample-inputs]: wavs of any sampling rate
         (also on validate, train and continue-train): resampled to the model's rate on the device
  python -m waveglow_amd.cli train TRAIN-FOLDER VAL-FOLDER CHECKPOINTS-FOLDER [--device cuda:0] [--custom-hparams ...]
         [--pre-trained-model CKPT --warm-start] [--device-dataset]  (src/waveglow_cli/training.py:24-79)
  python -m waveglow_amd.cli continue-train TRAIN-FOLDER VAL-FOLDER CHECKPOINTS-FOLDER [...]   (training.py:82-124)
         --device-dataset: all wavs stay on the device and every batch is built there (waveglow_amd/device_data.py)
  python -m waveglow_amd.cli validate CHECKPOINTS-FOLDER OUTPUT-FOLDER DATA-FOLDER [--sigma S] [--denoiser-strength D]
         [--device cuda:0] [--custom-hparams ...] [--full-run] [--files NAME ...] [--custom-checkpoints IT ...]
         [--custom-seed N] [--batch-size B] [--pitch-metrics] [--intelligibility-metrics] [--likelihood]
         (src/waveglow_cli/validation.py:86-153)
         copy synthesis of validation utterances and their metrics on the device (MCD, DTW-MCD, penalties, cosine
         similarity): OUTPUT-FOLDER/log.txt, total.csv and one folder of mels and wavs per utterance and checkpoint;
         no PNG plots and no structural similarity, single process only.  --pitch-metrics adds the F0 RMSE, the gross
         pitch error and the voicing decision error between the original and the synthesis (a YIN tracker on the device);
         --intelligibility-metrics adds STOI and ESTOI of the two, resampled to 10 kHz on the device;
         --likelihood adds what the checkpoint assigns to the ORIGINAL wav: negative log-likelihood in nats per sample (the
         training loss of that utterance alone, at hparams.sigma), bits per sample and the variance of z
Under ``python -m torch.distributed.run`` the training commands run data-parallel (one process per GPU, RCCL).
"""
from __future__ import annotations

import argparse
import os
import random
import sys
from logging import getLogger
from pathlib import Path

import numpy as np
import torch
from scipy.io.wavfile import write as write_wav

from .audio import float_to_wav, normalize_wav
from .checkpoint import CheckpointWaveglow
from .hparams import split_hparams_string
from .sharding import shard_list
from .synthesizer import Synthesizer


def _unit_float(v: str) -> float:
  f = float(v)
  if not 0 <= f <= 1:
    raise argparse.ArgumentTypeError("Value needs to be in interval [0, 1]!")
  return f


def build_parser() -> argparse.ArgumentParser:
  p = argparse.ArgumentParser(prog="waveglow-cli")
  sub = p.add_subparsers(dest="command", required=True)
  for name, desc in (("synthesize", "Synthesize mel-spectrograms to audio files (.wav)."),
                     ("synthesize-wav", "Re-synthesize audio files: wav -> mel-spectrogram -> wav.")):
    s = sub.add_parser(name, description=desc)
    s.add_argument("checkpoint", type=Path, metavar="CHECKPOINT")
    s.add_argument("folder", type=Path, metavar="FOLDER")
    s.add_argument("--sigma", type=_unit_float, default=1.0)
    s.add_argument("--denoiser-strength", type=_unit_float, default=0.0005)
    s.add_argument("--device", type=str, default="cuda:0")
    s.add_argument("--custom-hparams", type=str, default=None)
    s.add_argument("--custom-seed", type=int, default=None)
    s.add_argument("-out", "--output-directory", type=Path, default=None)
    s.add_argument("-o", "--overwrite", action="store_true")
    s.add_argument("--batch-size", type=int, default=1,
                   help="utterances per launch sequence (ragged batch; results equal one-by-one synthesis)")
    s.add_argument("--output-sampling-rate", type=int, default=None, metavar="R",
                   help="resample the synthesis to R Hz on the device before it is normalised and written")
    if name == "synthesize-wav":
      s.add_argument("--resample-inputs", action="store_true",
                     help="resample wav files at other sampling rates to the model's on the device instead of refusing them")
  for name, desc in (("train", "Start training of a new model."), ("continue-train", "Continue training from the last checkpoint.")):
    t = sub.add_parser(name, description=desc)
    t.add_argument("train_folder", type=Path, metavar="TRAIN-FOLDER")
    t.add_argument("val_folder", type=Path, metavar="VAL-FOLDER")
    t.add_argument("checkpoints_dir", type=Path, metavar="CHECKPOINTS-FOLDER")
    t.add_argument("--device", type=str, default="cuda:0")
    t.add_argument("--custom-hparams", type=str, default=None)
    t.add_argument("--device-dataset", action="store_true",
                   help="keep all wavs on the device and build every batch there (same batches; cache_wavs is ignored)")
    t.add_argument("--resample-inputs", action="store_true",
                   help="resample wav files at other sampling rates to the model's on the device instead of refusing them")
    if name == "train":
      t.add_argument("--pre-trained-model", type=Path, default=None)
      t.add_argument("--warm-start", action="store_true")
  v = sub.add_parser("validate", description="Validate checkpoint(s) using the validation set or any other dataset.")
  v.add_argument("checkpoints_dir", type=Path, metavar="CHECKPOINTS-FOLDER")
  v.add_argument("output_dir", type=Path, metavar="OUTPUT-FOLDER")
  v.add_argument("dataset_dir", type=Path, metavar="DATA-FOLDER")
  v.add_argument("--sigma", type=_unit_float, default=1.0)
  v.add_argument("--denoiser-strength", type=_unit_float, default=0.0005)
  v.add_argument("--device", type=str, default="cuda:0")
  v.add_argument("--custom-hparams", type=str, default=None)
  v.add_argument("--full-run", action="store_true", help="validate all files in DATA-FOLDER")
  v.add_argument("--files", type=str, nargs="*", metavar="UTTERANCE", default=[],
                 help="names of utterances in DATA-FOLDER; if left unset a random utterance is chosen")
  v.add_argument("--custom-checkpoints", type=int, nargs="*", default=[],
                 help="validate the checkpoints of these iterations; if left unset the last one")
  v.add_argument("--custom-seed", type=int, default=None)
  v.add_argument("--batch-size", type=int, default=1,
                 help="utterances per launch sequence (ragged batch; results equal one-by-one validation)")
  v.add_argument("--pitch-metrics", action="store_true",
                 help="also track F0 of the original and the synthesis (YIN) and report F0 RMSE, gross pitch error and "
                      "voicing decision error in seven more columns")
  v.add_argument("--intelligibility-metrics", action="store_true",
                 help="also compute the short-time objective intelligibility of the synthesis against the original at "
                      "10 kHz (STOI and ESTOI) in four more columns")
  v.add_argument("--resample-inputs", action="store_true",
                 help="resample wav files at other sampling rates to the model's on the device instead of refusing them; "
                      "original.wav is still written as loaded")
  v.add_argument("--likelihood", action="store_true",
                 help="also score the original wav under each checkpoint (no sampling): negative log-likelihood per "
                      "sample, bits per sample and the variance of z over its whole frames, in four more columns")
  return p


def train_cmd(ns, resume: bool) -> bool:
  from .training import get_last_checkpoint, load_dataset, train
  rank, world = int(os.environ.get("RANK", "0")), int(os.environ.get("WORLD_SIZE", "1"))
  device = torch.device(ns.device if world == 1 else f"cuda:{int(os.environ.get('LOCAL_RANK', '0'))}")
  torch.cuda.set_device(device)
  if world > 1 and not torch.distributed.is_initialized():
    torch.distributed.init_process_group("nccl", device_id=device)
  for d in (ns.train_folder, ns.val_folder):
    if not d.is_dir():
      getLogger(__name__).error(f"{d} is not a directory!")
      return False
  checkpoint = warm = None
  if resume:
    checkpoint = CheckpointWaveglow.load(get_last_checkpoint(ns.checkpoints_dir)[0], device)
  elif ns.pre_trained_model is not None and ns.warm_start:
    warm = CheckpointWaveglow.load(ns.pre_trained_model, device)
  train(custom_hparams=split_hparams_string(ns.custom_hparams), logdir=None, trainset=load_dataset(ns.train_folder),
        valset=load_dataset(ns.val_folder), save_checkpoint_dir=ns.checkpoints_dir, checkpoint=checkpoint,
        warm_model=warm, device=device, device_dataset=ns.device_dataset, resample_inputs=ns.resample_inputs)
  if world > 1:
    torch.distributed.destroy_process_group()
  return True


def synthesize(ns, from_wav: bool = False) -> bool:
  logger = getLogger(__name__)
  rank, world = int(os.environ.get("RANK", "0")), int(os.environ.get("WORLD_SIZE", "1"))
  device = torch.device(ns.device if world == 1 else f"cuda:{int(os.environ.get('LOCAL_RANK', '0'))}")
  out_dir = ns.output_directory or ns.folder
  if out_dir.is_file():
    logger.error("Output directory is a file!")
    return False
  seed = ns.custom_seed if ns.custom_seed is not None else random.randint(1, 9999)
  try:
    ckpt = CheckpointWaveglow.load(ns.checkpoint, device)
  except Exception:
    logger.error("Checkpoint couldn't be loaded!")
    return False
  suffix = ".wav" if from_wav else ".npy"
  mel_files = sorted(p for p in ns.folder.rglob("*") if p.is_file() and p.suffix.lower() == suffix)
  mel_files = shard_list(mel_files, rank, world)
  synth = Synthesizer(ckpt, custom_hparams=split_hparams_string(ns.custom_hparams), device=device)
  taco_stft = None
  if from_wav:
    from .taco_stft import TacotronSTFT
    taco_stft = TacotronSTFT(synth.hparams, device, resample_inputs=ns.resample_inputs)   # inference_wav.py:110
  todo = []
  for mel_path in mel_files:
    wav_path = out_dir / mel_path.relative_to(ns.folder).parent / f"{mel_path.stem}.wav"
    if wav_path.exists() and not ns.overwrite:
      continue
    todo.append((mel_path, wav_path))
  bs = max(1, ns.batch_size)
  for i in range(0, len(todo), bs):
    chunk = todo[i:i + bs]
    if len(chunk) == 1 and ns.output_sampling_rate is None:           # the reference-shaped path, one utterance
      mel_path, wav_path = chunk[0]
      if from_wav:
        mel = taco_stft.get_mel_tensor_from_file(mel_path).unsqueeze(0)
      else:
        mel = torch.FloatTensor(np.load(mel_path)).unsqueeze(0)
      res = synth.infer(mel, sigma=ns.sigma, denoiser_strength=ns.denoiser_strength, seed=seed)
      wav_path.parent.mkdir(parents=True, exist_ok=True)
      float_to_wav(normalize_wav(res.wav_denoised), wav_path, sample_rate=res.sampling_rate)
      continue
    # a batch: one mel call, one launch sequence, int16 samples back from the device (the same bytes as above)
    if from_wav:
      mel, frames = taco_stft.get_mel_tensors_from_files([p for p, _ in chunk])
      mels = [mel[b, :, :frames[b]] for b in range(len(chunk))]
    else:
      mels = [torch.FloatTensor(np.load(p)) for p, _ in chunk]
    results = synth.infer_batch_pcm(mels, sigma=ns.sigma, denoiser_strength=ns.denoiser_strength, seed=seed,
                                    **({} if ns.output_sampling_rate is None else
                                       {"output_sampling_rate": ns.output_sampling_rate}))
    for (_, wav_path), res in zip(chunk, results):
      wav_path.parent.mkdir(parents=True, exist_ok=True)
      write_wav(filename=wav_path, rate=res.sampling_rate, data=res.pcm)
  return True


def _save_validation(entry, output, val_dir: Path, iteration: int) -> None:
  """src/waveglow_cli/validation.py:61-83 without the plots."""
  dest = val_dir / f"it={iteration}_name={entry.basename}"
  dest.mkdir(parents=True, exist_ok=True)
  np.save(dest / "original.mel.npy", output.mel_orig)
  np.save(dest / "inferred_denoised.mel.npy", output.mel_inferred_denoised)
  float_to_wav(output.wav_orig, dest / "original.wav", sample_rate=output.orig_sr)
  write_wav(filename=dest / "inferred_denoised.wav", rate=output.inferred_sr, data=output.wav_inferred_denoised)
  write_wav(filename=dest / "inferred.wav", rate=output.inferred_sr, data=output.wav_inferred)


def validate_cmd(ns) -> bool:
  """src/waveglow_cli/validation.py:107-153."""
  import logging
  from functools import partial
  from .training import get_last_checkpoint, get_pytorch_filename, load_dataset
  from .validation import ValidationEntries, get_df, validate
  logger = getLogger(__name__)
  if int(os.environ.get("WORLD_SIZE", "1")) > 1:
    logger.error("validate runs in a single process: start it without torch.distributed.run")
    return False
  for d in (ns.checkpoints_dir, ns.dataset_dir):
    if not d.is_dir():
      logger.error(f"{d} is not a directory!")
      return False
  data = load_dataset(ns.dataset_dir)
  try:
    iterations = sorted(set(ns.custom_checkpoints)) or [get_last_checkpoint(ns.checkpoints_dir)[1]]
  except Exception as e:
    logger.error(str(e))
    return False
  ns.output_dir.mkdir(parents=True, exist_ok=True)
  val_logger = getLogger("waveglow_amd")
  handler = logging.FileHandler(ns.output_dir / "log.txt", mode="w")
  handler.setFormatter(logging.Formatter("[%(asctime)s] (%(levelname)s) %(message)s"))
  old_level = val_logger.level
  val_logger.addHandler(handler)
  val_logger.setLevel(logging.INFO)
  try:
    logger.info("Validating...")
    logger.info(f"Checkpoints: {','.join(str(x) for x in iterations)}")
    result = ValidationEntries()
    for iteration in iterations:
      logger.info(f"Current checkpoint: {iteration}")
      path = ns.checkpoints_dir / get_pytorch_filename(iteration)
      if not path.is_file():
        logger.error(f"Checkpoint {path} not found!")
        return False
      ckpt = CheckpointWaveglow.load(path, torch.device(ns.device))
      try:
        result.extend(validate(checkpoint=ckpt, data=data, custom_hparams=split_hparams_string(ns.custom_hparams),
                               entry_names=set(ns.files), full_run=ns.full_run,
                               save_callback=partial(_save_validation, val_dir=ns.output_dir, iteration=iteration),
                               sigma=ns.sigma, denoiser_strength=ns.denoiser_strength, seed=ns.custom_seed,
                               device=torch.device(ns.device), batch_size=ns.batch_size,
                               pitch_metrics=ns.pitch_metrics, resample_inputs=ns.resample_inputs,
                               intelligibility_metrics=ns.intelligibility_metrics, likelihood=ns.likelihood))
      except AssertionError as e:
        logger.error(str(e) or "validation failed an assertion")
        return False
    if len(result) > 0:
      get_df(result).to_csv(ns.output_dir / "total.csv", sep="\t", header=True, index=False)
      logger.info(f"Saved output to: {ns.output_dir.absolute()}")
    return True
  finally:
    val_logger.removeHandler(handler)
    val_logger.setLevel(old_level)
    handler.close()


def main(argv=None) -> int:
  ns = build_parser().parse_args(argv)
  if ns.command in ("synthesize", "synthesize-wav"):
    ok = synthesize(ns, from_wav=ns.command == "synthesize-wav")
  elif ns.command == "validate":
    ok = validate_cmd(ns)
  else:
    ok = train_cmd(ns, resume=ns.command == "continue-train")
  return 0 if ok else 1


if __name__ == "__main__":
  sys.exit(main())
