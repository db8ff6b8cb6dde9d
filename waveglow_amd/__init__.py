"""MI355X-native WaveGlow hot path (infer / forward) behind the reference's Python surface.

Public names mirror ``waveglow/__init__.py`` of stefantaubert/waveglow where the hot path touches them.
"""
from .hparams import HParams  # noqa: F401
from .model import WaveGlow  # noqa: F401
from .checkpoint import CheckpointWaveglow  # noqa: F401
from .synthesizer import InferenceResult, Synthesizer  # noqa: F401
from .model import WaveGlowLoss  # noqa: F401
from .audio import float_to_wav, normalize_wav  # noqa: F401


def __getattr__(name):
  # scipy-dependent / heavier pieces are imported on first use
  if name in ("train", "load_dataset", "Entry"):
    from . import training
    return getattr(training, name)
  if name in ("TacotronSTFT", "TSTFTHParams"):
    from . import taco_stft
    return getattr(taco_stft, name)
  if name == "MultiResolutionSTFTLoss":
    from .stft_loss import MultiResolutionSTFTLoss
    return MultiResolutionSTFTLoss
  if name == "MultiScaleMelLoss":
    from .mel_loss import MultiScaleMelLoss
    return MultiScaleMelLoss
  if name == "STOILoss":
    from .stoi_loss import STOILoss
    return STOILoss
  if name in ("SoftDTWLoss", "soft_dtw", "soft_dtw_alignment", "soft_dtw_divergence"):
    from . import softdtw
    return getattr(softdtw, name)
  if name in ("mel_metrics", "MelMetrics", "pitch_metrics", "PitchMetrics", "yin_f0", "intelligibility_metrics",
              "IntelligibilityMetrics", "stoi"):
    from . import metrics
    return getattr(metrics, name)
  if name in ("Likelihood", "log_likelihood", "log_likelihood_enqueue"):
    from . import likelihood
    return getattr(likelihood, name)
  if name in ("resample_enqueue", "resample_plan", "out_len"):
    # `waveglow_amd.resample` is the submodule (as `waveglow_amd.metrics` is); its function is `resample.resample`
    from . import resample
    return getattr(resample, name)
  if name in ("validate", "ValidationEntry", "ValidationEntries"):
    from . import validation
    return getattr(validation, name)
  if name in ("StreamSession", "StreamChunk", "stream_halo"):
    from . import streaming
    return getattr(streaming, name)
  if name == "Denoiser":
    from .denoiser import Denoiser
    return Denoiser
  raise AttributeError(name)
