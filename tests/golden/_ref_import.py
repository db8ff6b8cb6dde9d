"""Import the reference's own model code in the BUILD CONTAINER only (fixture generation).

/root/reference does not exist on the GPU box; nothing under tests/ imports this module
at test time.  The reference's package __init__ pulls in optional dependencies that are
absent here and are off the hot path, so empty stand-in modules
are registered for exactly those names before the import.
"""
import os
import sys
import types

REF_SRC = "/root/reference/src"
_STUBS = ["fastdtw", "fastdtw.fastdtw", "librosa", "librosa.util", "librosa.filters",
          "skimage", "skimage.metrics", "imageio", "mel_cepstral_distance", "wget",
          "gdown", "ordered_set"]


def import_reference():
  os.environ.setdefault("PYTHONDONTWRITEBYTECODE", "1")
  sys.dont_write_bytecode = True
  for name in _STUBS:
    if name not in sys.modules:
      m = types.ModuleType(name)
      m.__path__ = []  # allow submodule imports
      sys.modules[name] = m
  # names the reference imports *from* those modules at import time
  sys.modules["fastdtw.fastdtw"].fastdtw = lambda *a, **k: None
  sys.modules["fastdtw"].fastdtw = sys.modules["fastdtw.fastdtw"]
  for attr in ("pad_center", "tiny", "normalize"):
    setattr(sys.modules["librosa.util"], attr, lambda *a, **k: None)
  sys.modules["librosa.filters"].mel = lambda *a, **k: None
  sys.modules["librosa"].util = sys.modules["librosa.util"]
  sys.modules["librosa"].filters = sys.modules["librosa.filters"]
  sys.modules["skimage.metrics"].structural_similarity = lambda *a, **k: None
  sys.modules["ordered_set"].OrderedSet = set
  for attr in ("get_metrics_mels", "get_metrics_wavs", "compare_mel_spectrograms", "get_mcd_between_mel_spectograms"):
    setattr(sys.modules["mel_cepstral_distance"], attr, lambda *a, **k: None)
  if REF_SRC not in sys.path:
    sys.path.insert(0, REF_SRC)
  import waveglow.model as ref_model      # noqa: E402
  import waveglow.hparams as ref_hparams  # noqa: E402
  import waveglow.train as ref_train      # noqa: E402
  return ref_model, ref_hparams, ref_train


def _pad_center(data, *, size, axis=-1):
  """librosa.util.pad_center as documented: zero-pad ``axis`` to ``size``, ``(size - n) // 2`` zeros on the left."""
  import numpy as np
  data = np.asarray(data)
  n = data.shape[axis]
  if size < n:
    raise ValueError(f"pad_center: target size {size} is below the input's {n}")
  lpad = (size - n) // 2
  widths = [(0, 0)] * data.ndim
  widths[axis] = (lpad, size - n - lpad)
  return np.pad(data, widths, mode="constant")


def _tiny(x):
  """librosa.util.tiny as documented: the smallest positive normal number of x's dtype, float32 for non-float input."""
  import numpy as np
  x = np.asarray(x)
  floating = np.issubdtype(x.dtype, np.floating) or np.issubdtype(x.dtype, np.complexfloating)
  return np.finfo(x.dtype if floating else np.float32).tiny


def _normalize(S, *, norm=None, **kwargs):
  """librosa.util.normalize for the one way the reference calls it (``norm=None``): the identity."""
  assert norm is None and not kwargs
  return S


def _mel(*, sr, n_fft, n_mels, fmin, fmax):
  """librosa.filters.mel: the PROJECT's restatement (the one thing a fixture made this way does not pin)."""
  from waveglow_amd.taco_stft import slaney_mel_filterbank
  return slaney_mel_filterbank(sr, n_fft, n_mels, fmin, fmax)


def import_reference_stft():
  """The reference's own ``waveglow.stft``, ``waveglow.taco_stft`` and ``waveglow.denoiser`` modules with FUNCTIONAL
  stand-ins for the four librosa names they use (our code, written from librosa's documented behaviour).

  The reference binds those names at import time (``from librosa.util import ...``), and ``import_reference`` -- whose
  package import already pulls the three modules in with inert stubs -- runs first; so the stand-ins are installed and
  the three modules are dropped from ``sys.modules`` and imported again.  Returns (stft, taco_stft, denoiser)."""
  import importlib
  import_reference()
  util, filters = sys.modules["librosa.util"], sys.modules["librosa.filters"]
  util.pad_center, util.tiny, util.normalize = _pad_center, _tiny, _normalize
  filters.mel = _mel
  names = ("waveglow.stft", "waveglow.taco_stft", "waveglow.denoiser")
  for name in names:
    sys.modules.pop(name, None)
  return tuple(importlib.import_module(name) for name in names)
