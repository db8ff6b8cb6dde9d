"""ctypes binding of libwaveglow_amd.so (C ABI: include/waveglow_amd.h).

The library is built in-tree by ``__graft_entry__.build()`` / ``waveglow_amd.build.build_library()``.
There is no fallback: if it is missing or fails to load, every compute entry point raises.
"""
from __future__ import annotations

import ctypes as C
import os
from typing import Optional

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("WAVEGLOW_AMD_LIB", os.path.join(_HERE, "csrc", "libwaveglow_amd.so"))

WG_F32, WG_F16 = 0, 1
WG_PCM_I16, WG_PCM_F32 = 0, 1   # pool_dtype of wg_data_gather
WG_PCM_F64 = 2                  # d_out_dtype of wg_resample_backward only
WG_RESAMPLE_CLIP = 1           # flag of wg_resample
WG_SDTW_L2, WG_SDTW_SQ = 0, 1   # cost of wg_softdtw_forward / wg_softdtw_backward
WG_PLAN_INFER, WG_PLAN_FORWARD, WG_PLAN_TRAIN = 0, 1, 2     # direction of wg_plan
WG_PLAN_SINGLE, WG_PLAN_PAIR, WG_PLAN_RESIDENT = 0, 1, 2    # wg_plan_result.form
WG_TRAIN_RECOMPUTE = 1       # flag of the wg_train_* entry points that take flags (include/waveglow_amd.h)


class WgConfig(C.Structure):
  _fields_ = [(n, C.c_int32) for n in (
    "n_mel_channels", "n_flows", "n_group", "n_early_every", "n_early_size", "n_layers",
    "n_channels", "kernel_size", "upsample_kernel", "upsample_stride")]


class WgTrainWeights(C.Structure):
  """wg_train_weights (include/waveglow_amd.h): device pointers; wstart .. w1x1 are arrays of n_flows pointers, wupt is
  optional (null unless the mel input gradient is wanted), winv (array of n_flows pointers) too (null unless synthesis
  takes W^-1 from the per-call weights)."""
  _fields_ = [(n, C.c_void_p) for n in (
    "a1", "a1c", "b1", "a2", "b2", "es", "wat", "wbt", "wct", "wup", "bup", "wstart", "bstart", "out_init", "w1x1", "wupt",
    "winv")]


class WgTrainGrads(C.Structure):
  """wg_train_grads: device pointers; the last three are arrays of n_flows pointers."""
  _fields_ = [(n, C.c_void_p) for n in (
    "dw1", "db1", "dw2", "db2", "dwes", "dwup", "dbup", "dstart", "dout_init", "dw1x1")] + [
    ("layer_stride", C.c_int64), ("flow_stride", C.c_int64)]


class WgPitchParams(C.Structure):
  """wg_pitch_params (include/waveglow_amd.h)."""
  _fields_ = [("sampling_rate", C.c_double), ("threshold", C.c_double)] + [(n, C.c_int32) for n in (
    "frame_length", "hop_length", "tau_min", "tau_max")]


class WgStoiParams(C.Structure):
  """wg_stoi_params (include/waveglow_amd.h): device pointers to the window, the band table and the cos/sin table."""
  _fields_ = [(n, C.c_void_p) for n in ("window", "bands", "cossin")]


class WgPlanResult(C.Structure):
  """wg_plan_result (include/waveglow_amd.h): the kernel variant of a call, from wg_plan."""
  _fields_ = [(n, C.c_int32) for n in (
    "block_n", "form", "resident_wgs", "deep", "frag16", "halves", "rows_per_utterance", "rows_per_phase", "n_tiles")]


class WgError(RuntimeError):
  pass


_lib: Optional[C.CDLL] = None

# name -> (restype, argtypes); every symbol declared in include/waveglow_amd.h
SIGNATURES = {
  "wg_version": (C.c_char_p, []),
  "wg_last_error": (C.c_char_p, []),
  "wg_create": (C.c_int, [C.POINTER(WgConfig), C.c_int, C.POINTER(C.c_void_p)]),
  "wg_destroy": (C.c_int, [C.c_void_p]),
  "wg_set_tensor": (C.c_int, [C.c_void_p, C.c_char_p, C.c_void_p, C.POINTER(C.c_int64), C.c_int32]),
  "wg_num_expected_tensors": (C.c_int, [C.c_void_p]),
  "wg_expected_tensor_name": (C.c_char_p, [C.c_void_p, C.c_int32]),
  "wg_finalize": (C.c_int, [C.c_void_p]),
  "wg_infer_workspace_bytes": (C.c_size_t, [C.c_void_p, C.c_int32, C.c_int32]),
  "wg_forward_workspace_bytes": (C.c_size_t, [C.c_void_p, C.c_int32, C.c_int32, C.c_int32]),
  "wg_infer": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(C.c_void_p), C.c_int32, C.c_float,
                         C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_void_p, C.c_size_t, C.c_void_p]),
  "wg_forward": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(C.c_void_p),
                           C.POINTER(C.c_float), C.c_int32, C.c_int32, C.c_int32, C.c_int32,
                           C.c_void_p, C.c_size_t, C.c_void_p]),
  "wg_nll_workspace_bytes": (C.c_size_t, [C.c_void_p, C.c_int32, C.c_int32]),
  "wg_nll": (C.c_int, [C.c_void_p, C.c_void_p, C.POINTER(C.c_void_p), C.c_void_p, C.c_double, C.c_int32, C.c_int32,
                       C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]),
  "wg_loss": (C.c_int, [C.c_void_p, C.c_int64, C.POINTER(C.c_void_p), C.POINTER(C.c_int64), C.c_int32,
                        C.POINTER(C.c_float), C.c_float, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]),
  "wg_loss_dev": (C.c_int, [C.c_void_p, C.c_int64, C.POINTER(C.c_void_p), C.POINTER(C.c_int64), C.c_int32,
                            C.c_void_p, C.c_float, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]),
  "wg_macs_per_group_step": (C.c_double, [C.c_void_p]),
  "wg_train_workspace_bytes": (C.c_size_t, [C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_int32]),
  "wg_wn_waves": (C.c_int32, [C.c_int32]),
  "wg_train_param_count": (C.c_int32, [C.c_void_p, C.c_int32]),
  "wg_train_param_name": (C.c_char_p, [C.c_void_p, C.c_int32, C.c_int32]),
  "wg_train_param_numel": (C.c_int64, [C.c_void_p, C.c_int32, C.c_int32]),
  "wg_train_prepare_bytes": (C.c_size_t, [C.c_void_p]),
  "wg_train_prepare": (C.c_int, [C.c_void_p, C.POINTER(C.c_void_p), C.c_int32, C.POINTER(WgTrainWeights), C.c_void_p,
                                 C.c_size_t, C.c_void_p]),
  "wg_train_param_grads": (C.c_int, [C.c_void_p, C.POINTER(C.c_void_p), C.c_int32, C.POINTER(WgTrainGrads), C.c_void_p,
                                     C.c_size_t, C.c_void_p, C.c_void_p]),
  "wg_train_forward": (C.c_int, [C.c_void_p, C.POINTER(WgTrainWeights), C.c_void_p, C.c_void_p, C.c_void_p,
                                 C.POINTER(C.c_void_p), C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_void_p,
                                 C.c_size_t, C.c_int32, C.c_void_p]),
  "wg_train_backward": (C.c_int, [C.c_void_p, C.POINTER(WgTrainWeights), C.POINTER(WgTrainGrads), C.c_void_p,
                                  C.POINTER(C.c_void_p), C.c_float, C.c_void_p, C.c_void_p, C.c_void_p,
                                  C.c_int32, C.c_int32, C.c_int32, C.c_void_p, C.c_size_t, C.c_int32, C.c_int32,
                                  C.c_int32, C.c_void_p]),
  "wg_train_infer_forward": (C.c_int, [C.c_void_p, C.POINTER(WgTrainWeights), C.c_void_p, C.c_void_p,
                                       C.POINTER(C.c_void_p), C.c_int32, C.c_float, C.c_void_p, C.c_int32,
                                       C.c_int32, C.c_void_p, C.c_int32, C.c_void_p, C.c_size_t, C.c_int32,
                                       C.c_void_p]),
  "wg_train_infer_backward": (C.c_int, [C.c_void_p, C.POINTER(WgTrainWeights), C.POINTER(WgTrainGrads), C.c_void_p,
                                        C.c_float, C.c_float, C.c_void_p, C.c_void_p, C.POINTER(C.c_void_p),
                                        C.c_int32, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.c_size_t,
                                        C.c_int32, C.c_void_p]),
  "wg_stft_create": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.POINTER(C.c_void_p)]),
  "wg_stft_destroy": (C.c_int, [C.c_void_p]),
  "wg_stft_workspace_bytes": (C.c_size_t, [C.c_void_p, C.c_int32, C.c_int32]),
  "wg_stft_denoise": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_float, C.c_void_p, C.c_void_p,
                                C.c_int32, C.c_int32, C.c_void_p, C.c_size_t, C.c_void_p]),
  "wg_stft_denoise_grad_workspace_bytes": (C.c_size_t, [C.c_void_p, C.c_int32, C.c_int32]),
  "wg_stft_denoise_forward_saved": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_float, C.c_void_p,
                                              C.c_int32, C.c_int32, C.c_void_p, C.c_size_t, C.c_void_p]),
  "wg_stft_denoise_backward": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_float, C.c_int32,
                                         C.c_void_p, C.c_int32, C.c_int32, C.c_void_p, C.c_size_t, C.c_void_p]),
  "wg_stft_mel_workspace_bytes": (C.c_size_t, [C.c_void_p, C.c_int32, C.c_int32]),
  "wg_stft_mel": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32,
                            C.c_int32, C.c_void_p, C.c_size_t, C.c_void_p]),
  "wg_stft_mel_grad_workspace_bytes": (C.c_size_t, [C.c_void_p, C.c_int32, C.c_int32]),
  "wg_stft_mel_forward_saved": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p,
                                          C.c_int32, C.c_int32, C.c_void_p, C.c_size_t, C.c_void_p]),
  "wg_stft_mel_backward": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p,
                                     C.c_int32, C.c_int32, C.c_void_p, C.c_size_t, C.c_void_p]),
  "wg_wav_finish_workspace_bytes": (C.c_size_t, [C.c_int32]),
  "wg_wav_finish": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_int32,
                              C.c_void_p, C.c_size_t, C.c_void_p]),
  "wg_data_gather": (C.c_int, [C.c_void_p, C.c_int32, C.c_int64, C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p,
                               C.c_void_p, C.c_int32, C.c_int32, C.c_void_p]),
  "wg_stream_gather": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(C.c_void_p), C.c_int32, C.c_int32, C.c_int32,
                                 C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_void_p]),
  "wg_stream_emit": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_void_p]),
  "wg_metrics_workspace_bytes": (C.c_size_t, [C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32]),
  "wg_metrics_mfcc": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_int32,
                                C.c_void_p, C.c_size_t, C.c_void_p]),
  "wg_metrics_dtw": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32,
                               C.c_int32, C.c_int32, C.c_int32, C.c_void_p]),
  "wg_metrics_mel": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_int32,
                               C.c_int32, C.c_int32, C.c_int32, C.c_void_p, C.c_size_t, C.c_void_p]),
  "wg_pitch_frames": (C.c_int32, [C.POINTER(WgPitchParams), C.c_int32]),
  "wg_pitch_workspace_bytes": (C.c_size_t, [C.POINTER(WgPitchParams), C.c_int32, C.c_int32, C.c_int32]),
  "wg_pitch_yin": (C.c_int, [C.c_void_p, C.c_void_p, C.POINTER(WgPitchParams), C.c_void_p, C.c_void_p, C.c_void_p,
                             C.c_int32, C.c_int32, C.c_int32, C.c_void_p]),
  "wg_pitch_compare": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_int32,
                                 C.c_int32, C.c_void_p]),
  "wg_pitch_metrics": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_int32,
                                 C.POINTER(WgPitchParams), C.c_void_p, C.c_int32, C.c_void_p, C.c_size_t, C.c_void_p]),
  "wg_stoi_workspace_bytes": (C.c_size_t, [C.c_int32, C.c_int32]),
  "wg_stoi": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.POINTER(WgStoiParams),
                        C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]),
  "wg_stoi_saved_bytes": (C.c_size_t, [C.c_int32, C.c_int32]),
  "wg_stoi_backward_workspace_bytes": (C.c_size_t, [C.c_int32, C.c_int32]),
  "wg_stoi_forward": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_int32,
                                C.POINTER(WgStoiParams), C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t,
                                C.c_void_p]),
  "wg_stoi_backward": (C.c_int, [C.c_void_p, C.c_int32, C.c_int32, C.POINTER(WgStoiParams), C.c_void_p, C.c_void_p,
                                 C.c_size_t, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]),
  "wg_softdtw_bytes": (C.c_size_t, [C.c_int32, C.c_int32, C.c_int32]),
  "wg_softdtw_forward": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_double, C.c_int32, C.c_void_p,
                                   C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_void_p]),
  "wg_softdtw_backward": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_double, C.c_int32, C.c_void_p,
                                    C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_int32,
                                    C.c_int32, C.c_void_p]),
  "wg_softdtw_banded_bytes": (C.c_size_t, [C.c_int32, C.c_int32, C.c_int32, C.c_int32]),
  "wg_softdtw_banded_forward": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_double, C.c_int32,
                                          C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32,
                                          C.c_void_p]),
  "wg_softdtw_banded_backward": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_double, C.c_int32,
                                           C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32,
                                           C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_void_p]),
  "wg_resample_backward": (C.c_int, [C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_int32,
                                     C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_void_p]),
  "wg_resample_plan": (C.c_int, [C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.POINTER(C.c_int32), C.POINTER(C.c_int32),
                                 C.POINTER(C.c_int32), C.POINTER(C.c_int32)]),
  "wg_resample": (C.c_int, [C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_int32,
                            C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_void_p]),
  "wg_stftloss_create": (C.c_int, [C.c_int32, C.POINTER(C.c_int32), C.POINTER(C.c_int32), C.POINTER(C.c_int32),
                                  C.POINTER(C.c_void_p), C.c_float, C.c_int32, C.POINTER(C.c_void_p)]),
  "wg_stftloss_destroy": (C.c_int, [C.c_void_p]),
  "wg_stftloss_workspace_bytes": (C.c_size_t, [C.c_void_p, C.c_int32, C.c_int32, C.c_int32]),
  "wg_stftloss_forward": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_float, C.c_float, C.c_void_p,
                                    C.c_int32, C.c_int32, C.c_int32, C.c_void_p, C.c_size_t, C.c_void_p]),
  "wg_stftloss_backward": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_float, C.c_float, C.c_void_p,
                                     C.c_int32, C.c_int32, C.c_void_p, C.c_size_t, C.c_void_p]),
  "wg_melloss_create": (C.c_int, [C.c_int32, C.POINTER(C.c_int32), C.POINTER(C.c_int32), C.POINTER(C.c_int32),
                                 C.POINTER(C.c_int32), C.POINTER(C.c_void_p), C.POINTER(C.c_void_p), C.c_float, C.c_int32,
                                 C.POINTER(C.c_void_p)]),
  "wg_melloss_destroy": (C.c_int, [C.c_void_p]),
  "wg_melloss_spectra_elems": (C.c_size_t, [C.c_void_p, C.c_int32, C.c_int32]),
  "wg_melloss_mels_elems": (C.c_size_t, [C.c_void_p, C.c_int32, C.c_int32]),
  "wg_melloss_forward": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_float, C.c_float, C.c_void_p,
                                   C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_void_p]),
  "wg_melloss_backward": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_float, C.c_float, C.c_void_p, C.c_void_p,
                                    C.c_void_p, C.c_int32, C.c_int32, C.c_void_p]),
  "wg_plan": (C.c_int, [C.POINTER(WgConfig), C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.POINTER(WgPlanResult)]),
  "wg_debug_set_stamp_buffer":(C.c_int, [C.c_void_p, C.c_void_p]),
  "wg_profile_enable": (C.c_int, [C.c_void_p, C.c_int32]),
  "wg_profile_read": (C.c_int, [C.c_void_p, C.POINTER(C.c_double), C.POINTER(C.c_int64), C.c_int32]),
}


def load() -> C.CDLL:
  """Load the HIP library or raise -- never falls back to another implementation."""
  global _lib
  if _lib is not None:
    return _lib
  if not os.path.isfile(LIB_PATH):
    raise WgError(f"{LIB_PATH} not found: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
                  "(hipcc --offload-arch=gfx950). There is no CPU fallback.")
  lib = C.CDLL(LIB_PATH)
  for name, (res, args) in SIGNATURES.items():
    fn = getattr(lib, name)
    fn.restype = res
    fn.argtypes = args
  _lib = lib
  return lib


def plan(cfg: WgConfig, direction: int, B: int, n_frames: int, n_cu: int) -> WgPlanResult:
  """wg_plan: the WN-layer kernel variant a call of this size runs on a device with ``n_cu`` compute units (no GPU needed)."""
  out = WgPlanResult()
  check(load().wg_plan(C.byref(cfg), direction, B, n_frames, n_cu, C.byref(out)))
  return out


def device_index(device) -> int:
  """Ordinal of a 'cuda' torch.device; an index-less ``torch.device('cuda')`` means torch's CURRENT device (under
  LOCAL_RANK > 0 that is not GPU 0)."""
  import torch
  device = torch.device(device)
  return device.index if device.index is not None else torch.cuda.current_device()


def check(rc: int) -> None:
  if rc != 0:
    raise WgError(f"libwaveglow_amd error {rc}: {load().wg_last_error().decode()}")
