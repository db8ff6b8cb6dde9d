// Launch entry points of stream.hip, shared with stream_api.cpp (host).  The row types are the public ones
// (include/waveglow_amd.h: wg_stream_window, wg_stream_crop).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/waveglow_amd.h"

namespace wg {

constexpr int kStreamStats = 8;        // floats per row in stats_out
constexpr int kStreamEmitThreads = 512;

// destinations of wg_stream_gather, by value in the kernel's arguments
struct StreamGatherDst {
  void* mel;
  void* z_init;
  void* z_early[WG_STREAM_MAX_EARLY];
};

// windows [B] (device) -> the padded batch tensors (arguments checked by stream_api.cpp)
hipError_t launch_stream_gather(const wg_stream_window* windows, const StreamGatherDst& dst, int n_early, int B, int n_mel,
                                int n_mel_out, int n_rem, int n_early_size, int w_max, int cpf, bool is_f16,
                                hipStream_t s);

// crops [B] (device) -> pcm [B][n_max] int16, stats [B][8] fp32
hipError_t launch_stream_emit(const wg_stream_crop* crops, int16_t* pcm, float* stats, int B, int n_max, hipStream_t s);

}  // namespace wg
