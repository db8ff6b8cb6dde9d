// C ABI of the streaming step's two memory kernels (include/waveglow_amd.h: wg_stream_gather, wg_stream_emit).  Argument
// checks run before any device work; the tables live on the device and are read by the kernels only.
#include "wg_host.h"
#include "wg_stream.h"

using namespace wg;

extern "C" {

int wg_stream_gather(const wg_stream_window* windows, void* mel_out, void* z_init_out, void* const* z_early_out,
                     int32_t n_early, int32_t B, int32_t n_mel, int32_t n_mel_out, int32_t n_rem, int32_t n_early_size,
                     int32_t w_max, int32_t cols_per_frame, int32_t io_dtype, void* stream) {
  if (!windows || !mel_out || !z_init_out) return fail(WG_ERR_INVALID, "null argument");
  if (io_dtype != WG_F32 && io_dtype != WG_F16) return fail(WG_ERR_INVALID, "stream gather: bad io_dtype");
  if (n_early < 0 || n_early > WG_STREAM_MAX_EARLY || (n_early && !z_early_out))
    return fail(WG_ERR_INVALID, "stream gather: 0 <= n_early <= %d, with their outputs", WG_STREAM_MAX_EARLY);
  if (B < 1 || B > 65535 || n_mel < 1 || n_mel_out < n_mel || n_rem < 1 || w_max < 1 || (n_early && n_early_size < 1))
    return fail(WG_ERR_INVALID, "stream gather: 1 <= B <= 65535, 1 <= n_mel <= n_mel_out, n_rem >= 1, n_early_size >= 1, w_max >= 1");
  if (cols_per_frame < 8 || cols_per_frame % 8) return fail(WG_ERR_INVALID, "stream gather: cols_per_frame a multiple of 8");
  // every index inside one row block of a plane is an int in the kernel
  const int64_t most_ch = n_rem > n_early_size ? n_rem : n_early_size;
  if ((int64_t)n_mel_out * w_max >= (1ll << 31) || most_ch * cols_per_frame * w_max >= (1ll << 31))
    return fail(WG_ERR_INVALID, "stream gather: a window of %d frames is too large", w_max);
  StreamGatherDst dst{};
  dst.mel = mel_out;
  dst.z_init = z_init_out;
  uintptr_t bits = (uintptr_t)mel_out | (uintptr_t)z_init_out;
  for (int i = 0; i < n_early; ++i) {
    if (!z_early_out[i]) return fail(WG_ERR_INVALID, "null argument");
    dst.z_early[i] = z_early_out[i];
    bits |= (uintptr_t)z_early_out[i];
  }
  if (bits & 15) return fail(WG_ERR_INVALID, "stream gather: outputs must be 16-byte aligned");
  HIP_TRY(launch_stream_gather(windows, dst, n_early, B, n_mel, n_mel_out, n_rem, n_early ? n_early_size : 1, w_max,
                               cols_per_frame, io_dtype == WG_F16, (hipStream_t)stream));
  return WG_OK;
}

int wg_stream_emit(const wg_stream_crop* crops, int16_t* pcm_out, float* stats_out, int32_t B, int32_t n_max,
                   void* stream) {
  if (!crops || !pcm_out || !stats_out) return fail(WG_ERR_INVALID, "null argument");
  if (B < 1 || n_max < 8 || n_max % 8) return fail(WG_ERR_INVALID, "stream emit: B >= 1, n_max a multiple of 8");
  if ((uintptr_t)pcm_out & 15) return fail(WG_ERR_INVALID, "stream emit: pcm_out must be 16-byte aligned");
  HIP_TRY(launch_stream_emit(crops, pcm_out, stats_out, B, n_max, (hipStream_t)stream));
  return WG_OK;
}

}  // extern "C"
