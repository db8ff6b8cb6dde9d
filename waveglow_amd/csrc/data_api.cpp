// C ABI of the device-resident training data path (include/waveglow_amd.h: wg_data_gather).  Argument checks run before
// any device work.
#include "wg_host.h"

using namespace wg;

extern "C" {

int wg_data_gather(const void* pool, int32_t pool_dtype, int64_t pool_elems, const int64_t* offsets, int32_t n_utt,
                   const int32_t* picks, float* audio_out, int32_t* status_out, int32_t B, int32_t segment_length,
                   void* stream) {
  if (!pool || !offsets || !picks || !audio_out) return fail(WG_ERR_INVALID, "null argument");
  if (pool_dtype != WG_PCM_I16 && pool_dtype != WG_PCM_F32) return fail(WG_ERR_INVALID, "data gather: bad pool_dtype");
  if (B < 1 || n_utt < 1 || segment_length < 1 || pool_elems < 0)
    return fail(WG_ERR_INVALID, "data gather: B >= 1, n_utt >= 1, segment_length >= 1, pool_elems >= 0");
  HIP_TRY(launch_data_gather(pool, pool_dtype == WG_PCM_I16, pool_elems, offsets, n_utt, picks, audio_out, status_out, B,
                             segment_length, (hipStream_t)stream));
  return WG_OK;
}

}  // extern "C"
