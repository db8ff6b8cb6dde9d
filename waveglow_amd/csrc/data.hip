// Training segments out of a wav pool that lives on the device: what the host did per utterance with
// get_wav_tensor_segment (src/waveglow/audio_utils.py:141-150: crop at a drawn start, or zero padding up to the segment
// length) on the samples convert_wav made of the file (audio_utils.py:36-64), for a whole batch in one launch.
//
// One thread per output sample, scalar loads and stores.  A segment starts wherever the draw fell: an int16 segment on
// an odd sample is only 2-byte aligned, an fp32 one only 4-byte aligned, and the last segment of the pool ends on the
// pool's last element, so no load wider than the element is provably aligned and in bounds.  Lane i still reads element
// i of a row, which is the coalesced pattern, and a batch is 2 MB: the launch is bound by its latency, not by the loads.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "wg_host.h"

namespace wg {

// grid (ceil(N / 256), min(B, 65535)), 256 threads.  Row b: u = picks[b][0], s = picks[b][1], len = offsets[u + 1] -
// offsets[u]; out[b][i] = conv(pool[offsets[u] + s + i]) where s + i < len, 0 elsewhere.  A pick outside the pool
// (u outside [0, n_utt), s < 0, s > max(len - N, 0)) gives a zero row and sets *status; so does an utterance whose
// offsets do not lie inside [0, pool_elems] in ascending order, so that nothing outside the pool is read whatever
// picks and offsets hold.
template <typename T>
__global__ void __launch_bounds__(256) data_gather_kernel(const T* __restrict__ pool, int64_t pool_elems,
                                                          const int64_t* __restrict__ offsets, int n_utt,
                                                          const int* __restrict__ picks, float* __restrict__ out,
                                                          int* status, int B, int N) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  for (int b = blockIdx.y; b < B; b += gridDim.y) {
    const int u = picks[2 * b], s = picks[2 * b + 1];
    int64_t base = 0, len = 0;
    bool ok = u >= 0 && u < n_utt && s >= 0;
    if (ok) {
      base = offsets[u];
      len = offsets[u + 1] - base;
      ok = base >= 0 && len >= 0 && base <= pool_elems && len <= pool_elems - base;
      const int64_t last = len > N ? len - N : 0;
      ok = ok && s <= last;
    }
    if (!ok && status && i == 0) *status = 1;
    if (i >= N) continue;
    const int64_t j = (int64_t)s + i;       // position inside the utterance; read only when ok, so 0 <= j < len
    float v = 0.0f;
    if (ok && j < len) {
      if constexpr (sizeof(T) == 2) v = (float)pool[base + j] * (1.0f / 32768.0f);   // exact: a power of two
      else v = pool[base + j];
    }
    out[(size_t)b * N + i] = v;
  }
}

hipError_t launch_data_gather(const void* pool, bool is_i16, int64_t pool_elems, const int64_t* offsets, int n_utt,
                              const int* picks, float* out, int* status, int B, int N, hipStream_t s) {
  const dim3 grid((N + 255) / 256, B < 65535 ? B : 65535);
  if (is_i16)
    hipLaunchKernelGGL(data_gather_kernel<int16_t>, grid, dim3(256), 0, s, (const int16_t*)pool, pool_elems, offsets,
                       n_utt, picks, out, status, B, N);
  else
    hipLaunchKernelGGL(data_gather_kernel<float>, grid, dim3(256), 0, s, (const float*)pool, pool_elems, offsets, n_utt,
                       picks, out, status, B, N);
  return hipGetLastError();
}

}  // namespace wg
