// The transpose of the device resampler (include/waveglow_amd.h: wg_resample_backward): with y = resample(x),
//   d_in[m] = sum_{n ascending} d_out[n] h[half + n down - m up]   over 0 <= n < out_len(len) with 0 <= half + n down - m up <= 2 half,
// for a ragged batch in one launch, written as a gather per input sample.  Each product is a gradient widened to fp64 (or
// fp64 as given) times an fp64 tap, the sum is fp64 in ascending n and is rounded to fp32 once.  No atomics, and no
// contraction anywhere in this file, as in resample.hip.  This file must not be built with a fast-math flag.
//
// The host hands over the taps as a second polyphase table [down][Kt], Kt = ceil((2 half + 1) / down):
//   taps_t[r][i] = h[r + i down], 0 where that index lies behind 2 half.
// With c = half - m up, r = c mod down (non-negative) and n0 = (r - c) / down (exact; negative near the start), input m is
// sum_i d_out[n0 + i] taps_t[r][i]: ascending i is ascending n, one contiguous row per input sample.  The loop runs over the
// i of the definition only (n inside [0, out_len), tap index inside [0, 2 half]), so nothing at or behind out_len(len) is read.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "wg_resample.h"

#pragma clang fp contract(off)

namespace wg {

namespace {

__device__ __forceinline__ int grad_len(const int* lens, int b, int n_in) {
  const int n = lens[b];
  return (n < 0 || n > n_in) ? 0 : n;
}

}  // namespace

// grid (ceil(n_in / kResampleTile), min(B, 65535)), 256 threads: one workgroup per (tile of kResampleTile consecutive input
// samples, utterance); thread tid owns the samples tid, tid + 256, ... of the tile.
// STAGE: the tile's span of d_out -- from n0(first) to n0(last) + Kt - 1, at most resample_grad_tile_span() <=
// kResampleGradStage values, which the host checks before it picks this variant -- is widened and staged once in LDS;
// otherwise (ratios with up / down above ~4) the gradients are read through the cache.  Which variant runs, the tile and
// the grid do not enter the arithmetic.  A tile wholly behind len only writes zeros; the branch is uniform over the
// workgroup, and so is every barrier.
template <typename T, bool STAGE>
__global__ void __launch_bounds__(256) resample_grad_kernel(const T* __restrict__ d_out, const int* __restrict__ lens,
                                                            float* __restrict__ d_in, const double* __restrict__ taps_t,
                                                            ResampleGeom g, int Kt, int B, int n_in, int n_out) {
  __shared__ double s_g[STAGE ? kResampleGradStage : 1];
  const int tid = threadIdx.x;
  const int up = g.up, down = g.down, half = g.half;
  const int64_t m0 = (int64_t)blockIdx.x * kResampleTile;
  for (int b = blockIdx.y; b < B; b += gridDim.y) {
    const int len = grad_len(lens, b, n_in);
    const int64_t olen = resample_out_len(len, up, down);
    const T* go = d_out + (size_t)b * n_out;
    float* gi = d_in + (size_t)b * n_in;
    int64_t n_base = 0;
    if (STAGE && m0 < len) {
      const int64_t m_last = (m0 + kResampleTile < len ? m0 + kResampleTile : len) - 1;
      n_base = resample_grad_first(m0, up, down, half);
      int64_t span = resample_grad_first(m_last, up, down, half) + Kt - n_base;
      if (span > kResampleGradStage) span = kResampleGradStage;                // never taken: see resample_grad_tile_span()
      for (int i = tid; i < (int)span; i += 256) {
        const int64_t n = n_base + i;
        s_g[i] = (n >= 0 && n < olen) ? (double)go[n] : 0.0;
      }
      __syncthreads();
    }
#pragma unroll 1
    for (int r = 0; r < kResampleTile / 256; ++r) {
      const int64_t m = m0 + tid + 256 * r;
      if (m >= n_in) break;
      float v = 0.0f;
      if (m < len) {
        const int64_t c = (int64_t)half - m * up;
        int64_t row = c % down;
        if (row < 0) row += down;
        const int64_t first = (row - c) / down;                                // output of i = 0
        int64_t il = first < 0 ? -first : 0;                                   // n >= 0
        int64_t ih = (2 * (int64_t)half - row) / down;                         // tap index <= 2 half (row <= half here or il > ih)
        if (2 * (int64_t)half < row) ih = -1;
        if (ih > olen - 1 - first) ih = olen - 1 - first;                      // n <= out_len - 1
        const double* tp = taps_t + (size_t)row * Kt;
        double acc = 0.0;
        for (int64_t i = il; i <= ih; ++i) {
          double gv;
          if constexpr (STAGE) {
            int64_t k = first - n_base + i;
            if (k > kResampleGradStage - 1) k = kResampleGradStage - 1;        // never taken: keeps the read inside s_g
            if (k < 0) k = 0;                                                  // never taken
            gv = s_g[k];
          } else {
            gv = (double)go[first + i];
          }
          acc = acc + gv * tp[i];
        }
        v = (float)acc;
      }
      gi[m] = v;
    }
    if (STAGE) __syncthreads();                                               // the next utterance stages anew
  }
}

// up == down == 1: the gradients themselves, rounded to fp32 if fp64, and zeros behind the length.
template <typename T>
__global__ void __launch_bounds__(256) resample_grad_copy_kernel(const T* __restrict__ d_out, const int* __restrict__ lens,
                                                                 float* __restrict__ d_in, int B, int n_in, int n_out) {
  const int64_t m = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (m >= n_in) return;
  for (int b = blockIdx.y; b < B; b += gridDim.y) {
    const int len = grad_len(lens, b, n_in);
    d_in[(size_t)b * n_in + m] = m < len ? (float)d_out[(size_t)b * n_out + m] : 0.0f;
  }
}

template <typename T>
static hipError_t launch_grad_typed(const T* d_out, const int* lens, float* d_in, const double* taps_t,
                                    const ResampleGeom& g, int Kt, int B, int n_in, int n_out, hipStream_t s) {
  const unsigned gy = B < 65535 ? B : 65535;
  if (g.up == 1 && g.down == 1) {
    hipLaunchKernelGGL(resample_grad_copy_kernel<T>, dim3((unsigned)(((int64_t)n_in + 255) / 256), gy), dim3(256), 0, s,
                       d_out, lens, d_in, B, n_in, n_out);
    return hipGetLastError();
  }
  const dim3 grid((unsigned)(((int64_t)n_in + kResampleTile - 1) / kResampleTile), gy);
  if (resample_grad_staged(g.up, g.down, Kt))
    hipLaunchKernelGGL((resample_grad_kernel<T, true>), grid, dim3(256), 0, s, d_out, lens, d_in, taps_t, g, Kt, B, n_in,
                       n_out);
  else
    hipLaunchKernelGGL((resample_grad_kernel<T, false>), grid, dim3(256), 0, s, d_out, lens, d_in, taps_t, g, Kt, B, n_in,
                       n_out);
  return hipGetLastError();
}

hipError_t launch_resample_backward(const void* d_out, bool is_f64, const int* lens, float* d_in, const double* taps_t,
                                    const ResampleGeom& g, int Kt, int B, int n_in, int n_out, hipStream_t s) {
  if (is_f64) return launch_grad_typed((const double*)d_out, lens, d_in, taps_t, g, Kt, B, n_in, n_out, s);
  return launch_grad_typed((const float*)d_out, lens, d_in, taps_t, g, Kt, B, n_in, n_out, s);
}

}  // namespace wg
