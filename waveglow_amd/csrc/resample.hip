// Rational-ratio resampling on the device (include/waveglow_amd.h: wg_resample): scipy.signal.resample_poly(x, up, down)
// with its defaults in closed form,
//   y[n] = sum_{m ascending} x[m] h[half + n down - m up]     over 0 <= m < len with 0 <= half + n down - m up <= 2 half,
// for a ragged batch in one launch.  The reference has no counterpart; the definition is stated in the header and in
// DESIGN.md section 7.  Each product is an fp32 sample widened to fp64 times an fp64 tap, the sum is fp64 in ascending m
// and is rounded to fp32 once.  No atomics, and no contraction anywhere in this file: a product and the sum it goes into
// are rounded separately, as a host restatement in numpy rounds them.  This file must not be built with a fast-math flag.
//
// The host hands over the taps as a polyphase table [up][K], K = ceil((2 half + 1) / up), with every row REVERSED:
//   taps[p][j] = h[p + (K - 1 - j) up], 0 where that index lies behind 2 half.
// With P = half + n down, p = P mod up and q = P / up, output n is sum_j x[q - (K - 1) + j] taps[p][j]: ascending j is
// ascending m, one contiguous row per output.  The loop runs over the j of the definition only (m inside [0, len), tap
// index inside [0, 2 half]), so a sample behind the length is never read and never multiplied by a filler zero.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "wg_resample.h"

#pragma clang fp contract(off)

namespace wg {

// Sample count of utterance b: a length outside [0, n_in] counts as 0, so nothing is read past a row.
__device__ __forceinline__ int resample_len(const int* lens, int b, int n_in) {
  const int n = lens[b];
  return (n < 0 || n > n_in) ? 0 : n;
}

__device__ __forceinline__ float pcm_to_float(float v) { return v; }
__device__ __forceinline__ float pcm_to_float(int16_t v) { return (float)v * (1.0f / 32768.0f); }   // exact: a power of two

__device__ __forceinline__ float clip_unit(float y) { return y < -1.0f ? -1.0f : (y > 1.0f ? 1.0f : y); }   // NaN stays NaN

// grid (ceil(n_out / kResampleTile), min(B, 65535)), 256 threads: one workgroup per (tile of kResampleTile consecutive
// outputs, utterance); thread tid owns the outputs tid, tid + 256, ... of the tile, so a wave stores 64 neighbours.
// STAGE: the tile's input span -- from sample q(first) - (K - 1) to q(last), at most resample_tile_span() <= kResampleStage
// samples, which the host checks before it picks this variant -- is converted and staged once in LDS; otherwise (ratios
// with down / up above ~7) the samples are read through the cache.  The taps are read through the cache in both: the
// table of the largest ratios (164 KB) does not fit beside the samples.  Which variant runs, the tile and the grid do not
// enter the arithmetic: an output's terms and their order depend on n, len and the ratio alone.
// A tile wholly behind out_len(len) only writes zeros; the branch is uniform over the workgroup, and so is every barrier.
template <typename T, bool STAGE>
__global__ void __launch_bounds__(256) resample_kernel(const T* __restrict__ in, const int* __restrict__ lens,
                                                       float* __restrict__ out, const double* __restrict__ taps,
                                                       ResampleGeom g, int B, int n_in, int n_out) {
  __shared__ float s_x[STAGE ? kResampleStage : 1];
  const int tid = threadIdx.x;
  const int up = g.up, down = g.down, half = g.half, K = g.K;
  const int64_t n0 = (int64_t)blockIdx.x * kResampleTile;
  for (int b = blockIdx.y; b < B; b += gridDim.y) {
    const int len = resample_len(lens, b, n_in);
    const int64_t olen = resample_out_len(len, up, down);
    const T* x = in + (size_t)b * n_in;
    float* y = out + (size_t)b * n_out;
    int64_t m_base = 0;
    if (STAGE && n0 < olen) {
      const int64_t n_last = (n0 + kResampleTile < olen ? n0 + kResampleTile : olen) - 1;
      m_base = (half + n0 * down) / up - (K - 1);
      int64_t span = (half + n_last * down) / up - m_base + 1;
      if (span > kResampleStage) span = kResampleStage;                       // never taken: see resample_tile_span()
      for (int i = tid; i < (int)span; i += 256) {
        const int64_t m = m_base + i;
        s_x[i] = (m >= 0 && m < len) ? pcm_to_float(x[m]) : 0.0f;
      }
      __syncthreads();
    }
#pragma unroll 1
    for (int r = 0; r < kResampleTile / 256; ++r) {
      const int64_t n = n0 + tid + 256 * r;
      if (n >= n_out) break;
      float v = 0.0f;
      if (n < olen) {
        const int64_t P = half + n * down;
        const int p = (int)(P % up);
        const int64_t q = P / up;
        const int64_t first = q - (K - 1);                                     // sample of j = 0
        int64_t jl = first < 0 ? -first : 0;                                   // m >= 0
        const int64_t jt = 2 * half >= p ? K - 1 - (2 * half - p) / up : K;    // tap index <= 2 half
        if (jt > jl) jl = jt;
        int64_t jh = (int64_t)len - 1 - first;                                 // m <= len - 1
        if (jh > K - 1) jh = K - 1;
        const double* tp = taps + (size_t)p * K;
        double acc = 0.0;
        for (int64_t j = jl; j <= jh; ++j) {
          float xs;
          if constexpr (STAGE) {
            int64_t i = first - m_base + j;
            if (i > kResampleStage - 1) i = kResampleStage - 1;                // never taken: keeps the read inside s_x
            xs = s_x[i];
          } else {
            xs = pcm_to_float(x[first + j]);
          }
          acc = acc + (double)xs * tp[j];
        }
        v = (float)acc;
        if (g.clip) v = clip_unit(v);
      }
      y[n] = v;
    }
    if (STAGE) __syncthreads();                                               // the next utterance stages anew
  }
}

// up == down == 1: the samples themselves (converted if int16) and zeros behind the length -- a copy, so that the bits
// of the input come back (-0 included, which 0 + x 1 would turn into +0).
template <typename T>
__global__ void __launch_bounds__(256) resample_copy_kernel(const T* __restrict__ in, const int* __restrict__ lens,
                                                            float* __restrict__ out, bool clip, int B, int n_in,
                                                            int n_out) {
  const int64_t n = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (n >= n_out) return;
  for (int b = blockIdx.y; b < B; b += gridDim.y) {
    const int len = resample_len(lens, b, n_in);
    float v = 0.0f;
    if (n < len) {
      v = pcm_to_float(in[(size_t)b * n_in + n]);
      if (clip) v = clip_unit(v);
    }
    out[(size_t)b * n_out + n] = v;
  }
}

template <typename T>
static hipError_t launch_typed(const T* in, const int* lens, float* out, const double* taps, const ResampleGeom& g, int B,
                               int n_in, int n_out, hipStream_t s) {
  const unsigned gy = B < 65535 ? B : 65535;
  if (g.up == 1 && g.down == 1) {
    hipLaunchKernelGGL(resample_copy_kernel<T>, dim3((unsigned)(((int64_t)n_out + 255) / 256), gy), dim3(256), 0, s, in,
                       lens, out, g.clip, B, n_in, n_out);
    return hipGetLastError();
  }
  const dim3 grid((unsigned)(((int64_t)n_out + kResampleTile - 1) / kResampleTile), gy);      // 64-bit: n_out may be 2^31 - 1
  if (resample_staged(g.up, g.down, g.K))
    hipLaunchKernelGGL((resample_kernel<T, true>), grid, dim3(256), 0, s, in, lens, out, taps, g, B, n_in, n_out);
  else
    hipLaunchKernelGGL((resample_kernel<T, false>), grid, dim3(256), 0, s, in, lens, out, taps, g, B, n_in, n_out);
  return hipGetLastError();
}

hipError_t launch_resample(const void* in, bool is_i16, const int* lens, float* out, const double* taps,
                           const ResampleGeom& g, int B, int n_in, int n_out, hipStream_t s) {
  if (is_i16) return launch_typed((const int16_t*)in, lens, out, taps, g, B, n_in, n_out, s);
  return launch_typed((const float*)in, lens, out, taps, g, B, n_in, n_out, s);
}

}  // namespace wg
