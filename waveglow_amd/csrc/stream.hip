// The two memory kernels of a streaming step (include/waveglow_amd.h: wg_stream_gather, wg_stream_emit).  A step over B
// streams runs one window per stream through wg_infer and the denoiser as a ragged batch; stream_gather_kernel forms the
// padded batch tensors of those windows out of the streams' own mel and noise buffers in ONE launch (instead of
// 2 + n_early slice copies and as many zero fills per stream), stream_emit_kernel crops the chunks out of the window
// audio, converts them to int16 and reduces their statistics in ONE launch (instead of a crop, two extrema and a count
// per stream).  Plain loads and stores, no LDS staging: a window is read once and written once.
// The int16 conversion is numpy's float32 arithmetic restated (convert_wav of audio_utils.py:36-64 on np.clip(y * gain, -1,
// 1)), as in wav.hip: this file must not be built with a fast-math flag.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "wg_stream.h"

namespace wg {

// Elements are copied as bits: uint32_t for fp32, uint16_t for fp16.
template <typename T>
union StreamPiece {
  T e[16 / sizeof(T)];
  uint4 v;
};

// grid (gx, 2 + n_early, B), 256 threads.  Plane 0 is the mel, plane 1 z_init, plane 2 + i z_early[i]; every workgroup
// strides over the whole destination row block of its plane, so each destination element is written exactly once.
// The window's frame count is clamped to [0, w_max] and to what the source pitch holds behind its start: nothing outside
// [0, pitch) of a source row is read whatever the table holds.
template <typename T>
__global__ void __launch_bounds__(256) stream_gather_kernel(const wg_stream_window* __restrict__ windows,
                                                            StreamGatherDst dst, int n_mel, int n_mel_out, int n_rem,
                                                            int n_es, int w_max, int cpf) {
  const int b = blockIdx.z, p = blockIdx.y;
  const wg_stream_window* w = windows + b;
  const int64_t start = w->start;
  int64_t n = w->count;
  if (start < 0 || n < 0) n = 0;
  if (n > w_max) n = w_max;
  const int first = blockIdx.x * 256 + threadIdx.x, step = gridDim.x * 256;
  if (p == 0) {
    const int64_t pitch = w->mel_pitch;
    if (start + n > pitch) n = pitch > start ? pitch - start : 0;
    const T* src = (const T*)w->mel + start;
    T* out = (T*)dst.mel + (size_t)b * n_mel_out * w_max;
    const int total = n_mel_out * w_max;
    for (int i = first; i < total; i += step) {
      const int m = i / w_max, f = i - m * w_max;
      T v = 0;
      if (m < n_mel && f < n) v = src[(int64_t)m * pitch + f];      // a mel window starts at any frame: element loads
      out[i] = v;
    }
    return;
  }
  constexpr int VE = 16 / sizeof(T);
  const int ch = p == 1 ? n_rem : n_es;
  const T* src = (const T*)(p == 1 ? w->z_init : w->z_early[p - 2]);
  const int lw = cpf * w_max, vper = lw / VE;                       // cpf is a multiple of 8: whole 16-byte pieces
  T* out = (T*)(p == 1 ? dst.z_init : dst.z_early[p - 2]) + (size_t)b * ch * lw;
  const int64_t pitch = w->noise_pitch, c0 = (int64_t)cpf * start;
  if (c0 + cpf * n > pitch) n = pitch > c0 ? (pitch - c0) / cpf : 0;
  const int64_t cols = cpf * n;                                     // a multiple of VE: a piece is inside the window or behind it
  src += c0;                                                        // cpf * sizeof(T) is a multiple of 16: alignment is the base's
  const bool wide = ((((uintptr_t)src) | (uintptr_t)(pitch * (int64_t)sizeof(T))) & 15) == 0;
  const int total = ch * vper;
  for (int i = first; i < total; i += step) {
    const int c = i / vper, col = (i - c * vper) * VE;
    StreamPiece<T> x;
    x.v = make_uint4(0, 0, 0, 0);
    if (col < cols) {
      const T* s = src + (int64_t)c * pitch + col;
      if (wide) {
        x.v = *(const uint4*)s;
      } else {
#pragma unroll
        for (int k = 0; k < VE; ++k) x.e[k] = s[k];
      }
    }
    *(uint4*)(out + (size_t)c * lw + col) = x.v;
  }
}

hipError_t launch_stream_gather(const wg_stream_window* windows, const StreamGatherDst& dst, int n_early, int B, int n_mel,
                                int n_mel_out, int n_rem, int n_early_size, int w_max, int cpf, bool is_f16,
                                hipStream_t s) {
  // enough workgroups per plane that a thread moves a few pieces of the largest plane, at most 64
  const int64_t most = (int64_t)(n_rem > n_early_size ? n_rem : n_early_size) * cpf * w_max / 4;
  int gx = (int)((most + 4 * 256 - 1) / (4 * 256));
  gx = gx < 1 ? 1 : (gx > 64 ? 64 : gx);
  const dim3 grid(gx, 2 + n_early, B);
  if (is_f16)
    hipLaunchKernelGGL(stream_gather_kernel<uint16_t>, grid, dim3(256), 0, s, windows, dst, n_mel, n_mel_out, n_rem,
                       n_early_size, w_max, cpf);
  else
    hipLaunchKernelGGL(stream_gather_kernel<uint32_t>, grid, dim3(256), 0, s, windows, dst, n_mel, n_mel_out, n_rem,
                       n_early_size, w_max, cpf);
  return hipGetLastError();
}

struct StreamRange {
  float rmin, rmax, dmin, dmax, bad;   // raw and denoised extrema; bad > 0 when a sample is NaN or infinite
  int clipped;                         // samples the clip to [-1, 1] changed
};

__device__ __forceinline__ void stream_join(StreamRange& r, const StreamRange& o) {
  r.rmin = fminf(r.rmin, o.rmin);
  r.rmax = fmaxf(r.rmax, o.rmax);
  r.dmin = fminf(r.dmin, o.dmin);
  r.dmax = fmaxf(r.dmax, o.dmax);
  r.bad = fmaxf(r.bad, o.bad);
  r.clipped += o.clipped;
}

// grid (B), kStreamEmitThreads threads x 8 samples per round: one workgroup per row, so that the statistics of a row are
// joined inside the launch (wave shuffles, then the waves through LDS) -- a chunk is some thousand samples.
__global__ void __launch_bounds__(kStreamEmitThreads) stream_emit_kernel(const wg_stream_crop* __restrict__ crops,
                                                                         int16_t* __restrict__ pcm,
                                                                         float* __restrict__ stats, int n_max) {
  constexpr int kWaves = kStreamEmitThreads / 64;
  __shared__ StreamRange sw[kWaves];
  const int tid = threadIdx.x, b = blockIdx.x;
  const wg_stream_crop* c = crops + b;
  int n = c->count;
  int off = c->offset;
  if (off < 0 || n < 0) n = 0, off = 0;
  if (n > n_max) n = n_max;
  const float gain = c->gain;
  const float* rp = c->raw + off;
  const float* dp = c->denoised + off;
  const bool wide = (((uintptr_t)rp | (uintptr_t)dp) & 15) == 0;
  StreamRange r{INFINITY, -INFINITY, INFINITY, -INFINITY, 0.0f, 0};
  for (int i = tid * 8; i < n_max; i += kStreamEmitThreads * 8) {     // n_max is a multiple of 8
    float x[8], y[8];
    if (wide && i + 8 <= n) {
      const float4 xa = *(const float4*)(rp + i), xb = *(const float4*)(rp + i + 4);
      const float4 ya = *(const float4*)(dp + i), yb = *(const float4*)(dp + i + 4);
      x[0] = xa.x, x[1] = xa.y, x[2] = xa.z, x[3] = xa.w, x[4] = xb.x, x[5] = xb.y, x[6] = xb.z, x[7] = xb.w;
      y[0] = ya.x, y[1] = ya.y, y[2] = ya.z, y[3] = ya.w, y[4] = yb.x, y[5] = yb.y, y[6] = yb.z, y[7] = yb.w;
    } else {
#pragma unroll
      for (int k = 0; k < 8; ++k) {
        x[k] = i + k < n ? rp[i + k] : 0.0f;
        y[k] = i + k < n ? dp[i + k] : 0.0f;
      }
    }
    union {
      int16_t h[8];
      uint4 v;
    } out;
#pragma unroll
    for (int k = 0; k < 8; ++k) {
      const bool in = i + k < n;
      const float g = y[k] * gain;                                      // denoised * gain (float32)
      if (in) {
        r.rmin = fminf(r.rmin, x[k]);
        r.rmax = fmaxf(r.rmax, x[k]);
        r.dmin = fminf(r.dmin, y[k]);
        r.dmax = fmaxf(r.dmax, y[k]);
        if (!isfinite(x[k]) || !isfinite(y[k])) r.bad = 1.0f;
        if (g > 1.0f || g < -1.0f) r.clipped += 1;
      }
      const float q = fminf(fmaxf(g, -1.0f), 1.0f);                     // np.clip(g, -1, 1); NaN -> a defined value
      const float v = rintf((q / 1.0f) * 32767.0f);                     // np.round(wav / -min * 32767, 0)
      out.h[k] = in ? (int16_t)(int)v : (int16_t)0;
    }
    *(uint4*)(pcm + (size_t)b * n_max + i) = out.v;
  }
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) {
    StreamRange o;
    o.rmin = __shfl_xor(r.rmin, d);
    o.rmax = __shfl_xor(r.rmax, d);
    o.dmin = __shfl_xor(r.dmin, d);
    o.dmax = __shfl_xor(r.dmax, d);
    o.bad = __shfl_xor(r.bad, d);
    o.clipped = __shfl_xor(r.clipped, d);
    stream_join(r, o);
  }
  if ((tid & 63) == 0) sw[tid >> 6] = r;
  __syncthreads();
  if (tid == 0) {
#pragma unroll
    for (int k = 1; k < kWaves; ++k) stream_join(r, sw[k]);
    float* o = stats + (size_t)b * kStreamStats;
    const bool any = n > 0;
    o[0] = any ? r.rmin : 0.0f, o[1] = any ? r.rmax : 0.0f, o[2] = any ? r.dmin : 0.0f, o[3] = any ? r.dmax : 0.0f;
    o[4] = (float)r.clipped, o[5] = r.bad, o[6] = 0.0f, o[7] = 0.0f;
  }
}

hipError_t launch_stream_emit(const wg_stream_crop* crops, int16_t* pcm, float* stats, int B, int n_max, hipStream_t s) {
  hipLaunchKernelGGL(stream_emit_kernel, dim3(B), dim3(kStreamEmitThreads), 0, s, crops, pcm, stats, n_max);
  return hipGetLastError();
}

}  // namespace wg
