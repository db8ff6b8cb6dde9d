// PCM finishing of a synthesised batch on the device: what the host did per utterance with is_overamp on the raw audio
// (src/waveglow/audio_utils.py:132-138) and convert_wav(normalize_wav(denoised), int16) (audio_utils.py:36-64, :67-95).
// Two launches: wav_stats_kernel reduces minimum / maximum of both signals per chunk, wav_pcm_kernel joins the chunks of
// its utterance, scales by the peak and rounds to int16.  Minimum and maximum do not depend on the order of the reduction,
// and the scaling is numpy's float32 arithmetic restated (IEEE division, round half to even): the int16 samples are the
// host functions' bit for bit.  This file must not be built with a fast-math flag.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "wg_host.h"

namespace wg {

constexpr int kWavParts = 64;          // chunks per utterance = lanes of the wave that joins them
constexpr int kWavStats = 8;           // floats per utterance in stats_out, and per chunk in the workspace

// Sample count of utterance b, clamped to the row: nothing is indexed past the pitch whatever lens holds.
__device__ __forceinline__ int wav_len(const int* lens, int b, int N) {
  const int n = lens[b];
  return n < 0 ? 0 : (n > N ? N : n);
}

struct WavRange {
  float rmin, rmax, dmin, dmax, bad;   // raw and denoised extrema; bad > 0 when a sample is NaN or infinite
};

__device__ __forceinline__ void wav_join(WavRange& r, const WavRange& o) {
  r.rmin = fminf(r.rmin, o.rmin);
  r.rmax = fmaxf(r.rmax, o.rmax);
  r.dmin = fminf(r.dmin, o.dmin);
  r.dmax = fmaxf(r.dmax, o.dmax);
  r.bad = fmaxf(r.bad, o.bad);
}

__device__ __forceinline__ WavRange wav_wave_join(WavRange r) {
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) {
    WavRange o;
    o.rmin = __shfl_xor(r.rmin, d);
    o.rmax = __shfl_xor(r.rmax, d);
    o.dmin = __shfl_xor(r.dmin, d);
    o.dmax = __shfl_xor(r.dmax, d);
    o.bad = __shfl_xor(r.bad, d);
    wav_join(r, o);
  }
  return r;
}

__device__ __forceinline__ void wav_take(WavRange& r, float x, float y) {
  r.rmin = fminf(r.rmin, x);
  r.rmax = fmaxf(r.rmax, x);
  r.dmin = fminf(r.dmin, y);
  r.dmax = fmaxf(r.dmax, y);
  if (!isfinite(x) || !isfinite(y)) r.bad = 1.0f;
}

// grid (kWavParts, B), 256 threads: chunk p of utterance b covers samples [p * chunk, (p + 1) * chunk) below lens[b];
// chunk is a multiple of 4 and so is N, so a float4 never leaves the row.
__global__ void __launch_bounds__(256) wav_stats_kernel(const float* raw, const float* den, const int* lens, float* part,
                                                        int N, int chunk) {
  __shared__ WavRange sw[4];
  const int tid = threadIdx.x, p = blockIdx.x, b = blockIdx.y;
  const int n = wav_len(lens, b, N);
  const int lo = p * chunk, hi = min(lo + chunk, n);
  const float* rp = raw + (size_t)b * N;
  const float* dp = den + (size_t)b * N;
  WavRange r{INFINITY, -INFINITY, INFINITY, -INFINITY, 0.0f};
  for (int i = lo + 4 * tid; i < hi; i += 4 * 256) {
    const float4 x = *(const float4*)(rp + i), y = *(const float4*)(dp + i);
    wav_take(r, x.x, y.x);
    if (i + 1 < hi) wav_take(r, x.y, y.y);
    if (i + 2 < hi) wav_take(r, x.z, y.z);
    if (i + 3 < hi) wav_take(r, x.w, y.w);
  }
  r = wav_wave_join(r);
  if ((tid & 63) == 0) sw[tid >> 6] = r;
  __syncthreads();
  if (tid == 0) {
    wav_join(r, sw[1]);
    wav_join(r, sw[2]);
    wav_join(r, sw[3]);
    float* o = part + ((size_t)b * kWavParts + p) * kWavStats;
    o[0] = r.rmin, o[1] = r.rmax, o[2] = r.dmin, o[3] = r.dmax, o[4] = r.bad;
  }
}

// grid (ceil(N / 2048), B), 256 threads x 8 samples.  Every block joins the chunks of its utterance (64 x 5 floats) and
// block 0 also writes them out: stats[b] = {raw min, raw max, raw peak, denoised min, denoised max, denoised peak,
// non-finite flag, 0}, peak = max |x| = max(-min, max).  An utterance without samples has all of them 0.
__global__ void __launch_bounds__(256) wav_pcm_kernel(const float* den, const int* lens, const float* part, int16_t* pcm,
                                                      float* stats, int N) {
  __shared__ float s_peak;
  const int tid = threadIdx.x, b = blockIdx.y;
  const int n = wav_len(lens, b, N);
  if (tid < 64) {
    const float* q = part + ((size_t)b * kWavParts + tid) * kWavStats;
    WavRange r = wav_wave_join(WavRange{q[0], q[1], q[2], q[3], q[4]});
    if (n == 0) r = WavRange{0.0f, 0.0f, 0.0f, 0.0f, 0.0f};
    const float peak = fmaxf(-r.dmin, r.dmax);
    if (tid == 0) {
      s_peak = peak;
      if (blockIdx.x == 0) {
        float* o = stats + (size_t)b * kWavStats;
        o[0] = r.rmin, o[1] = r.rmax, o[2] = fmaxf(-r.rmin, r.rmax);
        o[3] = r.dmin, o[4] = r.dmax, o[5] = peak;
        o[6] = r.bad, o[7] = 0.0f;
      }
    }
  }
  __syncthreads();
  const int i = (blockIdx.x * 256 + tid) * 8;
  if (i >= N) return;
  const float peak = s_peak;
  const bool scale = peak != 1.0f && peak != 0.0f;      // normalize_wav: max_val != hi and max_val != 0
  const float* dp = den + (size_t)b * N + i;
  const float4 xa = *(const float4*)dp, xb = *(const float4*)(dp + 4);
  const float x[8] = {xa.x, xa.y, xa.z, xa.w, xb.x, xb.y, xb.z, xb.w};
  union {
    int16_t h[8];
    uint4 v;
  } out;
#pragma unroll
  for (int k = 0; k < 8; ++k) {
    const float y = scale ? (x[k] * 1.0f) / peak : x[k];                  // wav.astype(float32) * hi / max_val
    float v = rintf((y / 1.0f) * 32767.0f);                               // np.round(wav / -min * 32767, 0)
    v = fmaxf(fminf(v, 32767.0f), -32768.0f);                             // no-op for finite input; NaN -> a defined value
    out.h[k] = i + k < n ? (int16_t)(int)v : (int16_t)0;
  }
  *(uint4*)(pcm + (size_t)b * N + i) = out.v;
}

}  // namespace wg

extern "C" {

size_t wg_wav_finish_workspace_bytes(int32_t B) {
  return B < 1 ? 0 : (size_t)B * wg::kWavParts * wg::kWavStats * sizeof(float);
}

int wg_wav_finish(const float* raw, const float* denoised, const int32_t* lens, int16_t* pcm_out, float* stats_out,
                  int32_t B, int32_t n_samples, void* workspace, size_t workspace_bytes, void* stream) {
  using namespace wg;
  if (!raw || !denoised || !lens || !pcm_out || !stats_out || !workspace) return fail(WG_ERR_INVALID, "null argument");
  if (B < 1 || n_samples < 8 || n_samples % 8) return fail(WG_ERR_INVALID, "wav finish: B >= 1, n_samples a multiple of 8");
  if (((uintptr_t)raw | (uintptr_t)denoised | (uintptr_t)pcm_out) & 15)
    return fail(WG_ERR_INVALID, "wav finish: audio and pcm must be 16-byte aligned");
  if (workspace_bytes < wg_wav_finish_workspace_bytes(B)) return fail(WG_ERR_WORKSPACE, "wav finish workspace too small");
  hipStream_t s = (hipStream_t)stream;
  const int chunk = ((n_samples + kWavParts - 1) / kWavParts + 3) / 4 * 4;
  hipLaunchKernelGGL(wav_stats_kernel, dim3(kWavParts, B), dim3(256), 0, s, raw, denoised, lens, (float*)workspace,
                     n_samples, chunk);
  HIP_TRY(hipGetLastError());
  hipLaunchKernelGGL(wav_pcm_kernel, dim3((n_samples + 2047) / 2048, B), dim3(256), 0, s, denoised, lens,
                     (const float*)workspace, pcm_out, stats_out, n_samples);
  HIP_TRY(hipGetLastError());
  return WG_OK;
}

}  // extern "C"
