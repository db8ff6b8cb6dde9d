// Limits and launch entry point of resample.hip, shared with resample_api.cpp (host).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace wg {

constexpr int kResampleMaxRate = 1024;       // max(up, down) of the reduced ratio
constexpr int kResampleMaxIn = 1 << 26;      // n_in
constexpr int kResampleTile = 1024;          // consecutive outputs of one workgroup (256 threads x 4)
constexpr int kResampleStage = 8192;         // fp32 input samples a workgroup stages in LDS at most (32 KB)

struct ResampleGeom {
  int up, down, half;
  int K;          // taps of one polyphase row: ceil((2 half + 1) / up)
  bool clip;
};

// out_len of include/waveglow_amd.h (wg_resample): ceil(len up / down)
__host__ __device__ inline int64_t resample_out_len(int64_t len, int up, int down) {
  return (len * up + down - 1) / down;
}

// Input samples one tile of outputs can touch: q(last) - q(first) + K with q(n) = (half + n down) / up (floor).
__host__ __device__ inline int64_t resample_tile_span(int up, int down, int K) {
  return ((int64_t)(kResampleTile - 1) * down + up - 1) / up + K + 1;
}

// whether the workgroups of this ratio stage their samples in LDS (resample_kernel<T, true>) or read them through the cache
__host__ __device__ inline bool resample_staged(int up, int down, int K) {
  return resample_tile_span(up, down, K) <= kResampleStage;
}

// in [B][n_in] fp32 or int16, lens [B], taps [up][K] fp64 -> out [B][n_out] fp32 (arguments checked by resample_api.cpp)
hipError_t launch_resample(const void* in, bool is_i16, const int* lens, float* out, const double* taps,
                           const ResampleGeom& g, int B, int n_in, int n_out, hipStream_t s);

// ---- the transpose (resample_grad.hip)
constexpr int kResampleGradStage = 4096;     // fp64 output gradients a workgroup stages in LDS at most (32 KB)

// First output whose tap index half + n down - m up is not negative: ceil((m up - half) / down), negative near the start.
__host__ __device__ inline int64_t resample_grad_first(int64_t m, int up, int down, int half) {
  const int64_t c = (int64_t)half - m * up;
  int64_t row = c % down;
  if (row < 0) row += down;
  return (row - c) / down;
}

// Output gradients one tile of input samples can touch: first(last) - first(first) + Kt, Kt = ceil((2 half + 1) / down).
__host__ __device__ inline int64_t resample_grad_tile_span(int up, int down, int Kt) {
  return ((int64_t)(kResampleTile - 1) * up + down - 1) / down + Kt + 1;
}

__host__ __device__ inline bool resample_grad_staged(int up, int down, int Kt) {
  return resample_grad_tile_span(up, down, Kt) <= kResampleGradStage;
}

// d_out [B][n_out] fp32 or fp64, lens [B], taps_t [down][Kt] fp64 -> d_in [B][n_in] fp32 (arguments checked by
// resample_api.cpp)
hipError_t launch_resample_backward(const void* d_out, bool is_f64, const int* lens, float* d_in, const double* taps_t,
                                    const ResampleGeom& g, int Kt, int B, int n_in, int n_out, hipStream_t s);

}  // namespace wg
