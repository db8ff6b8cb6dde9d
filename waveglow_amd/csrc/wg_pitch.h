// Limits and launch entry points of pitch.hip, shared with pitch_api.cpp (host).
#pragma once
#include <hip/hip_runtime.h>

namespace wg {

constexpr int kPitchMinFrame = 16;      // frame_length W
constexpr int kPitchMaxFrame = 2048;
constexpr int kPitchMaxTau = 1024;      // tau_max: 256 threads x at most 4 lags each
constexpr int kPitchRow = 8;            // fp64 values per pair of wg_pitch_compare

struct PitchGeom {
  double sr, threshold;
  int W, H, tau_min, tau_max;
};

// F(len) of include/waveglow_amd.h (wg_pitch_*): frames of `len` samples, 0 where len < W + tau_max
__host__ __device__ inline int pitch_frames(int len, int W, int H, int tau_max) {
  return len >= W + tau_max ? (len - W - tau_max) / H + 1 : 0;
}

// audio [B][N] fp32, lens [B] -> f0, ap [B][fmax] fp64, frames_out [B]; fmax >= max(1, pitch_frames(N))
hipError_t launch_yin(const float* audio, const int* lens, double* f0, double* ap, int* frames_out, const PitchGeom& g,
                      int B, int N, int fmax, hipStream_t s);
hipError_t launch_pitch_compare(const double* f0_a, const int* frames_a, const double* f0_b, const int* frames_b,
                                double* rows, int B, int fmax_a, int fmax_b, hipStream_t s);

}  // namespace wg
