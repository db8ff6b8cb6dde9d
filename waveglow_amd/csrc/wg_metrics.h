// Limits and launch entry points of metrics.hip, shared with metrics_api.cpp (host).
#pragma once
#include <hip/hip_runtime.h>

namespace wg {

constexpr int kMetricsMaxFrames = 4096;   // frames per utterance: the DTW keeps one row per thread slot, 1024 x 4
constexpr int kMetricsMaxFeat = 128;      // mel channels / feature rows
constexpr int kMetricsRow = 8;            // fp64 values per utterance of the fused call

// basis [n_mfcc][n_mel] fp64 (workspace), filled by every call that needs it
hipError_t launch_mfcc_basis(double* basis, int n_mel, int n_mfcc, hipStream_t s);
hipError_t launch_mfcc(const float* mel, const int* frames, const double* basis, float* out, int B, int n_mel, int n_mfcc,
                       int tmax, hipStream_t s);
// rows (fused call, [B][8]) or cost / frames_out (separate entry): the one that is null is not written
hipError_t launch_dtw(const float* fa, const int* frames_a, const float* fb, const int* frames_b, double* rows,
                      double* cost, int* frames_out, int B, int K, int tmax_a, int tmax_b, hipStream_t s);
hipError_t launch_padded(const float* mel_a, const float* fa, const int* frames_a, const float* mel_b, const float* fb,
                         const int* frames_b, double* rows, int B, int n_mel, int n_mfcc, int tmax_a, int tmax_b,
                         hipStream_t s);

}  // namespace wg
