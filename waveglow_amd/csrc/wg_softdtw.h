// Limits, buffer layout and launch entry points of softdtw.hip, shared with softdtw_api.cpp (host).
#pragma once
#include <hip/hip_runtime.h>

#include <stddef.h>

namespace wg {

constexpr int kSdtwMaxFrames = 4096;   // frames per utterance: one row per thread slot, 1024 x 4, as the exact DTW
constexpr int kSdtwMaxFeat = 128;      // feature rows
constexpr int kSdtwCostL2 = 0, kSdtwCostSq = 1;

// The R buffer (the accumulated-cost matrix, include/waveglow_amd.h: wg_softdtw_forward) is diagonal-major and skewed:
//   R(i, j) of pair b lies at r[(b * (tmax_a + tmax_b - 1) + (i + j)) * tmax_a + i].
// The threads of the wavefront own consecutive rows i and work on one anti-diagonal i + j per step, so a step's stores
// (forward) and loads (backward) go to consecutive addresses.  Only cells with i < Ta and j < Tb are written or read.
inline size_t sdtw_r_elems(int B, int tmax_a, int tmax_b) {
  return (size_t)B * (size_t)(tmax_a + tmax_b - 1) * (size_t)tmax_a;
}

// value [B] fp64; r may be null (values only)
hipError_t launch_sdtw_forward(const float* fa, const int* frames_a, const float* fb, const int* frames_b, double gamma,
                               int cost, double* value, double* r, int B, int K, int tmax_a, int tmax_b, hipStream_t s);
// e [B][tmax_a][tmax_b] fp64, written whole: the alignment inside the frames, zeros elsewhere
hipError_t launch_sdtw_backward(const float* fa, const int* frames_a, const float* fb, const int* frames_b, double gamma,
                                int cost, const double* r, double* e, int B, int K, int tmax_a, int tmax_b, hipStream_t s);
// g_a [B][K][tmax_a] / g_b [B][K][tmax_b] fp32 from e; either may be null
hipError_t launch_sdtw_grads(const float* fa, const int* frames_a, const float* fb, const int* frames_b, int cost,
                             const double* e, const double* g_value, float* g_a, float* g_b, int B, int K, int tmax_a,
                             int tmax_b, hipStream_t s);

// ---- Sakoe-Chiba band (include/waveglow_amd.h: wg_softdtw_banded_*) ----
constexpr int kSdtwMaxBand = 511;      // 2 w + 2 threads serve a diagonal: 1024 at the widest

// The band-stored R, and E during the backward, keep S = min(2 band + 1, tmax_a) slots per anti-diagonal:
//   R(i, j) of pair b lies at r[(b * (tmax_a + tmax_b - 1) + (i + j)) * S + (i - lo_b(i + j))],
// lo_b(d) the first in-band row of diagonal d by the pair's own counts.  Only in-band cells are written or read.
inline int sdtw_band_rows(int tmax_a, int band) { return 2 * band + 1 < tmax_a ? 2 * band + 1 : tmax_a; }
inline size_t sdtw_band_elems(int B, int tmax_a, int tmax_b, int band) {
  return (size_t)B * (size_t)(tmax_a + tmax_b - 1) * (size_t)sdtw_band_rows(tmax_a, band);
}

// as launch_sdtw_forward, r in the band layout
hipError_t launch_sdtw_band_forward(const float* fa, const int* frames_a, const float* fb, const int* frames_b,
                                    double gamma, int cost, double* value, double* r, int B, int K, int tmax_a, int tmax_b,
                                    int band, hipStream_t s);
// e_band (band layout, only in-band cells written) and e (dense, written whole) may each be null
hipError_t launch_sdtw_band_backward(const float* fa, const int* frames_a, const float* fb, const int* frames_b,
                                     double gamma, int cost, const double* r, double* e_band, double* e, int B, int K,
                                     int tmax_a, int tmax_b, int band, hipStream_t s);
hipError_t launch_sdtw_band_grads(const float* fa, const int* frames_a, const float* fb, const int* frames_b, int cost,
                                  const double* e_band, const double* g_value, float* g_a, float* g_b, int B, int K,
                                  int tmax_a, int tmax_b, int band, hipStream_t s);

}  // namespace wg
