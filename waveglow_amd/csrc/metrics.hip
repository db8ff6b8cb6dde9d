// Validation metrics of mel-spectrogram pairs on the device (src/waveglow/validation.py:211-235 and utils.py:510-523,
// restated; include/waveglow_amd.h: wg_metrics_*): MFCCs by the orthonormal DCT-II, mel-cepstral distortion of the
// zero-padded pair, exact dynamic time warping with the warped path's length carried beside its cost, and the per-channel
// cosine similarity.  Everything is fp64 arithmetic on the fp32 inputs, every sum runs in one fixed order and no kernel
// uses atomics, so a call gives the same bits every time and an utterance the same bits in any batch.
// No contraction anywhere in this file: a product and the sum it goes into are rounded separately, as a host restatement
// in numpy rounds them.  This file must not be built with a fast-math flag.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "wg_metrics.h"

#pragma clang fp contract(off)

namespace wg {

// Frame count of utterance b: a count outside [1, min(tmax, 4096)] counts as 0, so nothing is indexed past a row.
__device__ __forceinline__ int metrics_frames(const int* frames, int b, int tmax) {
  const int n = frames[b];
  const int hi = tmax < kMetricsMaxFrames ? tmax : kMetricsMaxFrames;
  return (n < 1 || n > hi) ? 0 : n;
}

// ---------------------------------------------------------------------------------------------------------------- MFCC
// basis[(k-1) * N + n] = sqrt(2/N) cos(pi k (2n+1) / (2N)), k = 1..n_mfcc
__global__ void __launch_bounds__(256) mfcc_basis_kernel(double* basis, int N, int n_mfcc) {
  const int idx = blockIdx.x * 256 + threadIdx.x;
  if (idx >= N * n_mfcc) return;
  const int k = idx / N + 1, n = idx % N;
  basis[idx] = sqrt(2.0 / (double)N) * cos(M_PI * (double)k * (double)(2 * n + 1) / (double)(2 * N));
}

// grid (ceil(tmax / 256), n_mfcc, B): one thread per output value; the basis row is the same address for the whole block.
__global__ void __launch_bounds__(256) mfcc_kernel(const float* mel, const int* frames, const double* basis, float* out,
                                                   int N, int n_mfcc, int tmax) {
  const int t = blockIdx.x * 256 + threadIdx.x, k = blockIdx.y, b = blockIdx.z;
  if (t >= tmax) return;
  const int T = metrics_frames(frames, b, tmax);
  float r = 0.0f;
  if (t < T) {
    const float* m = mel + (size_t)b * N * tmax + t;
    const double* w = basis + (size_t)k * N;
    double acc = 0.0;
    for (int n = 0; n < N; ++n) acc += (double)m[(size_t)n * tmax] * w[n];
    r = (float)acc;
  }
  out[((size_t)b * n_mfcc + k) * tmax + t] = r;
}

// ----------------------------------------------------------------------------------------------------------------- DTW
// Euclidean distance of column i of a [K][ta] and column j of b [K][tb], fp64, k ascending
__device__ __forceinline__ double dtw_dist(const float* a, const float* b, int K, int ta, int tb, int i, int j) {
  double s = 0.0;
  for (int k = 0; k < K; ++k) {
    const double d = (double)a[(size_t)k * ta + i] - (double)b[(size_t)k * tb + j];
    s += d * d;
  }
  return sqrt(s);
}

// One workgroup per pair, an anti-diagonal per step.  Thread `tid` owns rows tid * R .. tid * R + R - 1 of the cost
// matrix and keeps their cells of the last two diagonals, cost and path length, in registers; the only value another
// thread needs is the last row of its upper neighbour on the previous diagonal, which goes through LDS (two buffers, one
// barrier per step).  The distances of the next diagonal are computed before the barrier, so their loads do not sit on
// the chain cost -> minimum -> cost.  Every cell is computed by the same expression whatever R and the batch are.
template <int R>
__global__ void __launch_bounds__(1024) dtw_kernel(const float* fa, const int* frames_a, const float* fb,
                                                   const int* frames_b, double* rows, double* cost, int* frames_out,
                                                   int K, int tmax_a, int tmax_b) {
  __shared__ double s_c[2][1024];
  __shared__ int s_l[2][1024];
  const int tid = threadIdx.x, b = blockIdx.x;
  const int Ta = metrics_frames(frames_a, b, tmax_a), Tb = metrics_frames(frames_b, b, tmax_b);
  if (Ta == 0 || Tb == 0) {                                                    // the whole block leaves: no barrier follows
    if (tid == 0) {
      if (rows) rows[b * kMetricsRow + 3] = NAN, rows[b * kMetricsRow + 4] = NAN, rows[b * kMetricsRow + 5] = NAN;
      if (cost) cost[b] = NAN;
      if (frames_out) frames_out[b] = 0;
    }
    return;
  }
  const float* A = fa + (size_t)b * K * tmax_a;
  const float* Bm = fb + (size_t)b * K * tmax_b;
  const int i0 = tid * R;
  double c1[R], c2[R], dcur[R], dnext[R];          // own rows on the diagonals d-1 and d-2, distances of d and d+1
  int l1[R], l2[R];
#pragma unroll
  for (int r = 0; r < R; ++r) {
    c1[r] = c2[r] = INFINITY;
    l1[r] = l2[r] = 0;
    dcur[r] = (i0 + r == 0) ? dtw_dist(A, Bm, K, tmax_a, tmax_b, 0, 0) : 0.0;
  }
  double nc1 = INFINITY, nc2 = INFINITY;           // row i0 - 1 on the diagonals d-1 and d-2
  int nl1 = 0, nl2 = 0;
  const int nd = Ta + Tb - 1;
  for (int d = 0; d < nd; ++d) {
#pragma unroll
    for (int r = 0; r < R; ++r) {
      const int i = i0 + r, j = d + 1 - i;
      dnext[r] = (i < Ta && j >= 0 && j < Tb) ? dtw_dist(A, Bm, K, tmax_a, tmax_b, i, j) : 0.0;
    }
    if (d > 0 && tid > 0) nc1 = s_c[(d - 1) & 1][tid - 1], nl1 = s_l[(d - 1) & 1][tid - 1];
#pragma unroll
    for (int r = R - 1; r >= 0; --r) {             // descending: row r - 1 still holds the previous diagonals
      const int i = i0 + r, j = d - i;
      const double up = r > 0 ? c1[r > 0 ? r - 1 : 0] : nc1, dg = r > 0 ? c2[r > 0 ? r - 1 : 0] : nc2, lf = c1[r];
      const int upl = r > 0 ? l1[r > 0 ? r - 1 : 0] : nl1, dgl = r > 0 ? l2[r > 0 ? r - 1 : 0] : nl2, lfl = l1[r];
      double best = up;                            // (i-1, j), then (i, j-1), then (i-1, j-1): the first minimum wins
      int bl = upl;
      if (lf < best) best = lf, bl = lfl;
      if (dg < best) best = dg, bl = dgl;
      double c = dcur[r] + best;
      int l = bl + 1;
      if (i == 0 && j == 0) c = dcur[r], l = 1;
      if (!(i < Ta && j >= 0 && j < Tb)) c = INFINITY, l = 0;
      c2[r] = c1[r], l2[r] = l1[r];
      c1[r] = c, l1[r] = l;
    }
    nc2 = nc1, nl2 = nl1;
    s_c[d & 1][tid] = c1[R - 1];
    s_l[d & 1][tid] = l1[R - 1];
    __syncthreads();
#pragma unroll
    for (int r = 0; r < R; ++r) dcur[r] = dnext[r];
  }
#pragma unroll
  for (int r = 0; r < R; ++r)
    if (i0 + r == Ta - 1) {                        // cell (Ta-1, Tb-1) lies on the last diagonal
      const double c = c1[r];
      const int l = l1[r];
      if (rows) {
        double* o = rows + (size_t)b * kMetricsRow;
        o[3] = c / (double)l;
        o[4] = 2.0 - (double)(Ta + Tb) / (double)l;
        o[5] = (double)l;
      }
      if (cost) cost[b] = c;
      if (frames_out) frames_out[b] = l;
    }
}

// ------------------------------------------------------------------------------------- zero-padded MCD and cosine score
__device__ __forceinline__ double wave_sum(double v) {
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) v += __shfl_xor(v, d);
  return v;
}

// grid B, 256 threads.  MCD: thread tid sums the frame distances of frames tid, tid + 256, ... ascending, the 256 partial
// sums are joined by a tree in LDS.  Cosine: wave w takes the channels w, w + 4, ...; a lane sums its frames ascending,
// the lanes are joined by a butterfly, the channel scores are summed ascending by one thread.
__global__ void __launch_bounds__(256) padded_kernel(const float* mel_a, const float* fa, const int* frames_a,
                                                     const float* mel_b, const float* fb, const int* frames_b,
                                                     double* rows, int n_mel, int n_mfcc, int tmax_a, int tmax_b) {
  __shared__ double s_part[256];
  __shared__ double s_score[kMetricsMaxFeat];
  const int tid = threadIdx.x, b = blockIdx.x;
  const int Ta = metrics_frames(frames_a, b, tmax_a), Tb = metrics_frames(frames_b, b, tmax_b);
  double* o = rows + (size_t)b * kMetricsRow;
  if (Ta == 0 || Tb == 0) {
    if (tid == 0) o[0] = NAN, o[1] = NAN, o[2] = NAN, o[6] = NAN, o[7] = 0.0;
    return;
  }
  const int F = Ta > Tb ? Ta : Tb;
  const float* A = fa + (size_t)b * n_mfcc * tmax_a;
  const float* Bm = fb + (size_t)b * n_mfcc * tmax_b;
  double acc = 0.0;
  for (int t = tid; t < F; t += 256) {
    double s = 0.0;
    for (int k = 0; k < n_mfcc; ++k) {
      const double x = t < Ta ? (double)A[(size_t)k * tmax_a + t] : 0.0;
      const double y = t < Tb ? (double)Bm[(size_t)k * tmax_b + t] : 0.0;
      const double d = x - y;
      s += d * d;
    }
    acc += sqrt(s);
  }
  s_part[tid] = acc;
  const int lane = tid & 63, wave = tid >> 6;
  const float* U = mel_a + (size_t)b * n_mel * tmax_a;
  const float* V = mel_b + (size_t)b * n_mel * tmax_b;
  for (int c = wave; c < n_mel; c += 4) {
    double uv = 0.0, uu = 0.0, vv = 0.0;
    for (int t = lane; t < F; t += 64) {
      const double u = t < Ta ? (double)U[(size_t)c * tmax_a + t] : 0.0;
      const double v = t < Tb ? (double)V[(size_t)c * tmax_b + t] : 0.0;
      uv += u * v;
      uu += u * u;
      vv += v * v;
    }
    uv = wave_sum(uv), uu = wave_sum(uu), vv = wave_sum(vv);
    const double den = sqrt(uu) * sqrt(vv);
    if (lane == 0) s_score[c] = den == 0.0 ? 1.0 : 1.0 - uv / den;          // utils.py:517-518: a NaN score counts as 1
  }
  __syncthreads();
  for (int w = 128; w >= 1; w >>= 1) {
    if (tid < w) s_part[tid] += s_part[tid + w];
    __syncthreads();
  }
  if (tid == 0) {
    double sc = 0.0;
    for (int c = 0; c < n_mel; ++c) sc += s_score[c];
    o[0] = s_part[0] / (double)F;
    o[1] = 2.0 - (double)(Ta + Tb) / (double)F;
    o[2] = (double)F;
    o[6] = 1.0 - sc / (double)n_mel;
    o[7] = 0.0;
  }
}

// --------------------------------------------------------------------------------------------------------------- launch
hipError_t launch_mfcc_basis(double* basis, int n_mel, int n_mfcc, hipStream_t s) {
  hipLaunchKernelGGL(mfcc_basis_kernel, dim3((n_mel * n_mfcc + 255) / 256), dim3(256), 0, s, basis, n_mel, n_mfcc);
  return hipGetLastError();
}

hipError_t launch_mfcc(const float* mel, const int* frames, const double* basis, float* out, int B, int n_mel, int n_mfcc,
                       int tmax, hipStream_t s) {
  hipLaunchKernelGGL(mfcc_kernel, dim3((tmax + 255) / 256, n_mfcc, B), dim3(256), 0, s, mel, frames, basis, out, n_mel,
                     n_mfcc, tmax);
  return hipGetLastError();
}

hipError_t launch_dtw(const float* fa, const int* frames_a, const float* fb, const int* frames_b, double* rows,
                      double* cost, int* frames_out, int B, int K, int tmax_a, int tmax_b, hipStream_t s) {
  const int R = (tmax_a + 1023) / 1024;                              // rows per thread, 1..4
  const int threads = ((tmax_a + R - 1) / R + 63) / 64 * 64;         // whole waves that cover tmax_a rows
#define WG_DTW(RR)                                                                                                  \
  hipLaunchKernelGGL(dtw_kernel<RR>, dim3(B), dim3(threads), 0, s, fa, frames_a, fb, frames_b, rows, cost, frames_out, \
                     K, tmax_a, tmax_b)
  switch (R) {
    case 1: WG_DTW(1); break;
    case 2: WG_DTW(2); break;
    case 3: WG_DTW(3); break;
    case 4: WG_DTW(4); break;
    default: return hipErrorInvalidValue;
  }
#undef WG_DTW
  return hipGetLastError();
}

hipError_t launch_padded(const float* mel_a, const float* fa, const int* frames_a, const float* mel_b, const float* fb,
                         const int* frames_b, double* rows, int B, int n_mel, int n_mfcc, int tmax_a, int tmax_b,
                         hipStream_t s) {
  hipLaunchKernelGGL(padded_kernel, dim3(B), dim3(256), 0, s, mel_a, fa, frames_a, mel_b, fb, frames_b, rows, n_mel, n_mfcc,
                     tmax_a, tmax_b);
  return hipGetLastError();
}

}  // namespace wg
