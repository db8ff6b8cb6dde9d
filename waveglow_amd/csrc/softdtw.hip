// Soft dynamic time warping of feature pairs on the device (Cuturi and Blondel, "Soft-DTW: a differentiable loss function
// for time-series", ICML 2017; include/waveglow_amd.h: wg_softdtw_*): the smoothed form of metrics.hip's exact DTW, with
// the accumulated-cost matrix R kept by the forward, the expected alignment E by the backward (Algorithm 2 of the paper)
// and the gradients of both feature sets from E.  Everything is fp64 arithmetic on the fp32 inputs, every sum runs in one
// fixed order and no kernel uses atomics, so a call gives the same bits every time and an utterance the same bits in any
// batch.  No contraction in this file: the frame distance is the expression of metrics.hip's dtw_dist, rounded the same
// way; where a fused multiply-add is wanted it is written as fma().  This file must not be built with a fast-math flag.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "wg_softdtw.h"

#pragma clang fp contract(off)

namespace wg {

// Frame count of utterance b: a count outside [1, min(tmax, 4096)] counts as 0, so nothing is indexed past a row.
__device__ __forceinline__ int sdtw_frames(const int* frames, int b, int tmax) {
  const int n = frames[b];
  const int hi = tmax < kSdtwMaxFrames ? tmax : kSdtwMaxFrames;
  return (n < 1 || n > hi) ? 0 : n;
}

// sum_k ascending (a[k][i] - b[k][j])^2 of column i of a [K][ta] and column j of b [K][tb]; its root for the L2 cost
template <bool SQ>
__device__ __forceinline__ double sdtw_dist(const float* a, const float* b, int K, int ta, int tb, int i, int j) {
  double s = 0.0;
  for (int k = 0; k < K; ++k) {
    const double d = (double)a[(size_t)k * ta + i] - (double)b[(size_t)k * tb + j];
    s += d * d;
  }
  return SQ ? s : sqrt(s);
}

// m - gamma log(sum_q exp(-(x_q - m) / gamma)), m = min x, the terms in the order given; +infinity stands for a cell
// outside the matrix and contributes an exact 0 by predicate.  The division is a product with 1 / gamma.
__device__ __forceinline__ double sdtw_softmin(double x0, double x1, double x2, double gamma, double inv_gamma) {
  double m = x0;
  if (x1 < m) m = x1;
  if (x2 < m) m = x2;
  const double e0 = x0 == INFINITY ? 0.0 : exp((m - x0) * inv_gamma);
  const double e1 = x1 == INFINITY ? 0.0 : exp((m - x1) * inv_gamma);
  const double e2 = x2 == INFINITY ? 0.0 : exp((m - x2) * inv_gamma);
  return m - gamma * log((e0 + e1) + e2);
}

// ------------------------------------------------------------------------------------------------------------- forward
// One workgroup per pair, an anti-diagonal per step: dtw_kernel's scheme.  Thread `tid` owns rows tid * R .. tid * R + R - 1
// of the matrix and keeps their cells of the last two diagonals in registers; the last row of its upper neighbour on the
// previous diagonal goes through LDS (two buffers, one barrier per step).  The distances of the next diagonal are computed
// before the barrier, so their loads do not sit on the chain cost -> softmin -> cost.  Every cell is computed by the same
// expression whatever R and the batch are.  With `rbuf` every cell inside the frames is stored (layout: wg_softdtw.h).
template <int R, bool SQ>
__global__ void __launch_bounds__(1024) sdtw_forward_kernel(const float* fa, const int* frames_a, const float* fb,
                                                            const int* frames_b, double gamma, double inv_gamma,
                                                            double* value, double* rbuf, int K, int tmax_a, int tmax_b) {
  __shared__ double s_c[2][1024];
  const int tid = threadIdx.x, b = blockIdx.x;
  const int Ta = sdtw_frames(frames_a, b, tmax_a), Tb = sdtw_frames(frames_b, b, tmax_b);
  if (Ta == 0 || Tb == 0) {                                                    // the whole block leaves: no barrier follows
    if (tid == 0) value[b] = NAN;
    return;
  }
  const float* A = fa + (size_t)b * K * tmax_a;
  const float* Bm = fb + (size_t)b * K * tmax_b;
  double* Rb = rbuf ? rbuf + (size_t)b * (size_t)(tmax_a + tmax_b - 1) * tmax_a : nullptr;
  const int i0 = tid * R;
  double c1[R], c2[R], dcur[R], dnext[R];          // own rows on the diagonals d-1 and d-2, distances of d and d+1
#pragma unroll
  for (int r = 0; r < R; ++r) {
    c1[r] = c2[r] = INFINITY;
    dcur[r] = (i0 + r == 0) ? sdtw_dist<SQ>(A, Bm, K, tmax_a, tmax_b, 0, 0) : 0.0;
  }
  double nc1 = INFINITY, nc2 = INFINITY;           // row i0 - 1 on the diagonals d-1 and d-2
  const int nd = Ta + Tb - 1;
  for (int d = 0; d < nd; ++d) {
#pragma unroll
    for (int r = 0; r < R; ++r) {
      const int i = i0 + r, j = d + 1 - i;
      dnext[r] = (i < Ta && j >= 0 && j < Tb) ? sdtw_dist<SQ>(A, Bm, K, tmax_a, tmax_b, i, j) : 0.0;
    }
    if (d > 0 && tid > 0) nc1 = s_c[(d - 1) & 1][tid - 1];
#pragma unroll
    for (int r = R - 1; r >= 0; --r) {             // descending: row r - 1 still holds the previous diagonals
      const int i = i0 + r, j = d - i;
      const double up = r > 0 ? c1[r > 0 ? r - 1 : 0] : nc1, dg = r > 0 ? c2[r > 0 ? r - 1 : 0] : nc2, lf = c1[r];
      double c = dcur[r] + sdtw_softmin(up, lf, dg, gamma, inv_gamma);       // (i-1, j), (i, j-1), (i-1, j-1)
      if (i == 0 && j == 0) c = dcur[r];
      const bool inside = i < Ta && j >= 0 && j < Tb;
      if (!inside) c = INFINITY;
      if (inside && Rb) Rb[(size_t)d * tmax_a + i] = c;
      c2[r] = c1[r];
      c1[r] = c;
    }
    nc2 = nc1;
    s_c[d & 1][tid] = c1[R - 1];
    __syncthreads();
#pragma unroll
    for (int r = 0; r < R; ++r) dcur[r] = dnext[r];
  }
#pragma unroll
  for (int r = 0; r < R; ++r)
    if (i0 + r == Ta - 1) value[b] = c1[r];        // cell (Ta-1, Tb-1) lies on the last diagonal
}

// ------------------------------------------------------------------------------------------------------------ backward
// The same ownership, descending diagonals.  With Q(s) = R(s) - d(s) a term of E(i,j) is E(s) exp((Q(s) - R(i,j)) / gamma),
// so a thread keeps E and Q of its rows on the diagonals d+1 and d+2, and the first row of its lower neighbour on d+1 goes
// through LDS (two values, two buffers, one barrier per step).  R of the next diagonal (d-1) is loaded and its distances
// are recomputed before the barrier.  A term whose successor lies outside the matrix is left out by predicate; cells
// outside hold zeros, never infinities, so nothing here forms inf - inf.  E inside the frames is written row-major; the
// launcher has zeroed the whole of E before.  With four rows per thread (more than 3072 rows) the values fetched ahead do
// not fit the registers of a 1024-thread workgroup: there a diagonal's R and distances are fetched at the head of its step.
template <int R, bool SQ>
__global__ void __launch_bounds__(1024) sdtw_backward_kernel(const float* fa, const int* frames_a, const float* fb,
                                                             const int* frames_b, double inv_gamma, const double* rbuf,
                                                             double* e_out, int K, int tmax_a, int tmax_b) {
  __shared__ double s_e[2][1024], s_q[2][1024];
  const int tid = threadIdx.x, b = blockIdx.x;
  const int Ta = sdtw_frames(frames_a, b, tmax_a), Tb = sdtw_frames(frames_b, b, tmax_b);
  if (Ta == 0 || Tb == 0) return;                                              // the whole block leaves; E stays zero
  const float* A = fa + (size_t)b * K * tmax_a;
  const float* Bm = fb + (size_t)b * K * tmax_b;
  const double* Rb = rbuf + (size_t)b * (size_t)(tmax_a + tmax_b - 1) * tmax_a;
  double* Eo = e_out + (size_t)b * tmax_a * tmax_b;
  const int i0 = tid * R;
  const bool has_lower = tid + 1 < (int)blockDim.x;
  const int nd = Ta + Tb - 1;
  constexpr bool kAhead = R < 4;
  constexpr int RN = kAhead ? R : 1;
  double e1[R], e2[R], q1[R], q2[R];               // own rows on the diagonals d+1 and d+2
  double rcur[R], qcur[R], rnext[RN], qnext[RN];   // R and Q of the diagonals d and d-1
#pragma unroll
  for (int r = 0; r < R; ++r) {
    e1[r] = e2[r] = q1[r] = q2[r] = 0.0;
    const int i = i0 + r, j = nd - 1 - i;
    const bool inside = kAhead && i < Ta && j >= 0 && j < Tb;
    rcur[r] = inside ? Rb[(size_t)(nd - 1) * tmax_a + i] : 0.0;
    qcur[r] = inside ? rcur[r] - sdtw_dist<SQ>(A, Bm, K, tmax_a, tmax_b, i, j) : 0.0;
  }
  double ne1 = 0.0, nq1 = 0.0, ne2 = 0.0, nq2 = 0.0;   // row i0 + R on the diagonals d+1 and d+2
  for (int d = nd - 1; d >= 0; --d) {
#pragma unroll
    for (int r = 0; r < R; ++r) {
      const int dl = kAhead ? d - 1 : d;           // the diagonal fetched in this step
      const int i = i0 + r, j = dl - i;
      const bool inside = i < Ta && j >= 0 && j < Tb;
      const double rv = inside ? Rb[(size_t)dl * tmax_a + i] : 0.0;
      const double qv = inside ? rv - sdtw_dist<SQ>(A, Bm, K, tmax_a, tmax_b, i, j) : 0.0;
      if (kAhead) rnext[r < RN ? r : 0] = rv, qnext[r < RN ? r : 0] = qv;
      else rcur[r] = rv, qcur[r] = qv;
    }
    if (d < nd - 1 && has_lower) ne1 = s_e[(d + 1) & 1][tid + 1], nq1 = s_q[(d + 1) & 1][tid + 1];
#pragma unroll
    for (int r = 0; r < R; ++r) {                  // ascending: row r + 1 still holds the later diagonals
      const int i = i0 + r, j = d - i;
      const bool last = r == R - 1;
      const int rn = last ? 0 : r + 1;
      const double e_dn = last ? ne1 : e1[rn], q_dn = last ? nq1 : q1[rn];   // (i+1, j)
      const double e_dg = last ? ne2 : e2[rn], q_dg = last ? nq2 : q2[rn];   // (i+1, j+1)
      const double e_rt = e1[r], q_rt = q1[r];                               // (i, j+1)
      const bool inside = i < Ta && j >= 0 && j < Tb;
      const double rc = rcur[r];
      double e = 0.0;
      if (inside) {
        const bool below = i + 1 < Ta, right = j + 1 < Tb;
        if (below) e += e_dn * exp((q_dn - rc) * inv_gamma);
        if (right) e += e_rt * exp((q_rt - rc) * inv_gamma);
        if (below && right) e += e_dg * exp((q_dg - rc) * inv_gamma);
        if (!below && !right) e = 1.0;             // cell (Ta-1, Tb-1)
        Eo[(size_t)i * tmax_b + j] = e;
      }
      e2[r] = e1[r], q2[r] = q1[r];
      e1[r] = e, q1[r] = qcur[r];
    }
    ne2 = ne1, nq2 = nq1;
    s_e[d & 1][tid] = e1[0];
    s_q[d & 1][tid] = q1[0];
    __syncthreads();
    if (kAhead) {
#pragma unroll
      for (int r = 0; r < R; ++r) rcur[r] = rnext[r < RN ? r : 0], qcur[r] = qnext[r < RN ? r : 0];
    }
  }
}

// --------------------------------------------------------------------------------------------------- feature gradients
constexpr int kSdtwKc = 16;                        // feature rows per pass: the accumulators of a pass stay in registers

__device__ __forceinline__ double sdtw_wave_sum(double v) {
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) v += __shfl_xor(v, d);
  return v;
}

// E(i,j) times d(d(i,j)) / d(a[k][i]) without its factor (a[k][i] - b[k][j]): E / d for L2 (0 where d = 0), 2 E for SQ
template <bool SQ>
__device__ __forceinline__ double sdtw_weight(double e, double s) {
  if (SQ) return 2.0 * e;
  return s > 0.0 ? e / sqrt(s) : 0.0;
}

// g_a: grid (B, ceil(tmax_a / 4)), 256 threads, one wave per row i.  Lane l sums its columns j = l, l + 64, ... ascending,
// the 64 partial sums are joined by a butterfly: the order depends on Tb alone.  Rows behind Ta are written as zeros.
template <bool SQ>
__global__ void __launch_bounds__(256) sdtw_grad_a_kernel(const float* fa, const int* frames_a, const float* fb,
                                                          const int* frames_b, const double* e_in, const double* g_value,
                                                          float* g_a, int K, int tmax_a, int tmax_b) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, b = blockIdx.x;
  const int i = blockIdx.y * 4 + wave;
  if (i >= tmax_a) return;
  const int Ta = sdtw_frames(frames_a, b, tmax_a), Tb = sdtw_frames(frames_b, b, tmax_b);
  float* out = g_a + (size_t)b * K * tmax_a + i;
  if (Ta == 0 || Tb == 0 || i >= Ta) {
    for (int k = lane; k < K; k += 64) out[(size_t)k * tmax_a] = 0.0f;
    return;
  }
  const float* A = fa + (size_t)b * K * tmax_a + i;
  const float* Bm = fb + (size_t)b * K * tmax_b;
  const double* E = e_in + ((size_t)b * tmax_a + i) * tmax_b;
  const double gv = g_value[b];
  for (int kc = 0; kc < K; kc += kSdtwKc) {
    double acc[kSdtwKc];
#pragma unroll
    for (int c = 0; c < kSdtwKc; ++c) acc[c] = 0.0;
    for (int j = lane; j < Tb; j += 64) {
      double s = 0.0;
      for (int k = 0; k < K; ++k) {
        const double d = (double)A[(size_t)k * tmax_a] - (double)Bm[(size_t)k * tmax_b + j];
        s += d * d;
      }
      const double w = sdtw_weight<SQ>(E[j], s);
#pragma unroll
      for (int c = 0; c < kSdtwKc; ++c)
        if (kc + c < K)
          acc[c] = fma(w, (double)A[(size_t)(kc + c) * tmax_a] - (double)Bm[(size_t)(kc + c) * tmax_b + j], acc[c]);
    }
#pragma unroll
    for (int c = 0; c < kSdtwKc; ++c) {
      const double v = sdtw_wave_sum(acc[c]);
      if (lane == 0 && kc + c < K) out[(size_t)(kc + c) * tmax_a] = (float)(gv * v);
    }
  }
}

// g_b: grid (B, ceil(tmax_b / 64)), 512 threads: lane l of every wave holds column j = 64 * blockIdx.y + l, so E is read
// along its rows.  Wave w sums the rows i = w, w + 8, ... ascending; the eight partial sums of a column are joined through
// LDS by a fixed tree, ((0+1)+(2+3))+((4+5)+(6+7)): the order depends on Ta alone.  Columns behind Tb are written as zeros.
constexpr int kSdtwGbWaves = 8;
static_assert(kSdtwKc / 2 == kSdtwGbWaves, "wave w joins accumulator w of a half");

template <bool SQ>
__global__ void __launch_bounds__(64 * kSdtwGbWaves) sdtw_grad_b_kernel(const float* fa, const int* frames_a,
                                                                        const float* fb, const int* frames_b,
                                                                        const double* e_in, const double* g_value,
                                                                        float* g_b, int K, int tmax_a, int tmax_b) {
  __shared__ double s_part[kSdtwGbWaves][kSdtwKc / 2][64];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, b = blockIdx.x;
  const int j = blockIdx.y * 64 + lane;
  const bool live = j < tmax_b;                    // a column of the buffer
  const int Ta = sdtw_frames(frames_a, b, tmax_a), Tb = sdtw_frames(frames_b, b, tmax_b);
  float* out = g_b + (size_t)b * K * tmax_b + j;
  if (Ta == 0 || Tb == 0 || (int)blockIdx.y * 64 >= Tb) {                      // the whole block leaves: no barrier follows
    if (live)
      for (int k = wave; k < K; k += kSdtwGbWaves) out[(size_t)k * tmax_b] = 0.0f;
    return;
  }
  const bool inside = j < Tb;
  const int jc = inside ? j : 0;                   // a lane behind Tb works on column 0 and writes zeros
  const float* A = fa + (size_t)b * K * tmax_a;
  const float* Bm = fb + (size_t)b * K * tmax_b + jc;
  const double* E = e_in + (size_t)b * tmax_a * tmax_b + jc;
  const double gv = g_value[b];
  for (int kc = 0; kc < K; kc += kSdtwKc) {
    double acc[kSdtwKc];
#pragma unroll
    for (int c = 0; c < kSdtwKc; ++c) acc[c] = 0.0;
    for (int i = wave; i < Ta; i += kSdtwGbWaves) {
      double s = 0.0;
      for (int k = 0; k < K; ++k) {
        const double d = (double)A[(size_t)k * tmax_a + i] - (double)Bm[(size_t)k * tmax_b];
        s += d * d;
      }
      const double w = sdtw_weight<SQ>(E[(size_t)i * tmax_b], s);
#pragma unroll
      for (int c = 0; c < kSdtwKc; ++c)
        if (kc + c < K)
          acc[c] = fma(w, (double)Bm[(size_t)(kc + c) * tmax_b] - (double)A[(size_t)(kc + c) * tmax_a + i], acc[c]);
    }
#pragma unroll
    for (int half = 0; half < 2; ++half) {         // eight accumulators at a time: wave w joins accumulator w
#pragma unroll
      for (int c = 0; c < kSdtwKc / 2; ++c) s_part[wave][c][lane] = acc[half * (kSdtwKc / 2) + c];
      __syncthreads();
      const double v = ((s_part[0][wave][lane] + s_part[1][wave][lane]) + (s_part[2][wave][lane] + s_part[3][wave][lane])) +
                       ((s_part[4][wave][lane] + s_part[5][wave][lane]) + (s_part[6][wave][lane] + s_part[7][wave][lane]));
      const int k = kc + half * (kSdtwKc / 2) + wave;
      if (live && k < K) out[(size_t)k * tmax_b] = inside ? (float)(gv * v) : 0.0f;
      __syncthreads();
    }
  }
}

// --------------------------------------------------------------------------------------------------------------- launch
namespace {
inline int sdtw_rows(int tmax_a) { return (tmax_a + 1023) / 1024; }                  // rows per thread, 1..4
inline int sdtw_threads(int tmax_a, int R) { return ((tmax_a + R - 1) / R + 63) / 64 * 64; }   // whole waves
}  // namespace

hipError_t launch_sdtw_forward(const float* fa, const int* frames_a, const float* fb, const int* frames_b, double gamma,
                               int cost, double* value, double* r, int B, int K, int tmax_a, int tmax_b, hipStream_t s) {
  const int R = sdtw_rows(tmax_a), threads = sdtw_threads(tmax_a, R);
  const double inv_gamma = 1.0 / gamma;
#define WG_SDTW(RR)                                                                                                     \
  if (cost == kSdtwCostSq)                                                                                              \
    hipLaunchKernelGGL((sdtw_forward_kernel<RR, true>), dim3(B), dim3(threads), 0, s, fa, frames_a, fb, frames_b, gamma, \
                       inv_gamma, value, r, K, tmax_a, tmax_b);                                                         \
  else                                                                                                                  \
    hipLaunchKernelGGL((sdtw_forward_kernel<RR, false>), dim3(B), dim3(threads), 0, s, fa, frames_a, fb, frames_b, gamma, \
                       inv_gamma, value, r, K, tmax_a, tmax_b)
  switch (R) {
    case 1: WG_SDTW(1); break;
    case 2: WG_SDTW(2); break;
    case 3: WG_SDTW(3); break;
    case 4: WG_SDTW(4); break;
    default: return hipErrorInvalidValue;
  }
#undef WG_SDTW
  return hipGetLastError();
}

hipError_t launch_sdtw_backward(const float* fa, const int* frames_a, const float* fb, const int* frames_b, double gamma,
                                int cost, const double* r, double* e, int B, int K, int tmax_a, int tmax_b, hipStream_t s) {
  const int R = sdtw_rows(tmax_a), threads = sdtw_threads(tmax_a, R);
  const double inv_gamma = 1.0 / gamma;
  hipError_t err = hipMemsetAsync(e, 0, (size_t)B * tmax_a * tmax_b * sizeof(double), s);
  if (err != hipSuccess) return err;
#define WG_SDTW(RR)                                                                                                     \
  if (cost == kSdtwCostSq)                                                                                              \
    hipLaunchKernelGGL((sdtw_backward_kernel<RR, true>), dim3(B), dim3(threads), 0, s, fa, frames_a, fb, frames_b,      \
                       inv_gamma, r, e, K, tmax_a, tmax_b);                                                             \
  else                                                                                                                  \
    hipLaunchKernelGGL((sdtw_backward_kernel<RR, false>), dim3(B), dim3(threads), 0, s, fa, frames_a, fb, frames_b,     \
                       inv_gamma, r, e, K, tmax_a, tmax_b)
  switch (R) {
    case 1: WG_SDTW(1); break;
    case 2: WG_SDTW(2); break;
    case 3: WG_SDTW(3); break;
    case 4: WG_SDTW(4); break;
    default: return hipErrorInvalidValue;
  }
#undef WG_SDTW
  return hipGetLastError();
}

hipError_t launch_sdtw_grads(const float* fa, const int* frames_a, const float* fb, const int* frames_b, int cost,
                             const double* e, const double* g_value, float* g_a, float* g_b, int B, int K, int tmax_a,
                             int tmax_b, hipStream_t s) {
  const bool sq = cost == kSdtwCostSq;
  if (g_a) {
    const dim3 grid(B, (tmax_a + 3) / 4);
    if (sq)
      hipLaunchKernelGGL(sdtw_grad_a_kernel<true>, grid, dim3(256), 0, s, fa, frames_a, fb, frames_b, e, g_value, g_a, K,
                         tmax_a, tmax_b);
    else
      hipLaunchKernelGGL(sdtw_grad_a_kernel<false>, grid, dim3(256), 0, s, fa, frames_a, fb, frames_b, e, g_value, g_a, K,
                         tmax_a, tmax_b);
    const hipError_t err = hipGetLastError();
    if (err != hipSuccess) return err;
  }
  if (g_b) {
    const dim3 grid(B, (tmax_b + 63) / 64);
    if (sq)
      hipLaunchKernelGGL(sdtw_grad_b_kernel<true>, grid, dim3(64 * kSdtwGbWaves), 0, s, fa, frames_a, fb, frames_b, e,
                         g_value, g_b, K, tmax_a, tmax_b);
    else
      hipLaunchKernelGGL(sdtw_grad_b_kernel<false>, grid, dim3(64 * kSdtwGbWaves), 0, s, fa, frames_a, fb, frames_b, e,
                         g_value, g_b, K, tmax_a, tmax_b);
  }
  return hipGetLastError();
}

// ===================================================================================================== Sakoe-Chiba band
// The same recursions with the cells outside the band |i m - j n| <= W counting as +infinity (include/waveglow_amd.h:
// wg_softdtw_banded_*).  On an anti-diagonal the band is the row interval lo(d) .. hi(d) of at most 2 w + 1 rows, and both
// ends advance by 0 or 1 per diagonal, so the wavefront needs no more threads than the band is wide.
struct SdtwBand {
  int n, m, W, nm;                                 // Ta - 1, Tb - 1, w max(n, m), max(n + m, 1)
};

__device__ __forceinline__ SdtwBand sdtw_band(int Ta, int Tb, int w) {
  SdtwBand g;
  g.n = Ta - 1, g.m = Tb - 1;
  g.W = w * (g.n > g.m ? g.n : g.m);
  g.nm = g.n + g.m > 0 ? g.n + g.m : 1;
  return g;
}

__device__ __forceinline__ int sdtw_floordiv(int a, int b) {                   // b > 0
  const int q = a / b;
  return (a % b != 0 && a < 0) ? q - 1 : q;
}
__device__ __forceinline__ int sdtw_ceildiv(int a, int b) { return -sdtw_floordiv(-a, b); }
__device__ __forceinline__ int sdtw_max(int a, int b) { return a > b ? a : b; }
__device__ __forceinline__ int sdtw_min(int a, int b) { return a < b ? a : b; }

// first and last in-band row of the anti-diagonal d, 0 <= d <= n + m
__device__ __forceinline__ int sdtw_band_lo(const SdtwBand& g, int d) {
  return sdtw_max(sdtw_max(0, d - g.m), sdtw_ceildiv(d * g.n - g.W, g.nm));
}
__device__ __forceinline__ int sdtw_band_hi(const SdtwBand& g, int d) {
  return sdtw_min(sdtw_min(g.n, d), sdtw_floordiv(d * g.n + g.W, g.nm));
}
// E or R of the in-band cell (i, j) in the band layout of wg_softdtw.h, relative to the pair's first element
__device__ __forceinline__ size_t sdtw_band_at(const SdtwBand& g, int S, int i, int j) {
  return (size_t)(i + j) * S + (i - sdtw_band_lo(g, i + j));
}

// Forward.  One workgroup of P threads per pair, P a power of two > 2 w + 1: on every diagonal thread t serves the one row
// i = t (mod P) of the interval, if there is one.  A row that enters the band needs its upper neighbour's cells of the two
// diagonals before, which another thread computed while this one served another row or none, so nothing is carried in
// registers: the last three diagonals live in LDS, slot i mod P holding R(i, d - i) and +infinity where the interval has
// no such row.  Every thread writes its slot on every step, so a buffer describes its whole diagonal; row i - 1 of the
// diagonals d - 1 and d - 2 is the only row those intervals can hold in slot (i - 1) mod P, because the intervals of three
// consecutive diagonals span at most 2 w + 3 <= P + 1 rows and row i - 1 +- P lies outside them.  Three buffers, so the
// buffer written on step d + 1 was last read before the barrier of step d: one barrier per step.  The cell itself is the
// dense kernel's expression.
template <bool SQ>
__global__ void __launch_bounds__(1024) sdtw_band_forward_kernel(const float* fa, const int* frames_a, const float* fb,
                                                                 const int* frames_b, double gamma, double inv_gamma,
                                                                 double* value, double* rbuf, int K, int tmax_a,
                                                                 int tmax_b, int w, int S) {
  __shared__ double s_c[3][1024];
  const int tid = threadIdx.x, b = blockIdx.x, mask = (int)blockDim.x - 1;
  const int Ta = sdtw_frames(frames_a, b, tmax_a), Tb = sdtw_frames(frames_b, b, tmax_b);
  if (Ta == 0 || Tb == 0) {                                                    // the whole block leaves: no barrier follows
    if (tid == 0) value[b] = NAN;
    return;
  }
  const SdtwBand g = sdtw_band(Ta, Tb, w);
  const float* A = fa + (size_t)b * K * tmax_a;
  const float* Bm = fb + (size_t)b * K * tmax_b;
  double* Rb = rbuf ? rbuf + (size_t)b * (size_t)(tmax_a + tmax_b - 1) * S : nullptr;
  const int nd = Ta + Tb - 1;
  int lo = 0, hi = 0;                                                          // the interval of diagonal 0
  double dcur = tid == 0 ? sdtw_dist<SQ>(A, Bm, K, tmax_a, tmax_b, 0, 0) : 0.0;
  int cur = 0, prev1 = 2, prev2 = 1;                                           // buffers of the diagonals d, d-1, d-2
  for (int d = 0; d < nd; ++d) {
    int lo_n = 0, hi_n = -1;                                                   // the interval of d + 1; empty behind the end
    if (d + 1 < nd) lo_n = sdtw_band_lo(g, d + 1), hi_n = sdtw_band_hi(g, d + 1);
    const int i_n = lo_n + ((tid - lo_n) & mask);
    const double dnext = i_n <= hi_n ? sdtw_dist<SQ>(A, Bm, K, tmax_a, tmax_b, i_n, d + 1 - i_n) : 0.0;
    const int i = lo + ((tid - lo) & mask);
    double c = INFINITY;
    if (i <= hi) {
      const double up = (i > 0 && d > 0) ? s_c[prev1][(i - 1) & mask] : INFINITY;      // (i-1, j)
      const double lf = d > 0 ? s_c[prev1][tid] : INFINITY;                            // (i, j-1)
      const double dg = (i > 0 && d > 1) ? s_c[prev2][(i - 1) & mask] : INFINITY;      // (i-1, j-1)
      c = dcur + sdtw_softmin(up, lf, dg, gamma, inv_gamma);
      if (d == 0) c = dcur;
      if (Rb) Rb[(size_t)d * S + (i - lo)] = c;
      if (d == nd - 1) value[b] = c;               // cell (Ta-1, Tb-1) is the last diagonal
    }
    s_c[cur][tid] = c;
    __syncthreads();
    const int t = prev2;
    prev2 = prev1, prev1 = cur, cur = t;
    dcur = dnext, lo = lo_n, hi = hi_n;
  }
}

// Backward: the mirror image, descending diagonals, E and Q = R - d of the last three diagonals in LDS with zeros where
// the interval has no row.  A successor outside the band or the matrix is left out by predicate, as in the dense kernel.
// E goes to the band layout (e_band, for the gradient kernels) and to the dense e_out (zeroed by the launcher), each if
// it is given.  R and the distances of the next diagonal are fetched before the barrier.
template <bool SQ>
__global__ void __launch_bounds__(1024) sdtw_band_backward_kernel(const float* fa, const int* frames_a, const float* fb,
                                                                  const int* frames_b, double inv_gamma,
                                                                  const double* rbuf, double* e_band, double* e_out, int K,
                                                                  int tmax_a, int tmax_b, int w, int S) {
  __shared__ double s_e[3][1024], s_q[3][1024];
  const int tid = threadIdx.x, b = blockIdx.x, mask = (int)blockDim.x - 1;
  const int Ta = sdtw_frames(frames_a, b, tmax_a), Tb = sdtw_frames(frames_b, b, tmax_b);
  if (Ta == 0 || Tb == 0) return;                                              // the whole block leaves; e_out stays zero
  const SdtwBand g = sdtw_band(Ta, Tb, w);
  const float* A = fa + (size_t)b * K * tmax_a;
  const float* Bm = fb + (size_t)b * K * tmax_b;
  const size_t pair = (size_t)b * (size_t)(tmax_a + tmax_b - 1) * S;
  const double* Rb = rbuf + pair;
  double* Eb = e_band ? e_band + pair : nullptr;
  double* Eo = e_out ? e_out + (size_t)b * tmax_a * tmax_b : nullptr;
  const int nd = Ta + Tb - 1;
  int lo = sdtw_band_lo(g, nd - 1), hi = sdtw_band_hi(g, nd - 1);
  int lo1 = 0, hi1 = -1, lo2 = 0, hi2 = -1;                                    // the intervals of d + 1 and d + 2
  double rcur = 0.0, qcur = 0.0;
  {
    const int i = lo + ((tid - lo) & mask);
    if (i <= hi) {
      rcur = Rb[(size_t)(nd - 1) * S + (i - lo)];
      qcur = rcur - sdtw_dist<SQ>(A, Bm, K, tmax_a, tmax_b, i, nd - 1 - i);
    }
  }
  int cur = 0, next1 = 2, next2 = 1;                                           // buffers of the diagonals d, d+1, d+2
  for (int d = nd - 1; d >= 0; --d) {
    int lo_p = 0, hi_p = -1;                                                   // the interval of d - 1
    if (d > 0) lo_p = sdtw_band_lo(g, d - 1), hi_p = sdtw_band_hi(g, d - 1);
    const int i_p = lo_p + ((tid - lo_p) & mask);
    double rnext = 0.0, qnext = 0.0;
    if (i_p <= hi_p) {
      rnext = Rb[(size_t)(d - 1) * S + (i_p - lo_p)];
      qnext = rnext - sdtw_dist<SQ>(A, Bm, K, tmax_a, tmax_b, i_p, d - 1 - i_p);
    }
    const int i = lo + ((tid - lo) & mask), j = d - i;
    double e = 0.0, q = 0.0;
    if (i <= hi) {
      const bool below = i + 1 >= lo1 && i + 1 <= hi1;                         // (i+1, j) in the band
      const bool right = i >= lo1 && i <= hi1;                                 // (i, j+1)
      const bool diag = i + 1 >= lo2 && i + 1 <= hi2;                          // (i+1, j+1)
      const int sn = (i + 1) & mask;
      const double rc = rcur;
      if (below) e += s_e[next1][sn] * exp((s_q[next1][sn] - rc) * inv_gamma);
      if (right) e += s_e[next1][tid] * exp((s_q[next1][tid] - rc) * inv_gamma);
      if (diag) e += s_e[next2][sn] * exp((s_q[next2][sn] - rc) * inv_gamma);
      if (d == nd - 1) e = 1.0;                    // cell (Ta-1, Tb-1)
      if (Eb) Eb[(size_t)d * S + (i - lo)] = e;
      if (Eo) Eo[(size_t)i * tmax_b + j] = e;
      q = qcur;
    }
    s_e[cur][tid] = e;
    s_q[cur][tid] = q;
    __syncthreads();
    const int t = next2;
    next2 = next1, next1 = cur, cur = t;
    lo2 = lo1, hi2 = hi1, lo1 = lo, hi1 = hi, lo = lo_p, hi = hi_p;
    rcur = rnext, qcur = qnext;
  }
}

// g_a and g_b from the band-layout E: the dense kernels' sums with the cells outside the band left out, so a lane starts
// at its first column (row) inside the band and stops behind the last; the order of what remains is unchanged.
template <bool SQ>
__global__ void __launch_bounds__(256) sdtw_band_grad_a_kernel(const float* fa, const int* frames_a, const float* fb,
                                                               const int* frames_b, const double* e_band,
                                                               const double* g_value, float* g_a, int K, int tmax_a,
                                                               int tmax_b, int w, int S) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, b = blockIdx.x;
  const int i = blockIdx.y * 4 + wave;
  if (i >= tmax_a) return;
  const int Ta = sdtw_frames(frames_a, b, tmax_a), Tb = sdtw_frames(frames_b, b, tmax_b);
  float* out = g_a + (size_t)b * K * tmax_a + i;
  if (Ta == 0 || Tb == 0 || i >= Ta) {
    for (int k = lane; k < K; k += 64) out[(size_t)k * tmax_a] = 0.0f;
    return;
  }
  const SdtwBand g = sdtw_band(Ta, Tb, w);
  const float* A = fa + (size_t)b * K * tmax_a + i;
  const float* Bm = fb + (size_t)b * K * tmax_b;
  const double* E = e_band + (size_t)b * (size_t)(tmax_a + tmax_b - 1) * S;
  const double gv = g_value[b];
  int jlo = 0, jhi = g.m;                                                      // the columns of row i inside the band
  if (g.n > 0) jlo = sdtw_max(0, sdtw_ceildiv(i * g.m - g.W, g.n)), jhi = sdtw_min(g.m, sdtw_floordiv(i * g.m + g.W, g.n));
  const int j0 = jlo > lane ? lane + ((jlo - lane + 63) >> 6 << 6) : lane;
  for (int kc = 0; kc < K; kc += kSdtwKc) {
    double acc[kSdtwKc];
#pragma unroll
    for (int c = 0; c < kSdtwKc; ++c) acc[c] = 0.0;
    for (int j = j0; j <= jhi; j += 64) {
      double s = 0.0;
      for (int k = 0; k < K; ++k) {
        const double d = (double)A[(size_t)k * tmax_a] - (double)Bm[(size_t)k * tmax_b + j];
        s += d * d;
      }
      const double wt = sdtw_weight<SQ>(E[sdtw_band_at(g, S, i, j)], s);
#pragma unroll
      for (int c = 0; c < kSdtwKc; ++c)
        if (kc + c < K)
          acc[c] = fma(wt, (double)A[(size_t)(kc + c) * tmax_a] - (double)Bm[(size_t)(kc + c) * tmax_b + j], acc[c]);
    }
#pragma unroll
    for (int c = 0; c < kSdtwKc; ++c) {
      const double v = sdtw_wave_sum(acc[c]);
      if (lane == 0 && kc + c < K) out[(size_t)(kc + c) * tmax_a] = (float)(gv * v);
    }
  }
}

template <bool SQ>
__global__ void __launch_bounds__(64 * kSdtwGbWaves) sdtw_band_grad_b_kernel(const float* fa, const int* frames_a,
                                                                             const float* fb, const int* frames_b,
                                                                             const double* e_band, const double* g_value,
                                                                             float* g_b, int K, int tmax_a, int tmax_b,
                                                                             int w, int S) {
  __shared__ double s_part[kSdtwGbWaves][kSdtwKc / 2][64];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, b = blockIdx.x;
  const int j = blockIdx.y * 64 + lane;
  const bool live = j < tmax_b;                    // a column of the buffer
  const int Ta = sdtw_frames(frames_a, b, tmax_a), Tb = sdtw_frames(frames_b, b, tmax_b);
  float* out = g_b + (size_t)b * K * tmax_b + j;
  if (Ta == 0 || Tb == 0 || (int)blockIdx.y * 64 >= Tb) {                      // the whole block leaves: no barrier follows
    if (live)
      for (int k = wave; k < K; k += kSdtwGbWaves) out[(size_t)k * tmax_b] = 0.0f;
    return;
  }
  const SdtwBand g = sdtw_band(Ta, Tb, w);
  const bool inside = j < Tb;
  const int jc = inside ? j : 0;                   // a lane behind Tb works on column 0 and writes zeros
  const float* A = fa + (size_t)b * K * tmax_a;
  const float* Bm = fb + (size_t)b * K * tmax_b + jc;
  const double* E = e_band + (size_t)b * (size_t)(tmax_a + tmax_b - 1) * S;
  const double gv = g_value[b];
  int ilo = 0, ihi = g.n;                                                      // the rows of column jc inside the band
  if (g.m > 0) ilo = sdtw_max(0, sdtw_ceildiv(jc * g.n - g.W, g.m)), ihi = sdtw_min(g.n, sdtw_floordiv(jc * g.n + g.W, g.m));
  const int i0 = ilo > wave ? wave + ((ilo - wave + kSdtwGbWaves - 1) / kSdtwGbWaves * kSdtwGbWaves) : wave;
  for (int kc = 0; kc < K; kc += kSdtwKc) {
    double acc[kSdtwKc];
#pragma unroll
    for (int c = 0; c < kSdtwKc; ++c) acc[c] = 0.0;
    for (int i = i0; i <= ihi; i += kSdtwGbWaves) {
      double s = 0.0;
      for (int k = 0; k < K; ++k) {
        const double d = (double)A[(size_t)k * tmax_a + i] - (double)Bm[(size_t)k * tmax_b];
        s += d * d;
      }
      const double wt = sdtw_weight<SQ>(E[sdtw_band_at(g, S, i, jc)], s);
#pragma unroll
      for (int c = 0; c < kSdtwKc; ++c)
        if (kc + c < K)
          acc[c] = fma(wt, (double)Bm[(size_t)(kc + c) * tmax_b] - (double)A[(size_t)(kc + c) * tmax_a + i], acc[c]);
    }
#pragma unroll
    for (int half = 0; half < 2; ++half) {         // eight accumulators at a time: wave w joins accumulator w
#pragma unroll
      for (int c = 0; c < kSdtwKc / 2; ++c) s_part[wave][c][lane] = acc[half * (kSdtwKc / 2) + c];
      __syncthreads();
      const double v = ((s_part[0][wave][lane] + s_part[1][wave][lane]) + (s_part[2][wave][lane] + s_part[3][wave][lane])) +
                       ((s_part[4][wave][lane] + s_part[5][wave][lane]) + (s_part[6][wave][lane] + s_part[7][wave][lane]));
      const int k = kc + half * (kSdtwKc / 2) + wave;
      if (live && k < K) out[(size_t)k * tmax_b] = inside ? (float)(gv * v) : 0.0f;
      __syncthreads();
    }
  }
}

namespace {
inline int sdtw_band_threads(int band) {           // the smallest power of two >= 2 band + 2, at least a wave
  int p = 64;
  while (p < 2 * band + 2) p *= 2;
  return p;
}
}  // namespace

hipError_t launch_sdtw_band_forward(const float* fa, const int* frames_a, const float* fb, const int* frames_b,
                                    double gamma, int cost, double* value, double* r, int B, int K, int tmax_a, int tmax_b,
                                    int band, hipStream_t s) {
  const int threads = sdtw_band_threads(band), S = sdtw_band_rows(tmax_a, band);
  const double inv_gamma = 1.0 / gamma;
  if (cost == kSdtwCostSq)
    hipLaunchKernelGGL(sdtw_band_forward_kernel<true>, dim3(B), dim3(threads), 0, s, fa, frames_a, fb, frames_b, gamma,
                       inv_gamma, value, r, K, tmax_a, tmax_b, band, S);
  else
    hipLaunchKernelGGL(sdtw_band_forward_kernel<false>, dim3(B), dim3(threads), 0, s, fa, frames_a, fb, frames_b, gamma,
                       inv_gamma, value, r, K, tmax_a, tmax_b, band, S);
  return hipGetLastError();
}

hipError_t launch_sdtw_band_backward(const float* fa, const int* frames_a, const float* fb, const int* frames_b,
                                     double gamma, int cost, const double* r, double* e_band, double* e, int B, int K,
                                     int tmax_a, int tmax_b, int band, hipStream_t s) {
  const int threads = sdtw_band_threads(band), S = sdtw_band_rows(tmax_a, band);
  const double inv_gamma = 1.0 / gamma;
  if (e) {
    const hipError_t err = hipMemsetAsync(e, 0, (size_t)B * tmax_a * tmax_b * sizeof(double), s);
    if (err != hipSuccess) return err;
  }
  if (cost == kSdtwCostSq)
    hipLaunchKernelGGL(sdtw_band_backward_kernel<true>, dim3(B), dim3(threads), 0, s, fa, frames_a, fb, frames_b, inv_gamma,
                       r, e_band, e, K, tmax_a, tmax_b, band, S);
  else
    hipLaunchKernelGGL(sdtw_band_backward_kernel<false>, dim3(B), dim3(threads), 0, s, fa, frames_a, fb, frames_b,
                       inv_gamma, r, e_band, e, K, tmax_a, tmax_b, band, S);
  return hipGetLastError();
}

hipError_t launch_sdtw_band_grads(const float* fa, const int* frames_a, const float* fb, const int* frames_b, int cost,
                                  const double* e_band, const double* g_value, float* g_a, float* g_b, int B, int K,
                                  int tmax_a, int tmax_b, int band, hipStream_t s) {
  const bool sq = cost == kSdtwCostSq;
  const int S = sdtw_band_rows(tmax_a, band);
  if (g_a) {
    const dim3 grid(B, (tmax_a + 3) / 4);
    if (sq)
      hipLaunchKernelGGL(sdtw_band_grad_a_kernel<true>, grid, dim3(256), 0, s, fa, frames_a, fb, frames_b, e_band, g_value,
                         g_a, K, tmax_a, tmax_b, band, S);
    else
      hipLaunchKernelGGL(sdtw_band_grad_a_kernel<false>, grid, dim3(256), 0, s, fa, frames_a, fb, frames_b, e_band, g_value,
                         g_a, K, tmax_a, tmax_b, band, S);
    const hipError_t err = hipGetLastError();
    if (err != hipSuccess) return err;
  }
  if (g_b) {
    const dim3 grid(B, (tmax_b + 63) / 64);
    if (sq)
      hipLaunchKernelGGL(sdtw_band_grad_b_kernel<true>, grid, dim3(64 * kSdtwGbWaves), 0, s, fa, frames_a, fb, frames_b,
                         e_band, g_value, g_b, K, tmax_a, tmax_b, band, S);
    else
      hipLaunchKernelGGL(sdtw_band_grad_b_kernel<false>, grid, dim3(64 * kSdtwGbWaves), 0, s, fa, frames_a, fb, frames_b,
                         e_band, g_value, g_b, K, tmax_a, tmax_b, band, S);
  }
  return hipGetLastError();
}

}  // namespace wg
