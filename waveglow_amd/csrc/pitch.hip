// Pitch metrics of audio pairs on the device (include/waveglow_amd.h: wg_pitch_*): a YIN fundamental-frequency tracker,
// steps 1-5 of de Cheveigne & Kawahara, "YIN, a fundamental frequency estimator for speech and music", JASA 111(4), 2002
// (difference function, cumulative mean normalised difference, absolute threshold, parabolic interpolation), and the F0 /
// voicing errors of two tracks.  The reference has no counterpart; the definition is stated in the header and DESIGN.md
// section 7.  Everything is fp64 arithmetic on the fp32 samples, every sum runs in one fixed order and no kernel uses
// atomics, so a call gives the same bits every time and an utterance the same bits in any batch.
// No contraction anywhere in this file: a product and the sum it goes into are rounded separately, as a host restatement
// in numpy rounds them.  This file must not be built with a fast-math flag.
#include <hip/hip_runtime.h>
#include <limits.h>
#include <math.h>
#include <stdint.h>

#include "wg_pitch.h"

#pragma clang fp contract(off)

namespace wg {

// Sample count of utterance b: a length outside [0, N] counts as 0, so nothing is read past a row.
__device__ __forceinline__ int pitch_len(const int* lens, int b, int N) {
  const int n = lens[b];
  return (n < 0 || n > N) ? 0 : n;
}

// ----------------------------------------------------------------------------------------------------------------- YIN
// grid (fmax, B), 256 threads: one workgroup per (frame, utterance).  The frame's W + tau_max samples are staged once in
// LDS as fp32.  Thread `tid` owns the R consecutive lags tid * R + 1 .. tid * R + R (lag 0 has d = 0 and d' = 1 by
// definition) and runs j ascending: x[j] is one address for the whole wave (a broadcast), the R samples x[j + tau] are a
// window in registers that takes one new LDS read per j, R * tid + const apart between lanes.  d(tau) is therefore the
// plain ascending fp64 sum of the definition whatever R is; R only follows from tau_max (1, 2 or 4).
// The running sum of d is a scan in a fixed shape: ascending inside a thread, a Hillis-Steele scan over the 64 lanes of a
// wave, the wave totals added ascending.  The shape depends on tau_max alone, never on B, fmax or the grid.
// The index of every LDS read is clamped to the last staged sample, and staging reads W + tau_max samples from s on:
// nothing behind s + W + tau_max - 1 is read.
template <int R>
__global__ void __launch_bounds__(256) yin_kernel(const float* audio, const int* lens, double* f0, double* ap,
                                                  int* frames_out, PitchGeom g, int N, int fmax) {
  __shared__ float s_x[kPitchMaxFrame + kPitchMaxTau];
  __shared__ double s_dp[kPitchMaxTau + 1];
  __shared__ double s_wave[4];
  __shared__ double s_min[4];
  __shared__ int s_cand[4];
  const int tid = threadIdx.x, t = blockIdx.x, b = blockIdx.y;
  const int lane = tid & 63, wave = tid >> 6;
  const int W = g.W, tau_max = g.tau_max;
  int F = pitch_frames(pitch_len(lens, b, N), W, g.H, tau_max);
  if (F > fmax) F = fmax;
  if (t >= F) {                                                                // the whole block leaves: no barrier follows
    if (tid == 0) {
      f0[(size_t)b * fmax + t] = 0.0;
      ap[(size_t)b * fmax + t] = 0.0;
      if (t == 0) frames_out[b] = 0;
    }
    return;
  }
  if (t == 0 && tid == 0) frames_out[b] = F;
  const int n = W + tau_max;
  const float* x = audio + (size_t)b * N + (size_t)t * g.H;                  // t * H + n <= len <= N
  for (int i = tid; i < n; i += 256) s_x[i] = x[i];
  __syncthreads();

  const int tau0 = tid * R + 1;
  double acc[R], win[R];
#pragma unroll
  for (int r = 0; r < R; ++r) acc[r] = 0.0;
  if (tau0 <= tau_max) {
#pragma unroll
    for (int r = 0; r + 1 < R; ++r) {
      const int i = tau0 + r;
      win[r] = (double)s_x[i < n ? i : n - 1];
    }
#pragma unroll 4
    for (int j = 0; j < W; ++j) {
      const int i = j + tau0 + R - 1;
      win[R - 1] = (double)s_x[i < n ? i : n - 1];
      const double xj = (double)s_x[j];
#pragma unroll
      for (int r = 0; r < R; ++r) {
        const double d = xj - win[r];
        acc[r] += d * d;
      }
#pragma unroll
      for (int r = 0; r + 1 < R; ++r) win[r] = win[r + 1];
    }
  }
  // running sum of d(1 .. tau): inside the thread, across the wave, across the waves
  double run[R];
#pragma unroll
  for (int r = 0; r < R; ++r) {
    if (tau0 + r > tau_max) acc[r] = 0.0;                                      // a lag behind tau_max read clamped samples
    run[r] = r == 0 ? acc[0] : run[r > 0 ? r - 1 : 0] + acc[r];
  }
  double v = run[R - 1];
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const double u = __shfl_up(v, o);
    if (lane >= o) v += u;
  }
  if (lane == 63) s_wave[wave] = v;
  double before = __shfl_up(v, 1);                                             // the lanes below this one
  if (lane == 0) before = 0.0;
  __syncthreads();
  double base = 0.0;
  for (int w = 0; w < wave; ++w) base += s_wave[w];
  before = base + before;
  // d'(tau), this thread's first lag under the threshold and its smallest d' inside [tau_min, tau_max]
  int cand = INT_MAX;
  double lowest = INFINITY;
#pragma unroll
  for (int r = R - 1; r >= 0; --r) {
    const int tau = tau0 + r;
    if (tau <= tau_max) {
      const double cum = before + run[r];
      const double dp = cum == 0.0 ? 1.0 : acc[r] * (double)tau / cum;
      s_dp[tau] = dp;
      if (tau >= g.tau_min) {
        if (dp < g.threshold) cand = tau;
        if (dp < lowest) lowest = dp;
      }
    }
  }
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) {
    const int c = __shfl_xor(cand, o);
    const double l = __shfl_xor(lowest, o);
    cand = c < cand ? c : cand;
    lowest = l < lowest ? l : lowest;
  }
  if (lane == 0) s_cand[wave] = cand, s_min[wave] = lowest;
  __syncthreads();
  if (tid != 0) return;
  for (int w = 1; w < 4; ++w) {
    cand = s_cand[w] < cand ? s_cand[w] : cand;
    lowest = s_min[w] < lowest ? s_min[w] : lowest;
  }
  double f = 0.0, a = lowest;
  if (cand != INT_MAX) {
    int tau = cand;
    while (tau + 1 <= tau_max && s_dp[tau + 1] < s_dp[tau]) ++tau;
    a = s_dp[tau];
    double shift = 0.0;
    if (tau - 1 >= 1 && tau + 1 <= tau_max) {
      const double pa = s_dp[tau - 1], pb = s_dp[tau], pc = s_dp[tau + 1];
      const double den = pa - 2.0 * pb + pc;
      if (den > 0.0) {
        const double sh = (pa - pc) / (2.0 * den);
        if (fabs(sh) <= 1.0) shift = sh;
      }
    }
    f = g.sr / ((double)tau + shift);
  }
  f0[(size_t)b * fmax + t] = f;
  ap[(size_t)b * fmax + t] = a;
}

// ------------------------------------------------------------------------------------------------------- pair metrics
// grid B, 256 threads.  Thread tid takes the frames tid, tid + 256, ... ascending; the 256 partial sums and counts are
// joined by a tree in LDS, like padded_kernel of metrics.hip.  A frame is voiced where its f0 > 0.
__global__ void __launch_bounds__(256) pitch_compare_kernel(const double* f0_a, const int* frames_a, const double* f0_b,
                                                            const int* frames_b, double* rows, int fmax_a, int fmax_b) {
  __shared__ double s_sum[2][256];
  __shared__ int s_cnt[5][256];
  const int tid = threadIdx.x, b = blockIdx.x;
  int Fa = frames_a[b], Fb = frames_b[b];
  if (Fa < 0 || Fa > fmax_a) Fa = 0;
  if (Fb < 0 || Fb > fmax_b) Fb = 0;
  const int F = Fa < Fb ? Fa : Fb;
  const double* A = f0_a + (size_t)b * fmax_a;
  const double* Bm = f0_b + (size_t)b * fmax_b;
  double cents2 = 0.0, hz2 = 0.0;
  int gross = 0, vuv = 0, va = 0, vb = 0, both = 0;
  for (int t = tid; t < F; t += 256) {
    const double fa = A[t], fb = Bm[t];
    const bool a_on = fa > 0.0, b_on = fb > 0.0;
    va += a_on, vb += b_on, vuv += a_on != b_on;
    if (a_on && b_on) {
      ++both;
      const double ratio = fb / fa;
      const double c = 1200.0 * log2(ratio), h = fb - fa;
      cents2 += c * c;
      hz2 += h * h;
      gross += fabs(ratio - 1.0) > 0.2;
    }
  }
  s_sum[0][tid] = cents2, s_sum[1][tid] = hz2;
  s_cnt[0][tid] = gross, s_cnt[1][tid] = vuv, s_cnt[2][tid] = va, s_cnt[3][tid] = vb, s_cnt[4][tid] = both;
  __syncthreads();
  for (int w = 128; w >= 1; w >>= 1) {
    if (tid < w) {
      s_sum[0][tid] += s_sum[0][tid + w], s_sum[1][tid] += s_sum[1][tid + w];
#pragma unroll
      for (int k = 0; k < 5; ++k) s_cnt[k][tid] += s_cnt[k][tid + w];
    }
    __syncthreads();
  }
  if (tid == 0) {
    double* o = rows + (size_t)b * kPitchRow;
    const int n = s_cnt[4][0];
    o[0] = n > 0 ? sqrt(s_sum[0][0] / (double)n) : NAN;
    o[1] = n > 0 ? sqrt(s_sum[1][0] / (double)n) : NAN;
    o[2] = n > 0 ? (double)s_cnt[0][0] / (double)n : NAN;
    o[3] = F > 0 ? (double)s_cnt[1][0] / (double)F : NAN;
    o[4] = (double)F;
    o[5] = (double)s_cnt[2][0];
    o[6] = (double)s_cnt[3][0];
    o[7] = (double)n;
  }
}

// --------------------------------------------------------------------------------------------------------------- launch
hipError_t launch_yin(const float* audio, const int* lens, double* f0, double* ap, int* frames_out, const PitchGeom& g,
                      int B, int N, int fmax, hipStream_t s) {
  const int R = (g.tau_max + 255) / 256;                             // lags per thread: 1, 2 or 4
#define WG_YIN(RR) \
  hipLaunchKernelGGL(yin_kernel<RR>, dim3(fmax, B), dim3(256), 0, s, audio, lens, f0, ap, frames_out, g, N, fmax)
  switch (R) {
    case 1: WG_YIN(1); break;
    case 2: WG_YIN(2); break;
    case 3:
    case 4: WG_YIN(4); break;
    default: return hipErrorInvalidValue;
  }
#undef WG_YIN
  return hipGetLastError();
}

hipError_t launch_pitch_compare(const double* f0_a, const int* frames_a, const double* f0_b, const int* frames_b,
                                double* rows, int B, int fmax_a, int fmax_b, hipStream_t s) {
  hipLaunchKernelGGL(pitch_compare_kernel, dim3(B), dim3(256), 0, s, f0_a, frames_a, f0_b, frames_b, rows, fmax_a, fmax_b);
  return hipGetLastError();
}

}  // namespace wg
