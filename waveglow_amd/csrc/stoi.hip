// Short-time objective intelligibility of audio pairs on the device (include/waveglow_amd.h: wg_stoi): STOI (Taal,
// Hendriks, Heusdens and Jensen, "An algorithm for intelligibility prediction of time-frequency weighted noisy speech", IEEE
// TASL 19(7), 2011) and ESTOI (Jensen and Taal, "An algorithm for predicting the intelligibility of speech masked by
// modulated noise maskers", IEEE/ACM TASLP 24(11), 2016) of 10 kHz fp32 audio.  The reference has no counterpart; the
// definition is stated in the header and DESIGN.md section 7.  Everything is fp64 arithmetic on the fp32 samples, every sum
// runs in one fixed order that depends on the utterance alone and no kernel uses atomics, so a call gives the same bits
// every time and an utterance the same bits in any batch and on any row pitch.  Products may be contracted into the sums
// they go into (fused multiply-add): parity with a host restatement is to a tolerance.  No kernel calls a device cos or
// sin; the twiddles come from the caller's 512-entry table.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "wg_stoi.h"

namespace wg {

namespace {

constexpr double kStoiEps = 2.220446049250313e-16;        // 2^-52
constexpr double kStoiRange = 40.0;                       // dB below the loudest frame
constexpr double kStoiClip = 6.623413251903491;           // 1 + 10^(15 / 20)

// Sample count of row b: a length outside [0, pitch] counts as 0, so nothing is read past a row.
__device__ __forceinline__ int stoi_len(const int* lens, int b, int pitch) {
  const int n = lens[b];
  return (n < 0 || n > pitch) ? 0 : n;
}

__device__ __forceinline__ int stoi_common_len(const int* len_x, const int* len_y, int b, int pitch) {
  const int nx = stoi_len(len_x, b, pitch), ny = stoi_len(len_y, b, pitch);
  return nx < ny ? nx : ny;
}

}  // namespace

// ------------------------------------------------------------------------------------------------- (a) frame energies
// grid (ceil(F0max / 4), B), 256 threads: one wave per frame of the clean signal.  Lane l squares the windowed samples
// l, l + 64, l + 128, l + 192 ascending, the 64 partial sums are joined by a butterfly; e = 20 log10(sqrt(sum) + EPS).
__global__ void __launch_bounds__(256) stoi_energy_kernel(const float* x, const int* len_x, const int* len_y,
                                                          const double* window, double* energy, int pitch, int F0max) {
  const int lane = threadIdx.x & 63, b = blockIdx.y;
  const int t = blockIdx.x * 4 + (threadIdx.x >> 6);
  const int F0 = stoi_frames(stoi_common_len(len_x, len_y, b, pitch));
  if (t >= F0) return;                                                        // per wave; no barrier in this kernel
  const float* src = x + (size_t)b * pitch + (size_t)t * kStoiH;             // t * H + W < n <= pitch
  double acc = 0.0;
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int j = lane + 64 * i;
    const double v = window[j] * (double)src[j];
    acc += v * v;
  }
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) acc += __shfl_xor(acc, o);
  if (lane == 0) energy[(size_t)b * F0max + t] = 20.0 * log10(sqrt(acc) + kStoiEps);
}

// --------------------------------------------------------------------------------------------- (b) kept-frame list
// grid B, 256 threads.  The maximum of the energies, then frame t is kept where max - 40 - e[t] < 0; the kept indices are
// written ascending by a ballot scan over passes of 256 frames.  counts[b] = {n, F0, K, J}.
__global__ void __launch_bounds__(256) stoi_compact_kernel(const double* energy, const int* len_x, const int* len_y,
                                                           int* kept, int* counts, int pitch, int F0max) {
  __shared__ double s_max[256];
  __shared__ int s_wave[4];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, b = blockIdx.x;
  const int n = stoi_common_len(len_x, len_y, b, pitch);
  const int F0 = stoi_frames(n);
  const double* e = energy + (size_t)b * F0max;
  int* out = kept + (size_t)b * F0max;
  double m = -INFINITY;
  for (int t = tid; t < F0; t += 256) m = e[t] > m ? e[t] : m;
  s_max[tid] = m;
  __syncthreads();
  for (int w = 128; w >= 1; w >>= 1) {
    if (tid < w) s_max[tid] = s_max[tid + w] > s_max[tid] ? s_max[tid + w] : s_max[tid];
    __syncthreads();
  }
  const double floor_db = s_max[0] - kStoiRange;
  int base = 0;
  for (int c = 0; c < F0; c += 256) {
    const int t = c + tid;
    const bool keep = t < F0 && floor_db - e[t] < 0.0;
    const unsigned long long votes = __ballot(keep);
    if (lane == 0) s_wave[wave] = __popcll(votes);
    __syncthreads();
    int before = base + __popcll(votes & ((1ull << lane) - 1ull));
    for (int w = 0; w < wave; ++w) before += s_wave[w];
    if (keep) out[before] = t;
    base += s_wave[0] + s_wave[1] + s_wave[2] + s_wave[3];
    __syncthreads();
  }
  if (tid == 0) {
    const int J = base - 1 - (kStoiSeg - 1);
    counts[b * 4 + 0] = n, counts[b * 4 + 1] = F0, counts[b * 4 + 2] = base, counts[b * 4 + 3] = J > 0 ? J : 0;
  }
}

// -------------------------------------------------------------------------------------------------- (c) band spectra
// grid (ceil(Fmax / 8), 2, B), 256 threads: one workgroup transforms kStoiFrameTile = 8 consecutive frames of the
// silence-free signal of x (blockIdx.y = 0) or y (1).  With k[i] the i-th kept frame, the silence-free signal is the
// overlap-add of the windowed kept frames at hop 128, so its frame t is, sample by sample,
//   j < 128:  w[j] x[128 k[t] + j] + w[j + 128] x[128 k[t-1] + j + 128]      (t = 0: the first term alone)
//   j >= 128: w[j] x[128 k[t] + j] + w[j - 128] x[128 k[t+1] + j - 128]
// gathered straight from the input and windowed again.  The largest index read is 128 k[K-1] + 255 < n.
// Thread tid < 212 owns bin 7 + tid and runs the 256 samples ascending for the 8 frames at once: the twiddle of sample j is
// entry (bin * j) mod 512 of the table, one LDS read shared by the 8 frames, and the 8 samples are one address for the
// whole wave (a broadcast).  A (frame, bin) sum is one serial chain, whatever slot of whatever tile the frame is in.
// The powers then go through LDS to 15 x 8 threads, each summing its band's bins ascending.
__global__ void __launch_bounds__(256) stoi_bands_kernel(const float* x, const float* y, const int* counts, const int* kept,
                                                         const double* window, const int* bands, const double* cossin,
                                                         double* out, int pitch, int F0max, int Fmax) {
  constexpr int T = kStoiFrameTile;
  __shared__ double s_f[kStoiW * T];                     // [sample][frame]; afterwards the powers [frame][bin]
  __shared__ double2 s_cs[kStoiNfft];
  const int tid = threadIdx.x, t0 = blockIdx.x * T, b = blockIdx.z;
  const int F = counts[b * 4 + 2] - 1;                                        // K - 1 frames; K = 0 gives -1
  if (t0 >= F) return;                                                        // the whole block leaves: no barrier follows
  const float* src = (blockIdx.y ? y : x) + (size_t)b * pitch;
  const int* kp = kept + (size_t)b * F0max;
  s_cs[tid] = ((const double2*)cossin)[tid];
  s_cs[tid + 256] = ((const double2*)cossin)[tid + 256];
  const int jo = tid ^ 128;                                                   // the same sample in the neighbouring frame
  const double wj = window[tid], wo = window[jo];
#pragma unroll
  for (int r = 0; r < T; ++r) {
    const int t = t0 + r;
    double v = 0.0;
    if (t < F) {
      double a = wj * (double)src[(size_t)kp[t] * kStoiH + tid];
      const int other = tid < 128 ? t - 1 : t + 1;                            // t + 1 <= F = K - 1
      if (other >= 0) a += wo * (double)src[(size_t)kp[other] * kStoiH + jo];
      v = wj * a;
    }
    s_f[tid * T + r] = v;
  }
  __syncthreads();
  double re[T], im[T];
#pragma unroll
  for (int r = 0; r < T; ++r) re[r] = 0.0, im[r] = 0.0;
  if (tid < kStoiBins) {
    const int bin = kStoiBinLo + tid;
    int idx = 0;
#pragma unroll 2
    for (int j = 0; j < kStoiW; ++j) {
      const double2 cs = s_cs[idx];
      idx = (idx + bin) & (kStoiNfft - 1);
      const double2* f = (const double2*)(s_f + j * T);
#pragma unroll
      for (int r = 0; r < T; r += 2) {
        const double2 v = f[r >> 1];
        re[r] = fma(cs.x, v.x, re[r]), im[r] = fma(cs.y, v.x, im[r]);
        re[r + 1] = fma(cs.x, v.y, re[r + 1]), im[r + 1] = fma(cs.y, v.y, im[r + 1]);
      }
    }
  }
  __syncthreads();                                                            // every frame sample has been read
  if (tid < kStoiBins) {
#pragma unroll
    for (int r = 0; r < T; ++r) s_f[r * kStoiBins + tid] = re[r] * re[r] + im[r] * im[r];
  }
  __syncthreads();
  if (tid < kStoiBands * T) {
    const int r = tid / kStoiBands, band = tid - r * kStoiBands, t = t0 + r;
    if (t < F) {
      // the table is the caller's: whatever it holds, only bins 7 .. 218 exist here
      int lo = bands[2 * band], hi = bands[2 * band + 1];
      lo = lo < kStoiBinLo ? kStoiBinLo : lo;
      hi = hi > kStoiBinLo + kStoiBins ? kStoiBinLo + kStoiBins : hi;
      double sum = 0.0;
      for (int k = lo; k < hi; ++k) sum += s_f[r * kStoiBins + k - kStoiBinLo];
      out[(((size_t)b * 2 + blockIdx.y) * kStoiBands + band) * Fmax + t] = sqrt(sum);
    }
  }
}

// ------------------------------------------------------------------------------------------------------ (d) segments
// grid (ceil(Jmax / 4), B), 256 threads: one wave per segment m, the 15 x 30 blocks X[:, m .. m+29] and Y[:, m .. m+29]
// staged in LDS.  Lane `band` < 15 runs its row serially (the STOI term of the row, then the mean-removed, normalised rows
// in place); lane `i` < 30 then runs column i of the normalised rows over the 15 bands (ESTOI); lane 0 adds the 15 row
// terms and the 30 column terms ascending.  seg[b][m] = {sum over the bands of x . y', sum over the columns of x . y / 30}.
__global__ void __launch_bounds__(256) stoi_segment_kernel(const double* bands, const int* counts, double* seg, int Fmax,
                                                           int Jmax) {
  constexpr int N = kStoiSeg, NB = kStoiBands;
  __shared__ double s_x[kStoiSegTile][NB * N];
  __shared__ double s_y[kStoiSegTile][NB * N];
  __shared__ double s_row[kStoiSegTile][16];
  __shared__ double s_col[kStoiSegTile][32];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, b = blockIdx.y;
  const int J = counts[b * 4 + 3];
  if ((int)blockIdx.x * kStoiSegTile >= J) return;                            // the whole block leaves
  const int m = blockIdx.x * kStoiSegTile + wave;
  const bool on = m < J;                                                      // m + 29 <= J + 28 = F - 1
  const double* X = bands + (size_t)b * 2 * NB * Fmax;
  const double* Y = X + (size_t)NB * Fmax;
  double *sx = s_x[wave], *sy = s_y[wave];
  if (on) {
    for (int i = lane; i < NB * N; i += 64) {
      const int band = i / N, f = i - band * N;
      sx[i] = X[(size_t)band * Fmax + m + f];
      sy[i] = Y[(size_t)band * Fmax + m + f];
    }
  }
  __syncthreads();
  if (on && lane < NB) {
    double* xr = sx + lane * N;
    double* yr = sy + lane * N;
    double sxx = 0.0, syy = 0.0, sumx = 0.0, sumy = 0.0;
    for (int i = 0; i < N; ++i) {
      const double xv = xr[i], yv = yr[i];
      sxx += xv * xv, syy += yv * yv, sumx += xv, sumy += yv;
    }
    const double alpha = sqrt(sxx) / (sqrt(syy) + kStoiEps);
    double sump = 0.0;
    for (int i = 0; i < N; ++i) sump += fmin(alpha * yr[i], xr[i] * kStoiClip);
    const double mx = sumx / N, my = sumy / N, mp = sump / N;
    double nx = 0.0, ny = 0.0, np = 0.0;
    for (int i = 0; i < N; ++i) {
      const double dx = xr[i] - mx, dy = yr[i] - my, dp = fmin(alpha * yr[i], xr[i] * kStoiClip) - mp;
      nx += dx * dx, ny += dy * dy, np += dp * dp;
    }
    const double ix = sqrt(nx) + kStoiEps, iy = sqrt(ny) + kStoiEps, ip = sqrt(np) + kStoiEps;
    double corr = 0.0;
    for (int i = 0; i < N; ++i) {
      const double xv = xr[i], yv = yr[i];
      const double xn = (xv - mx) / ix;
      corr += xn * ((fmin(alpha * yv, xv * kStoiClip) - mp) / ip);
      xr[i] = xn;
      yr[i] = (yv - my) / iy;
    }
    s_row[wave][lane] = corr;
  }
  __syncthreads();
  if (on && lane < N) {
    double sumx = 0.0, sumy = 0.0;
    for (int k = 0; k < NB; ++k) sumx += sx[k * N + lane], sumy += sy[k * N + lane];
    const double mx = sumx / NB, my = sumy / NB;
    double nx = 0.0, ny = 0.0;
    for (int k = 0; k < NB; ++k) {
      const double dx = sx[k * N + lane] - mx, dy = sy[k * N + lane] - my;
      nx += dx * dx, ny += dy * dy;
    }
    const double ix = sqrt(nx) + kStoiEps, iy = sqrt(ny) + kStoiEps;
    double corr = 0.0;
    for (int k = 0; k < NB; ++k) corr += ((sx[k * N + lane] - mx) / ix) * ((sy[k * N + lane] - my) / iy);
    s_col[wave][lane] = corr;
  }
  __syncthreads();
  if (on && lane == 0) {
    double st = 0.0, es = 0.0;
    for (int k = 0; k < NB; ++k) st += s_row[wave][k];
    for (int i = 0; i < N; ++i) es += s_col[wave][i];
    seg[((size_t)b * Jmax + m) * 2] = st;
    seg[((size_t)b * Jmax + m) * 2 + 1] = es / N;
  }
}

// ------------------------------------------------------------------------------------------------------- (e) the row
// grid B, 256 threads.  Thread tid adds the segments tid, tid + 256, ... ascending, the 256 partial sums are joined by a
// tree in LDS: the shape depends on J alone.  rows[b] = {STOI, ESTOI, F0, K, J, 0, 0, 0}; no segment gives NaN twice.
__global__ void __launch_bounds__(256) stoi_final_kernel(const double* seg, const int* counts, double* rows, int Jmax) {
  __shared__ double s_sum[2][256];
  const int tid = threadIdx.x, b = blockIdx.x;
  const int J = counts[b * 4 + 3];
  const double* p = seg + (size_t)b * Jmax * 2;
  double st = 0.0, es = 0.0;
  for (int m = tid; m < J; m += 256) st += p[2 * m], es += p[2 * m + 1];
  s_sum[0][tid] = st, s_sum[1][tid] = es;
  __syncthreads();
  for (int w = 128; w >= 1; w >>= 1) {
    if (tid < w) s_sum[0][tid] += s_sum[0][tid + w], s_sum[1][tid] += s_sum[1][tid + w];
    __syncthreads();
  }
  if (tid == 0) {
    double* o = rows + (size_t)b * kStoiRow;
    o[0] = J > 0 ? s_sum[0][0] / ((double)kStoiBands * (double)J) : NAN;
    o[1] = J > 0 ? s_sum[1][0] / (double)J : NAN;
    o[2] = (double)counts[b * 4 + 1];
    o[3] = (double)counts[b * 4 + 2];
    o[4] = (double)J;
    o[5] = 0.0, o[6] = 0.0, o[7] = 0.0;
  }
}

// --------------------------------------------------------------------------------------------------------------- launch
hipError_t launch_stoi(const float* x, const int* len_x, const float* y, const int* len_y, const double* window,
                       const int* bands, const double* cossin, double* rows, const StoiGeom& g, const StoiBuffers& w,
                       hipStream_t s) {
  hipLaunchKernelGGL(stoi_energy_kernel, dim3((g.F0max + 3) / 4, g.B), dim3(256), 0, s, x, len_x, len_y, window, w.energy,
                     g.pitch, g.F0max);
  hipLaunchKernelGGL(stoi_compact_kernel, dim3(g.B), dim3(256), 0, s, w.energy, len_x, len_y, w.kept, w.counts, g.pitch,
                     g.F0max);
  hipLaunchKernelGGL(stoi_bands_kernel, dim3((g.Fmax + kStoiFrameTile - 1) / kStoiFrameTile, 2, g.B), dim3(256), 0, s, x, y,
                     w.counts, w.kept, window, bands, cossin, w.bands, g.pitch, g.F0max, g.Fmax);
  hipLaunchKernelGGL(stoi_segment_kernel, dim3((g.Jmax + kStoiSegTile - 1) / kStoiSegTile, g.B), dim3(256), 0, s, w.bands,
                     w.counts, w.seg, g.Fmax, g.Jmax);
  hipLaunchKernelGGL(stoi_final_kernel, dim3(g.B), dim3(256), 0, s, w.seg, w.counts, rows, g.Jmax);
  return hipGetLastError();
}

}  // namespace wg
