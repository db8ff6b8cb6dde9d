// Gradient of STOI and ESTOI with respect to the processed signal (include/waveglow_amd.h: wg_stoi_backward): the reverses of
// stages (e) .. (c) of stoi.hip and of the overlap-add in front of them.  The energy gate depends on the clean signal alone,
// so the kept-frame list, the clean band spectra and the counts are constants here; they and the processed band spectra
// come from the buffer wg_stoi_forward saved.  Everything is fp64, every sum runs in one fixed order that depends on the
// utterance alone and no kernel uses atomics: a call gives the same bits every time and an utterance the same bits in any
// batch and on any row pitch.  Products may be contracted into the sums they go into.  No kernel calls a device cos or sin.
// Conventions at the points where the definition is not smooth (header): the gradient through a square
// root of exactly 0 is 0; at a tie of min(alpha y, clip x) the gradient goes to the alpha y branch; alpha is differentiated.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "wg_stoi.h"

namespace wg {

namespace {

constexpr double kStoiEps = 2.220446049250313e-16;        // 2^-52
constexpr double kStoiClip = 6.623413251903491;           // 1 + 10^(15 / 20)

// d sqrt(v) / dv times `num` with the convention above: num / root where root = sqrt(v) > 0, else 0
__device__ __forceinline__ double over_root(double num, double root) { return root > 0.0 ? num / root : 0.0; }

}  // namespace

// ------------------------------------------------------------------------------------- inverse of the kept-frame list
// grid B, 256 threads: inv[b][f] = i where original frame f is silence-free frame i (kept[b][i] = f), -1 where it was gated.
__global__ void __launch_bounds__(256) stoi_inverse_kernel(const int* counts, const int* kept, int* inv, int F0max) {
  const int b = blockIdx.x;
  int F0 = counts[b * 4 + 1], K = counts[b * 4 + 2];
  F0 = F0 > F0max ? F0max : F0, K = K > F0 ? F0 : K;
  const int* kp = kept + (size_t)b * F0max;
  int* out = inv + (size_t)b * F0max;
  for (int t = threadIdx.x; t < F0; t += 256) out[t] = -1;
  __syncthreads();
  for (int i = threadIdx.x; i < K; i += 256) {
    const int f = kp[i];
    if (f >= 0 && f < F0) out[f] = i;                                         // the list is ascending: every f once
  }
}

// --------------------------------------------------------------------------------------- reverse of (e) and (d): segments
// grid (Jmax, B), 64 threads: one wave per segment m recomputes its 15 x 30 block from the saved X, Y and writes
//   blocks[b][m][band][i] = d (g0 STOI + g1 ESTOI) / d Y[band][m + i]   through this segment alone,
// the weights g0 / (15 J) and g1 / (30 J) folded in.  Lane `band` < 15 runs its row serially (the STOI term and its
// gradient, the row normalisation of ESTOI), lane i < 30 column i (the column normalisation, the correlation and their
// reverses), lane `band` again the reverse of the row normalisation.
__global__ void __launch_bounds__(64) stoi_segment_grad_kernel(const double* bands, const int* counts, const double* g_rows,
                                                               double* blocks, int Fmax, int Jmax) {
  constexpr int N = kStoiSeg, NB = kStoiBands;
  __shared__ double s_x[NB * N];       // X block; afterwards its row-normalised form
  __shared__ double s_y[NB * N];       // Y block
  __shared__ double s_u[NB * N];       // row-normalised Y; afterwards the gradient with respect to it
  __shared__ double s_g[NB * N];       // the STOI part of the result
  const int lane = threadIdx.x, m = blockIdx.x, b = blockIdx.y;
  const int J = counts[b * 4 + 3];
  if (m >= J || m >= Jmax) return;                                            // the whole block leaves; m + 29 <= F - 1
  const double* X = bands + (size_t)b * 2 * NB * Fmax;
  const double* Y = X + (size_t)NB * Fmax;
  for (int i = lane; i < NB * N; i += 64) {
    const int band = i / N, f = i - band * N;
    s_x[i] = X[(size_t)band * Fmax + m + f];
    s_y[i] = Y[(size_t)band * Fmax + m + f];
  }
  __syncthreads();
  const double w_stoi = g_rows[b * 2] / ((double)NB * (double)J);
  const double w_estoi = g_rows[b * 2 + 1] / ((double)N * (double)J);
  double my_row = 0.0, iy_row = 1.0, sny_row = 0.0;                            // row statistics of Y, kept for the last phase
  if (lane < NB) {
    double* xr = s_x + lane * N;
    const double* yr = s_y + lane * N;
    double* ur = s_u + lane * N;
    double* gr = s_g + lane * N;
    double sxx = 0.0, syy = 0.0, sumx = 0.0, sumy = 0.0;
    for (int i = 0; i < N; ++i) {
      const double xv = xr[i], yv = yr[i];
      sxx += xv * xv, syy += yv * yv, sumx += xv, sumy += yv;
    }
    const double rx = sqrt(sxx), ry = sqrt(syy), den = ry + kStoiEps;
    const double alpha = rx / den;
    double sump = 0.0;
    for (int i = 0; i < N; ++i) {
      const double a = alpha * yr[i], c = xr[i] * kStoiClip;
      sump += a <= c ? a : c;
    }
    const double mx = sumx / N, my = sumy / N, mp = sump / N;
    double nx = 0.0, ny = 0.0, np = 0.0;
    for (int i = 0; i < N; ++i) {
      const double a = alpha * yr[i], c = xr[i] * kStoiClip;
      const double dx = xr[i] - mx, dy = yr[i] - my, dp = (a <= c ? a : c) - mp;
      nx += dx * dx, ny += dy * dy, np += dp * dp;
    }
    const double snp = sqrt(np), sny = sqrt(ny);
    const double ix = sqrt(nx) + kStoiEps, iy = sny + kStoiEps, ip = snp + kStoiEps;
    double corr = 0.0;
    for (int i = 0; i < N; ++i) {
      const double a = alpha * yr[i], c = xr[i] * kStoiClip;
      corr += ((xr[i] - mx) / ix) * (((a <= c ? a : c) - mp) / ip);
    }
    // corr = sum xn q, q = dp / (sqrt(sum dp^2) + EPS): G = d corr / d dp, then the mean removal
    double sumg = 0.0;
    for (int i = 0; i < N; ++i) {
      const double a = alpha * yr[i], c = xr[i] * kStoiClip;
      const double dp = (a <= c ? a : c) - mp;
      const double G = ((xr[i] - mx) / ix - corr * over_root(dp, snp)) / ip;
      gr[i] = G;
      sumg += G;
    }
    const double mg = sumg / N;
    double dalpha = 0.0;                                                       // d corr / d alpha
    for (int i = 0; i < N; ++i) {
      const double a = alpha * yr[i], c = xr[i] * kStoiClip;
      const double gp = a <= c ? gr[i] - mg : 0.0;                             // the clip branch holds no y
      gr[i] = gp;
      dalpha += yr[i] * gp;
    }
    const double da = -(rx / (den * den)) * dalpha;                            // times d ||y|| / d y[i] = y[i] / ||y||
    for (int i = 0; i < N; ++i) gr[i] = w_stoi * (alpha * gr[i] + da * over_root(yr[i], ry));
    // the row normalisation of ESTOI
    for (int i = 0; i < N; ++i) {
      xr[i] = (xr[i] - mx) / ix;
      ur[i] = (yr[i] - my) / iy;
    }
    my_row = my, iy_row = iy, sny_row = sny;
  }
  __syncthreads();
  if (lane < N) {
    double sumx = 0.0, sumy = 0.0;
    for (int k = 0; k < NB; ++k) sumx += s_x[k * N + lane], sumy += s_u[k * N + lane];
    const double mx = sumx / NB, my = sumy / NB;
    double nx = 0.0, ny = 0.0;
    for (int k = 0; k < NB; ++k) {
      const double dx = s_x[k * N + lane] - mx, dy = s_u[k * N + lane] - my;
      nx += dx * dx, ny += dy * dy;
    }
    const double sny = sqrt(ny);
    const double ix = sqrt(nx) + kStoiEps, iy = sny + kStoiEps;
    // column term = sum_k xz[k] d[k] / iy, d = u - mean: its gradient with respect to d, then the mean removal
    double dot = 0.0;
    for (int k = 0; k < NB; ++k) dot += ((s_x[k * N + lane] - mx) / ix) * (s_u[k * N + lane] - my);
    const double pull = dot / (iy * iy);
    double sumg = 0.0;
    for (int k = 0; k < NB; ++k) sumg += ((s_x[k * N + lane] - mx) / ix) / iy - pull * over_root(s_u[k * N + lane] - my, sny);
    const double mg = sumg / NB;
    for (int k = 0; k < NB; ++k) {
      const double gd = ((s_x[k * N + lane] - mx) / ix) / iy - pull * over_root(s_u[k * N + lane] - my, sny);
      s_u[k * N + lane] = w_estoi * (gd - mg);                                 // column `lane` is this lane's alone
    }
  }
  __syncthreads();
  if (lane < NB) {
    const double* yr = s_y + lane * N;
    const double* gu = s_u + lane * N;
    double dot = 0.0;
    for (int i = 0; i < N; ++i) dot += gu[i] * (yr[i] - my_row);
    const double pull = dot / (iy_row * iy_row);
    double sumg = 0.0;
    for (int i = 0; i < N; ++i) sumg += gu[i] / iy_row - pull * over_root(yr[i] - my_row, sny_row);
    const double mg = sumg / N;
    double* out = blocks + (((size_t)b * Jmax + m) * NB + lane) * N;
    for (int i = 0; i < N; ++i)
      out[i] = s_g[lane * N + i] + ((gu[i] / iy_row - pull * over_root(yr[i] - my_row, sny_row)) - mg);
  }
}

// ------------------------------------------------------------------------ the blocks joined, reverse of the band root
// grid (ceil(Fmax / 256), 15, B), 256 threads: thread t adds the at most 30 blocks that cover (band, t), ascending in m, and
// goes through Y = sqrt(band sum): dband[b][band][t] = d / d (band sum) = sum / (2 Y), 0 where Y = 0.
__global__ void __launch_bounds__(256) stoi_band_grad_kernel(const double* blocks, const double* bands, const int* counts,
                                                             double* dband, int Fmax, int Jmax) {
  constexpr int N = kStoiSeg, NB = kStoiBands;
  const int t = blockIdx.x * 256 + threadIdx.x, band = blockIdx.y, b = blockIdx.z;
  int J = counts[b * 4 + 3];
  J = J > Jmax ? Jmax : J;
  const int F = counts[b * 4 + 2] - 1;
  if (t >= F || t >= Fmax) return;
  const int lo = t - (N - 1) > 0 ? t - (N - 1) : 0, hi = t < J - 1 ? t : J - 1;
  double sum = 0.0;
  for (int m = lo; m <= hi; ++m) sum += blocks[(((size_t)b * Jmax + m) * NB + band) * N + (t - m)];
  const double yv = bands[(((size_t)b * 2 + 1) * NB + band) * Fmax + t];
  dband[((size_t)b * NB + band) * Fmax + t] = yv > 0.0 ? sum / (2.0 * yv) : 0.0;
}

// ---------------------------------------------------------------------------------------- reverse of (c): band spectra
// grid (ceil(Fmax / 8), B), 256 threads: one workgroup per 8 consecutive frames of the silence-free processed signal.  The
// frames and the 212 (re, im) are recomputed exactly as stoi_bands_kernel computes them; thread tid < 212 then holds
// d re = 2 re dP, d im = 2 im dP of its bin with dP the sum, ascending in the band, of dband over the bands that hold the
// bin.  Thread j then runs the 212 bins ascending for the 8 frames at once,
//   dframe[b][t][j] = w[j] sum_bins (cos d re + sin d im)      twiddle (bin j) mod 512 of the caller's table,
// the gradient with respect to sample 128 t + j of the silence-free signal through frame t.
__global__ void __launch_bounds__(256) stoi_spectra_grad_kernel(const float* y, const int* counts, const int* kept,
                                                                const double* window, const int* bands,
                                                                const double* cossin, const double* dband, double* dframe,
                                                                int pitch, int F0max, int Fmax) {
  constexpr int T = kStoiFrameTile;
  __shared__ double s_f[kStoiW * T];                     // [sample][frame]
  __shared__ double2 s_cs[kStoiNfft];
  __shared__ double2 s_d[kStoiBins * T];                 // [bin][frame]: (d re, d im)
  const int tid = threadIdx.x, t0 = blockIdx.x * T, b = blockIdx.y;
  const int F = counts[b * 4 + 2] - 1;
  if (t0 >= F || counts[b * 4 + 3] <= 0) return;                              // the whole block leaves: no barrier follows
  const float* src = y + (size_t)b * pitch;
  const int* kp = kept + (size_t)b * F0max;
  s_cs[tid] = ((const double2*)cossin)[tid];
  s_cs[tid + 256] = ((const double2*)cossin)[tid + 256];
  const int jo = tid ^ 128;
  const double wj = window[tid], wo = window[jo];
#pragma unroll
  for (int r = 0; r < T; ++r) {
    const int t = t0 + r;
    double v = 0.0;
    if (t < F) {
      double a = wj * (double)src[(size_t)kp[t] * kStoiH + tid];
      const int other = tid < 128 ? t - 1 : t + 1;
      if (other >= 0) a += wo * (double)src[(size_t)kp[other] * kStoiH + jo];
      v = wj * a;
    }
    s_f[tid * T + r] = v;
  }
  __syncthreads();
  if (tid < kStoiBins) {
    double re[T], im[T];
#pragma unroll
    for (int r = 0; r < T; ++r) re[r] = 0.0, im[r] = 0.0;
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
    double dp[T];
#pragma unroll
    for (int r = 0; r < T; ++r) dp[r] = 0.0;
    for (int band = 0; band < kStoiBands; ++band) {
      int lo = bands[2 * band], hi = bands[2 * band + 1];
      lo = lo < kStoiBinLo ? kStoiBinLo : lo;
      hi = hi > kStoiBinLo + kStoiBins ? kStoiBinLo + kStoiBins : hi;
      if (bin >= lo && bin < hi) {
        const double* g = dband + ((size_t)b * kStoiBands + band) * Fmax;
#pragma unroll
        for (int r = 0; r < T; ++r)
          if (t0 + r < F) dp[r] += g[t0 + r];
      }
    }
#pragma unroll
    for (int r = 0; r < T; ++r) s_d[tid * T + r] = make_double2(2.0 * re[r] * dp[r], 2.0 * im[r] * dp[r]);
  }
  __syncthreads();
  double acc[T];
#pragma unroll
  for (int r = 0; r < T; ++r) acc[r] = 0.0;
  int idx = (kStoiBinLo * tid) & (kStoiNfft - 1);
#pragma unroll 2
  for (int k = 0; k < kStoiBins; ++k) {
    const double2 cs = s_cs[idx];
    idx = (idx + tid) & (kStoiNfft - 1);
#pragma unroll
    for (int r = 0; r < T; ++r) {
      const double2 d = s_d[k * T + r];
      acc[r] = fma(cs.x, d.x, acc[r]);
      acc[r] = fma(cs.y, d.y, acc[r]);
    }
  }
#pragma unroll
  for (int r = 0; r < T; ++r)
    if (t0 + r < F) dframe[((size_t)b * Fmax + t0 + r) * kStoiW + tid] = wj * acc[r];
}

// ------------------------------------------------------------------------------------------ reverse of the overlap-add
// grid (ceil(pitch / 256), B), 256 threads: a gather, one thread per sample n of y.  n lies in the original frames
// f = n / 128 - 1 and n / 128 (ascending); a kept one is silence-free frame i = inv[f] and put its sample j = n - 128 f,
// windowed, at p = 128 i + j of the silence-free signal, which the frames p / 128 - 1 and p / 128 of that signal read:
//   d_y[n] = sum_f w[j] (dframe[p / 128 - 1][p mod 128 + 128] + dframe[p / 128][p mod 128]),  frames outside [0, F) left out.
// Exact zeros at and behind the common length, in gated frames, behind the last frame, and in a row without a segment.
__global__ void __launch_bounds__(256) stoi_overlap_grad_kernel(const int* counts, const int* inv, const double* window,
                                                                const double* dframe, double* d_y, int pitch, int F0max,
                                                                int Fmax) {
  const int n = blockIdx.x * 256 + threadIdx.x, b = blockIdx.y;
  if (n >= pitch) return;
  const int len = counts[b * 4], F0 = counts[b * 4 + 1], F = counts[b * 4 + 2] - 1, J = counts[b * 4 + 3];
  double v = 0.0;
  if (n < len && J > 0) {
    const int* iv = inv + (size_t)b * F0max;
    const double* D = dframe + (size_t)b * Fmax * kStoiW;
    for (int f = n / kStoiH - 1; f <= n / kStoiH; ++f) {
      if (f < 0 || f >= F0 || f >= F0max) continue;
      const int i = iv[f];
      if (i < 0) continue;
      const int j = n - f * kStoiH;
      const int t = i + (j >= kStoiH), jj = j & (kStoiH - 1);
      double d = 0.0;
      if (t - 1 >= 0 && t - 1 < F) d += D[(size_t)(t - 1) * kStoiW + jj + kStoiH];
      if (t < F) d += D[(size_t)t * kStoiW + jj];
      v += window[j] * d;
    }
  }
  d_y[(size_t)b * pitch + n] = v;
}

// --------------------------------------------------------------------------------------------------------------- launch
hipError_t launch_stoi_backward(const float* y, const double* window, const int* bands, const double* cossin,
                                const double* g_rows, const StoiBuffers& saved, double* d_y, const StoiGeom& g,
                                const StoiGradBuffers& w, hipStream_t s) {
  hipLaunchKernelGGL(stoi_inverse_kernel, dim3(g.B), dim3(256), 0, s, saved.counts, saved.kept, w.inv, g.F0max);
  hipLaunchKernelGGL(stoi_segment_grad_kernel, dim3(g.Jmax, g.B), dim3(64), 0, s, saved.bands, saved.counts, g_rows,
                     w.blocks, g.Fmax, g.Jmax);
  hipLaunchKernelGGL(stoi_band_grad_kernel, dim3((g.Fmax + 255) / 256, kStoiBands, g.B), dim3(256), 0, s, w.blocks,
                     saved.bands, saved.counts, w.dband, g.Fmax, g.Jmax);
  hipLaunchKernelGGL(stoi_spectra_grad_kernel, dim3((g.Fmax + kStoiFrameTile - 1) / kStoiFrameTile, g.B), dim3(256), 0, s, y,
                     saved.counts, saved.kept, window, bands, cossin, w.dband, w.dframe, g.pitch, g.F0max, g.Fmax);
  hipLaunchKernelGGL(stoi_overlap_grad_kernel, dim3((g.pitch + 255) / 256, g.B), dim3(256), 0, s, saved.counts, w.inv,
                     window, w.dframe, d_y, g.pitch, g.F0max, g.Fmax);
  return hipGetLastError();
}

}  // namespace wg
