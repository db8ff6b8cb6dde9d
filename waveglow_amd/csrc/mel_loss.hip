// Multi-scale mel-spectrogram loss (log-mel L1 + linear-mel L1) with its backward, fp32 on exact-fp32 MFMA
// (v_mfma_f32_32x32x2_f32), for any scale (n_fft, hop, win, n_mels) inside the limits of stft_loss.hip.
//
// The two transforms and the transposed transform are the conv-STFT of stft_loss.hip, built from the same pieces
// (wg_stftconv.h: the packed bases, the operand tile gathered from the audio with the reflect padding as index arithmetic,
// the K loop of one chunk) around a GEMM kernel of its own.  Here the forward writes the (re, im) plane and nothing else,
// and the backward takes its operand from a plane of d loss / d (re, im) that ml_gspec_kernel has written: the mel
// projection sits between the transform and the loss, so the epilogue of the GEMM has nothing to reduce.
//
// The mel projection and its transpose are sparse: a row of the bank is multiplied over the span from its first to its
// last non-zero bin, a bin over the rows whose span covers it, both in ascending index order, one thread per output.
// Loss sums are reduced per thread and per workgroup in fp64 and combined by one fixed-order final kernel; overlapping
// frames are summed per sample in ascending frame order by the gather of stft_loss.hip.  No floating-point atomics.
//
// Ragged batches: a device array lens gives utterance b its own N_b = lens[b] samples and F_b = N_b / hop + 1 frames
// inside the dense layout.  Reflections use N_b, frames f >= F_b are neither stored nor read, a workgroup wholly behind
// its utterance does no work, and the cell count n_mels sum_b F_b is formed on the device.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "wg_melloss.h"

namespace wgml {

enum { kFwd = 0, kBwd = 1 };

struct GemmArgs {
  const float* A;        // packed fragments [MT][KS][64 lanes]
  int MT, KS, nby;       // M tiles, K steps of 2 (a multiple of 32), workgroups along M
  int n_fft, hop, lpad, N, F, Fp;
  const float* audio;    // kFwd: [B][N]
  float* spec;           // kFwd: [B][n_fft][Fp] rows of the transform, written for f < F_b
  const float* gspec;    // kBwd: [B][n_fft][Fp] d loss / d of those rows, read for f < F_b
  float* G;              // kBwd: [B][F][Wp] frame gradients over the window taps
  int Wp;
  const int* lens;       // ragged batch: device [B] sample counts (N, F, Fp are then the pitches) or null
  int min_len;           // ragged batch: a length < min_len or > N counts as 0
};

// backward operand of chunk kc: rows 64 kc .. + 63 of the gradient plane at 64 frames, read along the frames; element
// i = tid + 256 it is frame i & 63, row 64 kc + (i >> 6).  Zeros outside the transform.
__device__ __forceinline__ void fetch_bwd(const GemmArgs& a, int kc, int f0, int b, int F, int tid, float (&pv)[kSt]) {
#pragma unroll
  for (int it = 0; it < kSt; ++it) {
    const int i = tid + 256 * it;
    const int f = f0 + (i & 63), row = kc * kKC + (i >> 6);
    float v = 0.0f;
    if (f < F && row < a.n_fft) v = a.gspec[((size_t)b * a.n_fft + row) * a.Fp + f];
    pv[it] = v;
  }
}

// grid (Fp / 64, nby, B)
template <int MODE, int TW>
__global__ void __launch_bounds__(256, 2) ml_gemm_kernel(const GemmArgs a) {
  __shared__ __attribute__((aligned(16))) float bt[kBN * kLd];
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int f0 = blockIdx.x * kBN, b = blockIdx.z;
  const int m0 = (int)((long long)blockIdx.y * a.MT / a.nby);
  const int m1 = (int)((long long)(blockIdx.y + 1) * a.MT / a.nby);   // at most 4 TW tiles
  const int col = lane & 31, kk = lane >> 5;

  int N = a.N, F = a.F;                                     // this utterance's samples and frames; a.N / a.F are the pitches
  if (a.lens) {
    N = ragged_len(a.lens, b, a.N, a.min_len);
    F = ragged_frames(N, a.hop);
    if (f0 >= F) return;                                    // workgroup wholly behind the utterance: no GEMM
  }

  // wave w takes tiles m0 + w + 4 t < m1; a tile past the end repeats the last one (computed, never stored)
  size_t toff[TW];
#pragma unroll
  for (int t = 0; t < TW; ++t) {
    const int mt = m0 + wave + 4 * t;
    toff[t] = (size_t)(mt < m1 ? mt : m1 - 1) * a.KS * 64;
  }
  f32x16 acc[TW][2];
#pragma unroll
  for (int t = 0; t < TW; ++t)
#pragma unroll
    for (int n = 0; n < 2; ++n)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[t][n][r] = 0.0f;

  // The operand tile of chunk kc + 1 is loaded into registers before the products of chunk kc and written to LDS
  // after them, so its latency hides behind the MFMAs.
  float pv[kSt];
  const int nkc = a.KS / 32;
  if (MODE == kFwd) fetch_fwd(a, 0, f0, b, N, F, tid, pv);
  else fetch_bwd(a, 0, f0, b, F, tid, pv);
  for (int kc = 0; kc < nkc; ++kc) {
    __syncthreads();
#pragma unroll
    for (int it = 0; it < kSt; ++it) {
      const int i = tid + 256 * it;
      if (MODE == kFwd) bt[(i >> 6) * kLd + (i & 63)] = pv[it];    // bt[frame][tap]
      else bt[(i & 63) * kLd + (i >> 6)] = pv[it];                 // bt[frame][row]
    }
    __syncthreads();
    if (kc + 1 < nkc) {
      if (MODE == kFwd) fetch_fwd(a, kc + 1, f0, b, N, F, tid, pv);
      else fetch_bwd(a, kc + 1, f0, b, F, tid, pv);
    }
    // a wave with no tile of its own (fewer than four tiles in this workgroup) only stages
    if (m0 + wave < m1) mma_chunk<TW, MODE == kBwd>(acc, bt, a.A + (size_t)kc * 32 * 64 + lane, toff, col, kk);
  }

#pragma unroll
  for (int t = 0; t < TW; ++t) {
    const int mt = m0 + wave + 4 * t;
    if (mt >= m1) continue;
#pragma unroll
    for (int n = 0; n < 2; ++n)
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int q = (r & 3) + 8 * (r >> 2) + 4 * kk;      // accumulator row of register r
        if (MODE == kBwd) {                                 // tap on the lane, frame in the registers
          const int f = f0 + n * 32 + q;
          if (f < F) a.G[((size_t)b * a.F + f) * a.Wp + mt * 32 + col] = acc[t][n][r];
        } else {                                            // frame on the lane, basis row in the registers
          const int f = f0 + n * 32 + col;
          if (f < F) a.spec[((size_t)b * a.n_fft + mt * 32 + q) * a.Fp + f] = acc[t][n][r];
        }
      }
  }
}

// magnitude of bin k at frame f from the interleaved rows of one utterance's plane
__device__ __forceinline__ float bin_power(const float* sp, int k, int half, int Fp, int f, float& re, float& im) {
  if (k == 0 || k == half) {
    re = sp[(size_t)(k ? 1 : 0) * Fp + f];
    im = 0.0f;
  } else {
    re = sp[(size_t)(2 * k) * Fp + f];
    im = sp[(size_t)(2 * k + 1) * Fp + f];
  }
  return power(re, im);
}

struct MelArgs {
  const float* spec;     // [B][n_fft][Fp]
  const float* W;        // [n_mels][n_fft/2 + 1]
  const int* span;       // [n_mels][2]
  float* mel;            // out: [B][n_mels][Fp], written for f < F_b
  const float* mel_y;    // null (store only), or the target's mels: the two loss sums of this workgroup go to part
  double* part;          // [workgroups][2]
  int n_fft, n_mels, hop, N, F, Fp;
  float clamp;
  const int* lens;
  int min_len;
};

// mel[m][f] = sum_{k = first(m) .. last(m), ascending} W[m][k] M[k][f]; one thread per (row, frame), the frame on the
// lanes, wave w of workgroup y the rows 16 y + w + 4 i.  grid (Fp / 64, ceil(n_mels / 16), B).
__global__ void __launch_bounds__(256) ml_mel_kernel(const MelArgs a) {
  __shared__ double sh[2 * 256];
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int f0 = blockIdx.x * kBN, f = f0 + lane, b = blockIdx.z;
  const int half = a.n_fft / 2, K = half + 1;
  const size_t blk = ((size_t)blockIdx.z * gridDim.y + blockIdx.y) * gridDim.x + blockIdx.x;
  int F = a.F;
  if (a.lens) F = ragged_frames(ragged_len(a.lens, b, a.N, a.min_len), a.hop);
  if (f0 >= F) {                                            // the final kernel adds every partial
    if (a.mel_y && tid < 2) a.part[blk * 2 + tid] = 0.0;
    return;
  }
  const float* sp = a.spec + (size_t)b * a.n_fft * a.Fp;
  double s0 = 0.0, s1 = 0.0;
  if (f < F) {
    for (int i = 0; i < kMelRows / 4; ++i) {
      const int m = blockIdx.y * kMelRows + wave + 4 * i;
      if (m >= a.n_mels) break;
      const int k0 = a.span[2 * m], k1 = a.span[2 * m + 1];
      const float* w = a.W + (size_t)m * K;
      float acc = 0.0f;
      for (int k = k0; k <= k1; ++k) {
        float re, im;
        acc = __fmaf_rn(w[k], sqrtf(bin_power(sp, k, half, a.Fp, f, re, im)), acc);
      }
      const size_t at = ((size_t)b * a.n_mels + m) * a.Fp + f;
      a.mel[at] = acc;
      if (a.mel_y) {
        const float y = a.mel_y[at];
        s0 += fabs((double)logf(fmaxf(acc, a.clamp)) - (double)logf(fmaxf(y, a.clamp)));
        s1 += fabs((double)acc - (double)y);
      }
    }
  }
  if (!a.mel_y) return;
  sh[tid] = s0;
  sh[256 + tid] = s1;
  __syncthreads();
  for (int s = 128; s > 0; s >>= 1) {
    if (tid < s) {
      sh[tid] += sh[tid + s];
      sh[256 + tid] += sh[256 + tid + s];
    }
    __syncthreads();
  }
  if (tid < 2) a.part[blk * 2 + tid] = sh[256 * tid];
}

struct FinalArgs {
  const double* part[kMaxScales];
  int nblk[kMaxScales];
  double cnt[kMaxScales];          // dense batch: n_mels B F
  int hop[kMaxScales], n_mels[kMaxScales];
  int n_scales;
  float flog, flin;
  double* cnt_out;                 // [8]: the cell count of every scale, for the backward
  float* out;                      // log, lin, flog log + flin lin
  const int* lens;                 // ragged batch: device [B] sample counts, or null
  int B, N, min_len;
};

__global__ void __launch_bounds__(256) ml_final_kernel(const FinalArgs a) {
  __shared__ double sh[2 * 256];
  const int tid = threadIdx.x;
  double lg = 0.0, ln = 0.0;
  for (int r = 0; r < a.n_scales; ++r) {
    double s[2] = {0.0, 0.0};
    for (int i = tid; i < a.nblk[r]; i += 256)
      for (int q = 0; q < 2; ++q) s[q] += a.part[r][(size_t)i * 2 + q];
    __syncthreads();
    for (int q = 0; q < 2; ++q) sh[256 * q + tid] = s[q];
    __syncthreads();
    for (int w = 128; w > 0; w >>= 1) {
      if (tid < w)
        for (int q = 0; q < 2; ++q) sh[256 * q + tid] += sh[256 * q + tid + w];
      __syncthreads();
    }
    const double S0 = sh[0], S1 = sh[256];
    double cnt = a.cnt[r];
    if (a.lens) {                                           // n_mels sum_b F_b, exact integers in fp64 whatever the order
      double nf = 0.0;
      for (int b = tid; b < a.B; b += 256) nf += (double)ragged_frames(ragged_len(a.lens, b, a.N, a.min_len), a.hop[r]);
      __syncthreads();
      sh[tid] = nf;
      __syncthreads();
      for (int w = 128; w > 0; w >>= 1) {
        if (tid < w) sh[tid] += sh[tid + w];
        __syncthreads();
      }
      cnt = (double)a.n_mels[r] * sh[0];
    }
    if (tid == 0) {
      a.cnt_out[r] = cnt;
      if (cnt > 0.0) {                                      // no valid utterance: both terms are 0, not NaN
        lg += S0 / cnt;
        ln += S1 / cnt;
      }
    }
  }
  if (tid == 0) {
    for (int r = a.n_scales; r < kMaxScales; ++r) a.cnt_out[r] = 0.0;
    lg /= a.n_scales;
    ln /= a.n_scales;
    a.out[0] = (float)lg;
    a.out[1] = (float)ln;
    a.out[2] = (float)((double)a.flog * lg + (double)a.flin * ln);
  }
}

struct GmelArgs {
  const float *mel_x, *mel_y;   // [B][n_mels][Fp]
  float* gmel;                  // out: d loss / d mel(x), written for f < F_b
  const float* g;               // d loss / d (log, lin, loss), device
  const double* cnt;            // the cell count of this scale
  float flog, flin, inv_scales, clamp;
  int n_mels, hop, N, F, Fp;
  const int* lens;
  int min_len;
};

// d loss / d mel(x): the log term passes nothing under the clamp; sign(0) = 0.  grid (Fp / 64, ceil(n_mels / 4), B).
__global__ void __launch_bounds__(256) ml_gmel_kernel(const GmelArgs a) {
  const int f = blockIdx.x * kBN + (threadIdx.x & 63), m = blockIdx.y * 4 + (threadIdx.x >> 6), b = blockIdx.z;
  int F = a.F;
  if (a.lens) F = ragged_frames(ragged_len(a.lens, b, a.N, a.min_len), a.hop);
  if (f >= F || m >= a.n_mels) return;
  const double cnt = a.cnt[0];                              // >= n_mels here: this utterance has frames
  const float cl = (float)((double)((a.g[0] + a.flog * a.g[2]) * a.inv_scales) / cnt);
  const float cn = (float)((double)((a.g[1] + a.flin * a.g[2]) * a.inv_scales) / cnt);
  const size_t at = ((size_t)b * a.n_mels + m) * a.Fp + f;
  const float x = a.mel_x[at], y = a.mel_y[at];
  const float dl = logf(fmaxf(x, a.clamp)) - logf(fmaxf(y, a.clamp)), dn = x - y;
  const float sl = dl > 0.0f ? 1.0f : (dl < 0.0f ? -1.0f : 0.0f);
  const float sn = dn > 0.0f ? 1.0f : (dn < 0.0f ? -1.0f : 0.0f);
  const float inv = x >= a.clamp ? 1.0f / x : 0.0f;
  a.gmel[at] = cl * sl * inv + cn * sn;
}

struct GspecArgs {
  const float* spec;     // [B][n_fft][Fp] the prediction's transform
  const float* gmel;     // [B][n_mels][Fp]
  const float* W;
  const int* span;       // [n_mels][2] row spans, then [K][2] the rows covering each bin
  float* gspec;          // out: [B][n_fft][Fp], every row written for f < F_b
  int n_fft, n_mels, hop, N, F, Fp;
  const int* lens;
  int min_len;
};

// g_M[k][f] = sum_{m covering k, ascending} W[m][k] g_mel[m][f], then d (re, im) = (re, im) g_M / M, 0 where M = 0.
// One thread per (bin, frame), the frame on the lanes.  grid (Fp / 64, ceil((n_fft/2 + 1) / 16), B).
__global__ void __launch_bounds__(256) ml_gspec_kernel(const GspecArgs a) {
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int f = blockIdx.x * kBN + lane, b = blockIdx.z;
  const int half = a.n_fft / 2, K = half + 1;
  int F = a.F;
  if (a.lens) F = ragged_frames(ragged_len(a.lens, b, a.N, a.min_len), a.hop);
  if (f >= F) return;
  const float* sp = a.spec + (size_t)b * a.n_fft * a.Fp;
  float* gs = a.gspec + (size_t)b * a.n_fft * a.Fp;
  const float* gm = a.gmel + (size_t)b * a.n_mels * a.Fp;
  const int* cover = a.span + 2 * a.n_mels;
  for (int i = 0; i < kMelRows / 4; ++i) {
    const int k = blockIdx.y * kMelRows + wave + 4 * i;
    if (k >= K) break;
    const int mlo = cover[2 * k], mhi = cover[2 * k + 1];
    float g = 0.0f;
    for (int m = mlo; m <= mhi; ++m) {
      if (k < a.span[2 * m] || k > a.span[2 * m + 1]) continue;
      g = __fmaf_rn(a.W[(size_t)m * K + k], gm[(size_t)m * a.Fp + f], g);
    }
    float re, im;
    const float pw = bin_power(sp, k, half, a.Fp, f, re, im);
    const float s = pw > 0.0f ? g / sqrtf(pw) : 0.0f;
    if (k == 0 || k == half) {
      gs[(size_t)(k ? 1 : 0) * a.Fp + f] = s * re;
    } else {
      gs[(size_t)(2 * k) * a.Fp + f] = s * re;
      gs[(size_t)(2 * k + 1) * a.Fp + f] = s * im;
    }
  }
}

hipError_t launch_ml_forward(const wg_melloss* h, const Layout& L, const float* audio, const float* target,
                             const int* lens, float factor_log, float factor_lin, float* out3, float* spectra,
                             float* mels, float* tmp, int B, int N, hipStream_t s) {
  const bool saved = spectra != nullptr;
  float* tplane = tmp;                                      // the target's transform, one scale at a time
  float* part = tmp + L.plane_max;
  float* xplane = part + L.part_total;                      // values only: the prediction's transform, both mels, tail
  float* tmel = xplane + L.plane_max;
  double* cnt_out = (double*)(saved ? mels + L.tail : tmel + 2 * L.melp_max);
  FinalArgs fa{};
  fa.n_scales = h->n_scales;
  fa.flog = factor_log;
  fa.flin = factor_lin;
  fa.cnt_out = cnt_out;
  fa.out = out3;
  fa.lens = lens;
  fa.B = B;
  fa.N = N;
  fa.min_len = ragged_min_len(h->sc, h->n_scales);
  for (int i = 0; i < h->n_scales; ++i) {
    const Scale& r = h->sc[i];
    GemmArgs a{};
    a.A = r.d_Af;
    a.MT = r.MTf;
    a.KS = r.KSf;
    a.nby = gemm_nby(r.MTf);
    a.n_fft = r.n_fft;
    a.hop = r.hop;
    a.lpad = r.lpad;
    a.N = N;
    a.F = L.F[i];
    a.Fp = L.Fp[i];
    a.lens = lens;
    a.min_len = fa.min_len;
    MelArgs m{};
    m.W = r.d_W;
    m.span = r.d_span;
    m.part = (double*)(part + L.part[i]);
    m.n_fft = r.n_fft;
    m.n_mels = r.n_mels;
    m.hop = r.hop;
    m.N = N;
    m.F = L.F[i];
    m.Fp = L.Fp[i];
    m.clamp = h->clamp;
    m.lens = lens;
    m.min_len = fa.min_len;
    float* mel_x = saved ? mels + L.melx[i] : tmel;
    float* mel_y = saved ? mels + L.mely[i] : tmel + L.melp_max;
    const dim3 grid(L.nbx[i], a.nby, B), mgrid(L.nbx[i], L.nmy[i], B);
    a.audio = target;
    a.spec = tplane;
    WGSC_LAUNCH_GEMM(ml_gemm_kernel, kFwd, grid, s, a);
    if (hipError_t e = hipGetLastError()) return e;
    m.spec = tplane;
    m.mel = mel_y;
    m.mel_y = nullptr;
    hipLaunchKernelGGL(ml_mel_kernel, mgrid, dim3(256), 0, s, m);
    if (hipError_t e = hipGetLastError()) return e;
    a.audio = audio;
    a.spec = saved ? spectra + L.spec[i] : xplane;
    WGSC_LAUNCH_GEMM(ml_gemm_kernel, kFwd, grid, s, a);
    if (hipError_t e = hipGetLastError()) return e;
    m.spec = a.spec;
    m.mel = mel_x;
    m.mel_y = mel_y;
    hipLaunchKernelGGL(ml_mel_kernel, mgrid, dim3(256), 0, s, m);
    if (hipError_t e = hipGetLastError()) return e;
    fa.part[i] = m.part;
    fa.nblk[i] = L.nbx[i] * L.nmy[i] * B;
    fa.cnt[i] = (double)B * r.n_mels * L.F[i];
    fa.hop[i] = r.hop;
    fa.n_mels[i] = r.n_mels;
  }
  hipLaunchKernelGGL(ml_final_kernel, dim3(1), dim3(256), 0, s, fa);
  if (hipError_t e = hipGetLastError()) return e;
  return hipSuccess;
}

hipError_t launch_ml_backward(const wg_melloss* h, const Layout& L, const float* g_out3, const int* lens,
                              float factor_log, float factor_lin, const float* spectra, const float* mels,
                              float* audio_grad_out, float* tmp, int B, int N, hipStream_t s) {
  float* gspec = tmp;
  float* gmel = tmp + L.plane_max;
  float* G = gmel + L.melp_max;
  const int min_len = ragged_min_len(h->sc, h->n_scales);
  for (int i = 0; i < h->n_scales; ++i) {
    const Scale& r = h->sc[i];
    GmelArgs gm{};
    gm.mel_x = mels + L.melx[i];
    gm.mel_y = mels + L.mely[i];
    gm.gmel = gmel;
    gm.g = g_out3;
    gm.cnt = (const double*)(mels + L.tail) + i;
    gm.flog = factor_log;
    gm.flin = factor_lin;
    gm.inv_scales = 1.0f / h->n_scales;
    gm.clamp = h->clamp;
    gm.n_mels = r.n_mels;
    gm.hop = r.hop;
    gm.N = N;
    gm.F = L.F[i];
    gm.Fp = L.Fp[i];
    gm.lens = lens;
    gm.min_len = min_len;
    hipLaunchKernelGGL(ml_gmel_kernel, dim3(L.nbx[i], (r.n_mels + 3) / 4, B), dim3(256), 0, s, gm);
    if (hipError_t e = hipGetLastError()) return e;
    GspecArgs gs{};
    gs.spec = spectra + L.spec[i];
    gs.gmel = gmel;
    gs.W = r.d_W;
    gs.span = r.d_span;
    gs.gspec = gspec;
    gs.n_fft = r.n_fft;
    gs.n_mels = r.n_mels;
    gs.hop = r.hop;
    gs.N = N;
    gs.F = L.F[i];
    gs.Fp = L.Fp[i];
    gs.lens = lens;
    gs.min_len = min_len;
    const int K = r.n_fft / 2 + 1;
    hipLaunchKernelGGL(ml_gspec_kernel, dim3(L.nbx[i], (K + kMelRows - 1) / kMelRows, B), dim3(256), 0, s, gs);
    if (hipError_t e = hipGetLastError()) return e;
    GemmArgs a{};
    a.A = r.d_Ab;
    a.MT = r.MTb;
    a.KS = r.KSb;
    a.nby = gemm_nby(r.MTb);
    a.n_fft = r.n_fft;
    a.hop = r.hop;
    a.lpad = r.lpad;
    a.N = N;
    a.F = L.F[i];
    a.Fp = L.Fp[i];
    a.gspec = gspec;
    a.G = G;
    a.Wp = r.MTb * 32;
    a.lens = lens;
    a.min_len = min_len;
    const dim3 grid(L.nbx[i], a.nby, B);
    WGSC_LAUNCH_GEMM(ml_gemm_kernel, kBwd, grid, s, a);
    if (hipError_t e = hipGetLastError()) return e;
    if (hipError_t e = launch_gather(r, G, audio_grad_out, B, N, L.F[i], i > 0, lens, min_len, s)) return e;
  }
  return hipSuccess;
}

}  // namespace wgml
