// Denoiser (src/waveglow/denoiser.py:51-57) on exact-fp32 MFMA: conv-STFT (src/waveglow/stft.py:134-163) as a
// GEMM with the Hann-windowed Fourier basis, spectral subtraction + recombination in the epilogue, inverse STFT
// (stft.py:165-198) as a 4-tap polyphase GEMM with the pseudo-inverse basis, window-sum-square normalisation and
// cropping in its epilogue.  fp32 in / fp32 accumulate (v_mfma_f32_32x32x2_f32 is bit-for-bit an fp32 fma chain).
// Fixed geometry: filter 1024, hop 256 (TSTFTHParams defaults, taco_stft.py:36-43).
// Mel gradients (TacotronSTFT.mel_spectrogram_differentiable): mel_kernel also keeps the pre-log sums, mel_bwd_kernel
// turns d mel into d (re, im) in the inverse's [B][1056][Fs] layout, istft_kernel<true> is the transposed conv-STFT
// with the forward basis, and reflect_fold_kernel adds the reflect-padded edges back onto the audio gradient.
// With per-utterance lengths (a non-null lens) the three take the utterance's own frames and samples: d (re, im)
// behind its frames stays zero, the interior is stored up to its length, the edges fold about its own last sample.
// Denoiser gradients (Denoiser.forward_differentiable): stft_kernel<true> also keeps the raw (re, im), denoise_bwd_kernel
// turns d audio_out into d (re, im) (transposed istft + the epilogue's derivative), and the mel gradient's
// istft_kernel<true> + reflect_fold_kernel take that back to the audio.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "wg_stft.h"

namespace wg {

typedef float f32x16 __attribute__((ext_vector_type(16)));

constexpr int kMT = kRows / 32;        // 33

// LDS index of padded-audio position pos inside a 32-frame segment: one extra word per 256 so that the 32 lanes
// of a B-fragment read (same k, frames 256 apart) hit 32 different banks
__device__ __forceinline__ int seg_idx(int pos) { return pos + (pos >> 8); }

// Sample count of utterance b in a ragged batch (wg_stft_denoise, wg_stft_mel with lens).  A length the entry point
// does not allow (below min_len, above the row pitch, or with bits of mask set) counts as 0: the row comes out all zero
// and nothing is indexed with it.
__device__ __forceinline__ int ragged_len(const int* lens, int b, int pitch, int min_len, int mask) {
  const int n = lens[b];
  return (n < min_len || n > pitch || (n & mask)) ? 0 : n;
}
__device__ __forceinline__ int ragged_frames(int n) { return n ? n / kHop + 1 : 0; }

// kRaw = true (wg_stft_denoise_forward_saved): the same kernel also keeps (re, im) as the GEMM gave them in a.raw
template <bool kRaw>
__global__ void __launch_bounds__(512) stft_kernel(const StftArgs a) {
  __shared__ float seg[8960 + 40];
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int f0 = blockIdx.x * 32, b = blockIdx.y;
  const float* x = a.audio + (size_t)b * a.N;
  int N = a.N, F = a.F;                                 // this utterance's samples and frames; a.N / a.F are the pitches
  if (a.lens) {
    N = ragged_len(a.lens, b, a.N, a.min_len, a.len_mask);
    F = ragged_frames(N);
    if (f0 >= F) return;                                // tile wholly behind the utterance: its columns stay zero
  }
  for (int i = tid; i < 8960; i += 512) {
    int s = f0 * kHop + i - kFL / 2;                    // audio index of padded position (reflect, stft.py:141-147)
    if (s < 0) s = -s;
    if (s >= N) s = 2 * (N - 1) - s;
    seg[seg_idx(i)] = (s >= 0 && s < N) ? x[s] : 0.0f;
  }
  __syncthreads();
  constexpr int TPWV = 5;                               // M tiles per wave (wave w: w, w+8, ...; 33 tiles)
  f32x16 acc[TPWV];
#pragma unroll
  for (int t = 0; t < TPWV; ++t)
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[t][r] = 0.0f;
  const int col = lane & 31, kk = lane >> 5;
  const float* ap = a.fwdA + lane;
  for (int ks = 0; ks < kFL / 2; ++ks) {
    const float bv = seg[seg_idx(col * kHop + 2 * ks + kk)];
#pragma unroll
    for (int t = 0; t < TPWV; ++t) {
      const int mt = wave + 8 * t;
      if (mt < kMT) {
        const float av = ap[((size_t)mt * (kFL / 2) + ks) * 64];
        acc[t] = __builtin_amdgcn_mfma_f32_32x32x2f32(av, bv, acc[t], 0, 0, 0);
      }
    }
  }
  const int f = f0 + col;
#pragma unroll
  for (int t = 0; t < TPWV; ++t) {
    const int mt = wave + 8 * t;
    if (mt >= kMT) continue;
#pragma unroll
    for (int g = 0; g < 4; ++g) {
      const int row0 = mt * 32 + 8 * g + 4 * kk;        // rows row0..row0+3 = (re, im) of bins row0/2, row0/2+1
#pragma unroll
      for (int e = 0; e < 2; ++e) {
        const int bin = row0 / 2 + e;
        float re = acc[t][4 * g + 2 * e], im = acc[t][4 * g + 2 * e + 1];
        if (bin < kCut && f < F) {
          const float mag = sqrtf(re * re + im * im);
          if (a.mag0 && f == 0) a.mag0[(size_t)b * kCut + bin] = mag;
          if (a.mag) a.mag[((size_t)b * kCut + bin) * a.F + f] = mag;
          if (!a.rec) continue;
          if (kRaw) {
            float* wp = a.raw + ((size_t)b * kRows + row0 + 2 * e) * a.Fs + 3 + f;
            wp[0] = re;
            wp[a.Fs] = im;
          }
          if (a.bias) {                                // denoiser.py:54-55, recombined with the original phase
            const float md = fmaxf(mag - a.bias[bin] * a.strength, 0.0f);
            const float sc = mag > 0.0f ? md / mag : 0.0f;
            im = mag > 0.0f ? im * sc : 0.0f;
            re = mag > 0.0f ? re * sc : md;             // phase of (0,0) is 0: cos = 1
          }
          float* rp = a.rec + ((size_t)b * kRows + row0 + 2 * e) * a.Fs + 3 + f;
          rp[0] = re;
          rp[a.Fs] = im;
        }
      }
    }
  }
}

// Backward of istft_kernel<false> and of stft_kernel's denoiser epilogue in one GEMM of stft_kernel's shape:
//   gfull[n] = g[n - 512] 4 / ws(n) inside the utterance (4 alone where ws <= tiny), 0 in the cropped margins: the
//     transpose of the crop and the window-sum-square normalisation, so zero padding where the forward reflects;
//   gY[c][f] = sum_t inv[c][t] gfull[256 f + t]: a conv-STFT of gfull with the INVERSE basis (the transposed istft);
//   epilogue per (bin, frame) with the forward's raw (re, im), c = strength bias[bin], u = (re, im) / mag:
//     0 where mag == 0 and where mag - c < 0 (torch's clamp passes its bound);
//     phase_grad:  gX = ((mag - c) / mag) gY + (c / mag) (u . gY) u   (the derivative of max(mag - c, 0) X / mag)
//     otherwise:   gX = (u . gY) u            (the phase is a constant, as stft.py:160-161 detaches it)
// grid (ceil(F/32), B); one owner per gX cell, fixed fma order, no atomics.  gX comes zeroed: columns behind F, the
// pad rows and the tiles behind a shorter utterance are not written.
__global__ void __launch_bounds__(512) denoise_bwd_kernel(const DenoiseBwdArgs a) {
  __shared__ float seg[8960 + 40];
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int f0 = blockIdx.x * 32, b = blockIdx.y;
  const float* g = a.g + (size_t)b * a.N;
  int N = a.N, F = a.F;                                 // this utterance's samples and frames; a.N / a.F are the pitches
  if (a.lens) {
    N = ragged_len(a.lens, b, a.N, kFL, kHop - 1);
    F = ragged_frames(N);
    if (f0 >= F) return;                                // tile wholly behind the utterance: its columns stay zero
  }
  for (int i = tid; i < 8960; i += 512) {
    const int n = f0 * kHop + i;                        // position in the un-cropped inverse transform
    const int o = n - kFL / 2;
    float v = 0.0f;
    if (o >= 0 && o < N) {                              // g behind the utterance is never read
      const int q = n / kHop, r = n % kHop;
      float ws = 0.0f;                                  // window_sumsquare at n, summed as istft_kernel sums it
#pragma unroll
      for (int jj = 0; jj < 4; ++jj) {
        const int fr = q - jj;
        if (fr >= 0 && fr < F) ws += a.win_sq[r + kHop * jj];
      }
      v = g[o] * (float)(kFL / kHop);
      if (ws > 1.17549435e-38f) v /= ws;                // tiny(float32)
    }
    seg[seg_idx(i)] = v;
  }
  __syncthreads();
  constexpr int TPWV = 5;                               // M tiles per wave (wave w: w, w+8, ...; 33 tiles)
  f32x16 acc[TPWV];
#pragma unroll
  for (int t = 0; t < TPWV; ++t)
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[t][r] = 0.0f;
  const int col = lane & 31, kk = lane >> 5;
  const float* ap = a.invA + lane;
  for (int ks = 0; ks < kFL / 2; ++ks) {
    const float bv = seg[seg_idx(col * kHop + 2 * ks + kk)];
#pragma unroll
    for (int t = 0; t < TPWV; ++t) {
      const int mt = wave + 8 * t;
      if (mt < kMT) {
        const float av = ap[((size_t)mt * (kFL / 2) + ks) * 64];
        acc[t] = __builtin_amdgcn_mfma_f32_32x32x2f32(av, bv, acc[t], 0, 0, 0);
      }
    }
  }
  const int f = f0 + col;
#pragma unroll
  for (int t = 0; t < TPWV; ++t) {
    const int mt = wave + 8 * t;
    if (mt >= kMT) continue;
#pragma unroll
    for (int gq = 0; gq < 4; ++gq) {
      const int row0 = mt * 32 + 8 * gq + 4 * kk;       // rows row0..row0+3 = (re, im) of bins row0/2, row0/2+1
#pragma unroll
      for (int e = 0; e < 2; ++e) {
        const int bin = row0 / 2 + e;
        if (bin >= kCut || f >= F) continue;
        const float gre = acc[t][4 * gq + 2 * e], gim = acc[t][4 * gq + 2 * e + 1];
        const size_t i = ((size_t)b * kRows + row0 + 2 * e) * a.Fs + 3 + f;
        const float re = a.raw[i], im = a.raw[i + a.Fs];
        const float mag = sqrtf(re * re + im * im);     // the forward's own magnitude and clamp decision
        float c = 0.0f, d = mag;
        if (a.bias) {
          c = a.bias[bin] * a.strength;
          d = mag - a.bias[bin] * a.strength;
        }
        float xr = 0.0f, xi = 0.0f;
        if (mag > 0.0f && d >= 0.0f) {
          const float ur = re / mag, ui = im / mag;
          const float dn = ur * gre + ui * gim;
          if (a.phase_grad) {
            const float sc = d / mag, tc = (c / mag) * dn;
            xr = sc * gre + tc * ur;
            xi = sc * gim + tc * ui;
          } else {
            xr = dn * ur;
            xi = dn * ui;
          }
        }
        a.gX[i] = xr;
        a.gX[i + a.Fs] = xi;
      }
    }
  }
}

// kGrad = false: inverse STFT (stft.py:165-198).  kGrad = true: the same 4-tap polyphase GEMM with the forward basis
// is the transposed conv-STFT, g ypad[256 q + r] = sum_j sum_c fwd[c][r + 256 j] gX[c][q - j]; its epilogue stores the
// interior (audio positions 0..N-1) straight to out and the reflect-padded edges to a.edge; in a ragged batch N is the
// utterance's own length (513 or more, else 0) and out is 0 behind it.
template <bool kGrad>
__global__ void __launch_bounds__(512) istft_kernel(const IstftArgs a) {
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);   // M tile: output phase r in [32w, 32w+32)
  const int q0 = blockIdx.x * 32, b = blockIdx.y;
  const int col = lane & 31, kk = lane >> 5;
  int N = a.N, F = a.F;                                   // this utterance's samples and frames; a.N is the row pitch
  if (a.lens) {
    N = kGrad ? ragged_len(a.lens, b, a.N, kFL / 2 + 1, 0) : ragged_len(a.lens, b, a.N, kFL, kHop - 1);
    F = ragged_frames(N);
    // tile wholly behind the utterance (and, for the gradient, behind its right padding): zeros, no GEMM
    if (q0 * kHop - kFL / 2 >= N + (kGrad ? kFL / 2 : 0)) {
#pragma unroll
      for (int g = 0; g < 4; ++g)
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          const int o = (q0 + col) * kHop + wave * 32 + 8 * g + 4 * kk + e - kFL / 2;
          if (o < a.N) a.out[(size_t)b * a.N + o] = 0.0f;
        }
      return;
    }
  }
  f32x16 acc;
#pragma unroll
  for (int r = 0; r < 16; ++r) acc[r] = 0.0f;
  const float* ap = a.invA + (size_t)wave * 4 * (kRows / 2) * 64 + lane;
  const float* rb = a.rec + (size_t)b * kRows * a.Fs + 3 + q0 + col;
  for (int j = 0; j < 4; ++j) {
    for (int ks = 0; ks < kRows / 2; ++ks) {
      const float av = ap[((size_t)j * (kRows / 2) + ks) * 64];
      const float bv = rb[(size_t)(2 * ks + kk) * a.Fs - j];   // rec[c][q - j]; columns -3..-1 are zero
      acc = __builtin_amdgcn_mfma_f32_32x32x2f32(av, bv, acc, 0, 0, 0);
    }
  }
  const int q = q0 + col;
#pragma unroll
  for (int g = 0; g < 4; ++g) {
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const int r = wave * 32 + 8 * g + 4 * kk + e;
      const int n = q * kHop + r;                         // position in the un-cropped inverse transform
      const int o = n - kFL / 2;
      if (kGrad) {
        const float v = acc[4 * g + e];
        if (o >= 0 && o < N) a.out[(size_t)b * a.N + o] = v;
        else if (o < 0) a.edge[(size_t)b * kFL + n] = v;                      // n in [0, 512)
        else {
          if (o < N + kFL / 2) a.edge[(size_t)b * kFL + kFL / 2 + (o - N)] = v;
          if (o < a.N) a.out[(size_t)b * a.N + o] = 0.0f;                     // ragged batch: behind the utterance
        }
        continue;
      }
      if (o < 0 || o >= a.N) continue;
      if (o >= N) {                                       // ragged batch: zeros behind the utterance
        a.out[(size_t)b * a.N + o] = 0.0f;
        continue;
      }
      float ws = 0.0f;                                    // window_sumsquare at n (stft.py:45-95)
#pragma unroll
      for (int jj = 0; jj < 4; ++jj) {
        const int fr = q - jj;
        if (fr >= 0 && fr < F) ws += a.win_sq[r + kHop * jj];
      }
      float v = acc[4 * g + e];
      if (ws > 1.17549435e-38f) v /= ws;                  // tiny(float32)
      a.out[(size_t)b * a.N + o] = v * (float)(kFL / kHop);
    }
  }
}

// mel[b][m][f] = log(max(sum_k basis[m][k] |X|[b][k][f], 1e-5)): 80 x 513 MACs per frame, HBM/VALU-trivial.
// grid (ceil(F/64), B), 256 threads = 64 frames x 4 groups of mel rows.
__global__ void __launch_bounds__(256) mel_kernel(const MelArgs a) {
  const int f = blockIdx.x * 64 + (threadIdx.x & 63), grp = threadIdx.x >> 6, b = blockIdx.y;
  const int per = (a.n_mel + 3) / 4;
  float acc[32];
#pragma unroll
  for (int i = 0; i < 32; ++i) acc[i] = 0.0f;
  int F = a.F;                                            // this utterance's frames; a.F is the row pitch
  if (a.lens) {
    F = ragged_frames(ragged_len(a.lens, b, a.N, kFL / 2 + 1, 0));
    if ((int)blockIdx.x * 64 >= F) {                      // block wholly behind the utterance: zeros, magnitudes unread
      if (f < a.F)
        for (int m = grp; m < a.n_mel; m += 4) a.mel[((size_t)b * a.n_mel + m) * a.F + f] = 0.0f;
      return;
    }
  }
  const float* mp = a.mag + (size_t)b * kCut * a.F + (f < F ? f : F - 1);
  for (int k = 0; k < kCut; ++k) {
    const float v = mp[(size_t)k * a.F];
#pragma unroll
    for (int i = 0; i < 32; ++i) {
      const int m = grp * per + i;
      if (i < per && m < a.n_mel) acc[i] = fmaf(a.basis[(size_t)m * kCut + k], v, acc[i]);
    }
  }
  if (f >= a.F) return;
#pragma unroll
  for (int i = 0; i < 32; ++i) {
    const int m = grp * per + i;
    if (i < per && m < a.n_mel) {
      a.mel[((size_t)b * a.n_mel + m) * a.F + f] = f < F ? logf(fmaxf(acc[i], 1e-5f)) : 0.0f;
      if (a.pre) a.pre[((size_t)b * a.n_mel + m) * a.F + f] = acc[i];
    }
  }
}

// d mel -> d (re, im) for 64 frames x a quarter of the bins (blockIdx.z):
//   gA = g / A where A >= 1e-5 (torch's clamp passes its bound), else 0;  gmag[k] = sum_m basis[m][k] gA[m];
//   (g re, g im) = gmag (re, im) / mag, 0 where mag == 0.
// grid (ceil(F/64), B, 4), 256 threads = 64 frames x 4 waves; a wave's bin is uniform, so basis reads are broadcasts.
constexpr int kBwdSplit = 4;
__global__ void __launch_bounds__(256) mel_bwd_kernel(const MelBwdArgs a) {
  __shared__ float sg[128][64];
  const int fl = threadIdx.x & 63, b = blockIdx.y;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int f = blockIdx.x * 64 + fl;
  int F = a.F;                                            // this utterance's frames; a.F is the row pitch
  if (a.lens) {
    F = ragged_frames(ragged_len(a.lens, b, a.N, kFL / 2 + 1, 0));
    if ((int)blockIdx.x * 64 >= F) return;                // block wholly behind the utterance: gX stays zero
  }
  for (int m = wave; m < a.n_mel; m += 4) {
    float v = 0.0f;
    if (f < F) {
      const size_t i = ((size_t)b * a.n_mel + m) * a.F + f;
      const float A = a.pre[i];
      v = A >= 1e-5f ? a.g[i] / A : 0.0f;
    }
    sg[m][fl] = v;
  }
  __syncthreads();
  if (f >= F) return;
  const float* mp = a.mag + (size_t)b * kCut * a.F + f;
  const float* rp = a.rec + (size_t)b * kRows * a.Fs + 3 + f;
  float* gp = a.gX + (size_t)b * kRows * a.Fs + 3 + f;
  for (int k = blockIdx.z * 4 + wave; k < kCut; k += 4 * kBwdSplit) {
    const float* bp = a.basis + k;
    float gm = 0.0f;
    for (int m = 0; m < a.n_mel; ++m) gm = fmaf(bp[(size_t)m * kCut], sg[m][fl], gm);
    const float mag = mp[(size_t)k * a.F];
    const float s = mag > 0.0f ? gm / mag : 0.0f;
    gp[(size_t)(2 * k) * a.Fs] = s * rp[(size_t)(2 * k) * a.Fs];
    gp[(size_t)(2 * k + 1) * a.Fs] = s * rp[(size_t)(2 * k + 1) * a.Fs];
  }
}

// g y[s] += g ypad[512 - s] (1 <= s <= 512) + g ypad[2(N-1) - s + 512] (N-513 <= s <= N-2): the reflect padding of
// stft.py:141-147 folded back.  One thread per audio position, so overlapping edges of a short utterance do not race.
// grid (B), 256 threads; runs after istft_kernel<true> in stream order.  Ragged batch: N is the utterance's own length
// inside the row pitch, and an utterance that counts as 0 has nothing to fold.
__global__ void __launch_bounds__(256) reflect_fold_kernel(const float* edge, float* gy, int pitch, const int* lens) {
  const int b = blockIdx.x;
  const float* e = edge + (size_t)b * kFL;
  float* y = gy + (size_t)b * pitch;
  int N = pitch;
  if (lens) {
    N = ragged_len(lens, b, pitch, kFL / 2 + 1, 0);
    if (!N) return;
  }
  constexpr int kHalf = kFL / 2;
  for (int t = threadIdx.x; t < 2 * (kHalf + 1); t += 256) {
    const int s = t <= kHalf ? t : N - 2 * (kHalf + 1) + t;      // [0, 512] then [N-513, N-1]
    if (t > kHalf && s <= kHalf) continue;                        // already this block's lower range
    float v = y[s];
    if (s >= 1 && s <= kHalf) v += e[kHalf - s];
    if (s >= N - kHalf - 1 && s <= N - 2) v += e[kHalf + (N - 2 - s)];
    y[s] = v;
  }
}

hipError_t launch_mel_bwd(const MelBwdArgs& a, int B, hipStream_t s) {
  if (a.n_mel < 1 || a.n_mel > 128) return hipErrorInvalidValue;
  hipLaunchKernelGGL(mel_bwd_kernel, dim3((a.F + 63) / 64, B, kBwdSplit), dim3(256), 0, s, a);
  return hipGetLastError();
}

hipError_t launch_stft_grad(const IstftArgs& a, int B, hipStream_t s) {
  hipLaunchKernelGGL(istft_kernel<true>, dim3((a.F + 3 + 31) / 32, B), dim3(512), 0, s, a);
  const hipError_t e = hipGetLastError();
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(reflect_fold_kernel, dim3(B), dim3(256), 0, s, a.edge, a.out, a.N, a.lens);
  return hipGetLastError();
}

hipError_t launch_mel(const MelArgs& a, int B, hipStream_t s) {
  if (a.n_mel < 1 || a.n_mel > 128) return hipErrorInvalidValue;
  hipLaunchKernelGGL(mel_kernel, dim3((a.F + 63) / 64, B), dim3(256), 0, s, a);
  return hipGetLastError();
}

hipError_t launch_stft(const StftArgs& a, int B, hipStream_t s) {
  hipLaunchKernelGGL(stft_kernel<false>, dim3((a.F + 31) / 32, B), dim3(512), 0, s, a);
  return hipGetLastError();
}
hipError_t launch_stft_saved(const StftArgs& a, int B, hipStream_t s) {
  if (!a.rec || !a.raw) return hipErrorInvalidValue;
  hipLaunchKernelGGL(stft_kernel<true>, dim3((a.F + 31) / 32, B), dim3(512), 0, s, a);
  return hipGetLastError();
}
hipError_t launch_denoise_bwd(const DenoiseBwdArgs& a, int B, hipStream_t s) {
  hipLaunchKernelGGL(denoise_bwd_kernel, dim3((a.F + 31) / 32, B), dim3(512), 0, s, a);
  return hipGetLastError();
}
hipError_t launch_istft(const IstftArgs& a, int B, hipStream_t s) {
  hipLaunchKernelGGL(istft_kernel<false>, dim3((a.F + 3 + 31) / 32, B), dim3(512), 0, s, a);
  return hipGetLastError();
}

}  // namespace wg
