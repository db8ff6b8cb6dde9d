// The conv-STFT core of stft_loss.hip and mel_loss.hip: one resolution's geometry and packed bases (host), and the pieces
// of the GEMM that both losses run over them (device).  The basis has n_fft rows, interleaved (re_k, im_k), row 1 the real
// part of bin n_fft/2; only the taps under the window, [lpad, lpad + win), are multiplied.  Each loss keeps its own GEMM
// kernel (staging, main loop, epilogue) and its own GemmArgs; the functions defined out of line are in stft_loss.hip.
#pragma once
#include <hip/hip_runtime.h>

#include <stddef.h>
#include <stdint.h>

#include <vector>

namespace wgsc {

constexpr int kMaxFft = 2048;
constexpr int kBN = 64;          // frames per workgroup; the frame pitch Fp is F rounded up to it
constexpr int kKC = 64;          // depth of one staged operand tile
constexpr int kLd = kKC + 1;     // LDS row stride: 32 frames of one k fall on 32 banks
constexpr int kTW = 4;           // M tiles per wave at most (x 2 frame tiles = 128 accumulator registers)
constexpr int kSt = kBN * kKC / 256;   // staged elements per thread and chunk

struct Geom {
  int n_fft, hop, win, lpad;
  int MTf, KSf, MTb, KSb;        // forward: n_fft/32 row tiles x window taps; backward: window tap tiles x n_fft rows
  float *d_Af = nullptr, *d_Ab = nullptr;   // packed MFMA fragments [MT][KS][64 lanes] of the windowed Fourier basis
};

inline void set_geom(Geom& r, int n_fft, int hop, int win) {
  r.n_fft = n_fft;
  r.hop = hop;
  r.win = win;
  r.lpad = (n_fft - win) / 2;
  r.MTf = n_fft / 32;
  r.KSf = (win + kKC - 1) / kKC * (kKC / 2);
  r.MTb = (win + 31) / 32;
  r.KSb = (n_fft + kKC - 1) / kKC * (kKC / 2);
}

// WG_OK, or WG_ERR_INVALID with a message that begins with `prefix` ("stft loss: ", "mel loss: ")
int check_geom(const char* prefix, int n_fft, int hop, int win);

// The fragments mma_chunk reads, from fb = [2 (n_fft/2 + 1)][n_fft], real rows then imaginary rows: lane l of K step ks
// holds row (l & 31) of its tile at depth 2 ks + (l >> 5).  Forward: tiles of basis rows, depth over the window taps;
// backward: tiles of window taps, depth over the basis rows.  Zero outside the basis.
inline void pack_bases(const Geom& r, const float* fb, std::vector<float>& af, std::vector<float>& ab) {
  const int n = r.n_fft, K = n / 2 + 1;
  auto basis = [&](int row, int tap) -> float {
    if (row >= n || tap >= n) return 0.0f;
    const int ref = row == 0 ? 0 : row == 1 ? n / 2 : (row & 1) ? K + (row >> 1) : (row >> 1);
    return fb[(size_t)ref * n + tap];
  };
  af.resize((size_t)r.MTf * r.KSf * 64);
  ab.resize((size_t)r.MTb * r.KSb * 64);
  for (int mt = 0; mt < r.MTf; ++mt)
    for (int ks = 0; ks < r.KSf; ++ks)
      for (int lane = 0; lane < 64; ++lane)
        af[((size_t)mt * r.KSf + ks) * 64 + lane] = basis(mt * 32 + (lane & 31), r.lpad + 2 * ks + (lane >> 5));
  for (int mt = 0; mt < r.MTb; ++mt)
    for (int ks = 0; ks < r.KSb; ++ks)
      for (int lane = 0; lane < 64; ++lane)
        ab[((size_t)mt * r.KSb + ks) * 64 + lane] = basis(2 * ks + (lane >> 5), r.lpad + mt * 32 + (lane & 31));
}

// d_Af and d_Ab on the current device (a WG_* code); free_bases takes a geometry in any state
int upload_bases(Geom& r, const float* fb);
void free_bases(Geom& r);

inline size_t up64(size_t n) { return (n + 63) / 64 * 64; }

// shortest length a ragged batch may hold: every resolution reflects about the utterance's own end
template <class G>
inline int ragged_min_len(const G* res, int n_res) {
  int n = 0;
  for (int i = 0; i < n_res; ++i) n = res[i].n_fft > n ? res[i].n_fft : n;
  return n / 2 + 1;
}

// frames of N samples, their pitch and the workgroups along them
inline void frame_counts(int N, int hop, int& F, int& Fp, int& nbx) {
  F = N / hop + 1;
  Fp = (F + kBN - 1) / kBN * kBN;
  nbx = Fp / kBN;
}

// workgroups along the MT tiles of a GEMM (at most 4 kTW tiles each), and the tiles per wave of the fullest one
inline int gemm_nby(int MT) { return (MT + 4 * kTW - 1) / (4 * kTW); }
inline int tiles_per_wave(int MT, int nby) { return ((MT + nby - 1) / nby + 3) / 4; }

// KERNEL<MODE, TW>(a) with as many tiles per wave as the fullest workgroup needs: a wave of a larger instance would
// compute its spare tiles for nothing (a tile past the end repeats the last one), and the arithmetic of a tile does not
// depend on the instance
#define WGSC_LAUNCH_GEMM(KERNEL, MODE, grid, s, a)                                    \
  switch (wgsc::tiles_per_wave((a).MT, (a).nby)) {                                    \
    case 1: hipLaunchKernelGGL((KERNEL<MODE, 1>), grid, dim3(256), 0, s, a); break;   \
    case 2: hipLaunchKernelGGL((KERNEL<MODE, 2>), grid, dim3(256), 0, s, a); break;   \
    case 3: hipLaunchKernelGGL((KERNEL<MODE, 3>), grid, dim3(256), 0, s, a); break;   \
    default: hipLaunchKernelGGL((KERNEL<MODE, 4>), grid, dim3(256), 0, s, a); break;  \
  }

// The gather that ends both backwards: gx[b][s] (= or, with accumulate, +=) the frame gradients G [B][F][32 MTb] of
// every padded position that holds sample s.  grid (ceil(N / 256), B) by 256.
hipError_t launch_gather(const Geom& r, const float* G, float* gx, int B, int N, int F, bool accumulate, const int* lens,
                         int min_len, hipStream_t s);

#if defined(__HIP__)

typedef float f32x16 __attribute__((ext_vector_type(16)));

// Sample count of utterance b in a ragged batch, as ragged_len of stft.hip: a length outside [min_len, pitch] counts as
// 0, the utterance then contributes nothing and nothing is indexed with it.
__device__ __forceinline__ int ragged_len(const int* lens, int b, int pitch, int min_len) {
  const int n = lens[b];
  return (n < min_len || n > pitch) ? 0 : n;
}
__device__ __forceinline__ int ragged_frames(int n, int hop) { return n ? n / hop + 1 : 0; }

// re^2 + im^2 with one rounding per operation, in the forward and in the backward alike, so both see the same clamp and
// equal (re, im) give equal bits in every kernel.  __fmul_rn / __fadd_rn are plain * and + in this toolchain, which the
// compiler may contract to an fma, differently from one kernel to the next (the backward of the STFT loss then saw
// M(x) != M(y) on equal frames): the pragma, on operations written out here, is what keeps the three roundings.
__device__ __forceinline__ float power(float re, float im) {
#pragma clang fp contract(off)
  const float a = re * re, b = im * im;
  return a + b;
}

// forward operand of chunk kc: taps lpad + 64 kc .. + 63 of 64 frames, read along the audio (reflect padding as index
// arithmetic); element i = tid + 256 it is frame i >> 6, tap i & 63.  Args: a GemmArgs with audio, N, lpad, n_fft, hop.
template <class Args>
__device__ __forceinline__ void fetch_fwd(const Args& a, int kc, int f0, int b, int N, int F, int tid,
                                          float (&pv)[kSt]) {
  const float* x = a.audio + (size_t)b * a.N;
  const int k0 = a.lpad + kc * kKC, half = a.n_fft / 2;
#pragma unroll
  for (int it = 0; it < kSt; ++it) {
    const int i = tid + 256 * it;
    const int f = f0 + (i >> 6), k = k0 + (i & 63);
    float v = 0.0f;
    if (f < F && k < a.n_fft) {
      int s = f * a.hop + k - half;
      if (s < 0) s = -s;
      if (s >= N) s = 2 * (N - 1) - s;
      v = x[s];
    }
    pv[it] = v;
  }
}

// 32 K steps of one staged chunk for the wave's TW tiles (tile t at ap + toff[t]) x 2 frame tiles, with no branch
// inside: a guard around a tile's load and MFMAs keeps the compiler from issuing the A loads ahead of the products.
// SWAP exchanges the operand roles: the accumulator then holds the transposed tile (basis index on the lanes).
template <int TW, bool SWAP>
__device__ __forceinline__ void mma_chunk(f32x16 (&acc)[TW][2], const float* bt, const float* ap,
                                          const size_t (&toff)[TW], int col, int kk) {
#pragma unroll 4
  for (int ks = 0; ks < 32; ++ks) {
    const float b0 = bt[col * kLd + 2 * ks + kk];
    const float b1 = bt[(32 + col) * kLd + 2 * ks + kk];
    float av[TW];
#pragma unroll
    for (int t = 0; t < TW; ++t) av[t] = ap[toff[t] + (size_t)ks * 64];
#pragma unroll
    for (int t = 0; t < TW; ++t) {
      if (SWAP) {
        acc[t][0] = __builtin_amdgcn_mfma_f32_32x32x2f32(b0, av[t], acc[t][0], 0, 0, 0);
        acc[t][1] = __builtin_amdgcn_mfma_f32_32x32x2f32(b1, av[t], acc[t][1], 0, 0, 0);
      } else {
        acc[t][0] = __builtin_amdgcn_mfma_f32_32x32x2f32(av[t], b0, acc[t][0], 0, 0, 0);
        acc[t][1] = __builtin_amdgcn_mfma_f32_32x32x2f32(av[t], b1, acc[t][1], 0, 0, 0);
      }
    }
  }
}

#endif  // __HIP__

}  // namespace wgsc
