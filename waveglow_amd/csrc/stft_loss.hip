// Multi-resolution STFT loss (spectral convergence + log-magnitude L1) with its backward, fp32 on exact-fp32 MFMA
// (v_mfma_f32_32x32x2_f32), for any (n_fft, hop, win): n_fft a multiple of 32 up to 2048, 1 <= hop, win <= n_fft.
//
// One GEMM kernel serves the three transforms.  Rows of the basis are interleaved (re_k, im_k); the imaginary parts of
// bins 0 and n_fft/2 vanish, so row 1 carries re of bin n_fft/2 and the basis has exactly n_fft rows.  Only the taps
// under the window, [lpad, lpad + win), are multiplied (the others are zero in the basis).
//   forward  X[row][f] = sum_tap A[row][tap] xpad[f hop + tap]     A packed per M tile from global, the 64-frame x 64-tap
//            operand tile gathered from the audio (reflect padding as index arithmetic) into LDS
//   backward G[f][tap] = sum_row gX[row][f] A[row][tap]            the same products with the operand roles swapped, so
//            the accumulator holds taps on the lanes and G is written tap-contiguous; gX is formed from the saved
//            (re, im), M(y) and the device-side norms while the operand tile is staged
// then a gather sums, for every audio sample, the frame contributions of its (up to three, reflect padding) padded
// positions in ascending frame order.  Sums are reduced per thread and per workgroup in fp64 and combined by one
// fixed-order final kernel: no floating-point atomics anywhere.
//
// Ragged batches (a non-null lens): a device array lens gives utterance b its own N_b = lens[b] samples and
// F_b = N_b / hop + 1 frames inside the dense [B][n_samples] layout.  Reflections use N_b, frames f >= F_b add nothing
// and store nothing, a workgroup wholly behind its utterance does no GEMM, and the term count K sum_b F_b is formed on
// the device.  With lens == nullptr every kernel takes a uniform branch to the dense geometry.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "wg_host.h"
#include "wg_stftconv.h"

namespace wgsl {
using namespace wgsc;

constexpr int kMaxRes = 8;

enum { kFwdY = 0, kFwdX = 1, kFwdXSave = 2, kBwd = 3 };

struct GemmArgs {
  const float* A;        // packed fragments [MT][KS][64 lanes]
  int MT, KS, nby;       // M tiles, K steps of 2 (a multiple of 32), workgroups along M
  int n_fft, hop, lpad, N, F, Fp;
  float eps;
  const float* audio;    // forward: [B][N]
  float* xraw;           // [B][n_fft][Fp] rows of the prediction's transform (kFwdXSave writes, kBwd reads)
  float* my;             // [B][n_fft/2 + 1][Fp] M(target)
  double* part;          // kFwdX*: [workgroups][3] partial sums
  const double* sums;    // kBwd: S0 = sum (M(y) - M(x))^2, S1 = sum M(y)^2 of this resolution
  const float* g;        // kBwd: d loss / d (sc, mag, loss), device
  float fsc, fmag;       // kBwd: factor_sc, factor_mag
  float inv_res;         // kBwd: 1 / n_res
  double inv_cnt;        // kBwd: 1 / (B K F)
  float* G;              // kBwd: [B][F][Wp] frame gradients over the window taps
  int Wp;
  const int* lens;       // ragged batch: device [B] sample counts (N, F, Fp are then the pitches) or null
  int min_len;           // ragged batch: a length < min_len or > N counts as 0
  const double* cnt;     // kBwd, ragged batch: K sum_b F_b of this resolution, written by sl_final_kernel
};

// d loss / d M(x), divided by M(x): the factor of (re, im).  Zero under the clamp; sign(0) = 0.
__device__ __forceinline__ float grad_factor(float pw, float my, float eps, float cs, float cm) {
  if (!(pw >= eps)) return 0.0f;
  const float mx = sqrtf(pw);
  const float d = logf(my) - logf(mx);
  const float sg = d > 0.0f ? 1.0f : (d < 0.0f ? -1.0f : 0.0f);
  return (cs * (mx - my) - cm * sg / mx) / mx;
}

constexpr int kStB = kBN * (kKC / 2) / 256;   // backward: staged bins per thread and chunk

// backward operand of chunk kc: (re, im) and M(y) of bins 32 kc .. + 31 at 64 frames, read along the frames; element
// i = tid + 256 it is frame i & 63, bin 32 kc + (i >> 6).  Zeros (no gradient) outside the transform.
__device__ __forceinline__ void fetch_bwd(const GemmArgs& a, int kc, int f0, int b, int F, int tid, float (&pv)[kSt],
                                          float (&pm)[kStB], float& pm2) {
  const int half = a.n_fft / 2;
  const float* myb = a.my + (size_t)b * (half + 1) * a.Fp;
#pragma unroll
  for (int it = 0; it < kStB; ++it) {
    const int i = tid + 256 * it;
    const int f = f0 + (i & 63), p = kc * (kKC / 2) + (i >> 6);
    float re = 0.0f, im = 0.0f, my = 0.0f;
    if (f < F && p < half) {
      const float* xr = a.xraw + ((size_t)b * a.n_fft + 2 * p) * a.Fp + f;
      re = xr[0];
      im = xr[a.Fp];
      my = myb[(size_t)p * a.Fp + f];
      if (p == 0) pm2 = myb[(size_t)half * a.Fp + f];
    }
    pv[it] = re;
    pv[kStB + it] = im;
    pm[it] = my;
  }
}

template <int MODE, int TW>
__global__ void __launch_bounds__(256, 2) sl_gemm_kernel(const GemmArgs a) {
  __shared__ __attribute__((aligned(16))) float bt[kBN * kLd];
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int f0 = blockIdx.x * kBN, b = blockIdx.z;
  const int m0 = (int)((long long)blockIdx.y * a.MT / a.nby);
  const int m1 = (int)((long long)(blockIdx.y + 1) * a.MT / a.nby);   // at most 4 TW tiles
  const int col = lane & 31, kk = lane >> 5;
  const int half = a.n_fft / 2;

  int N = a.N, F = a.F;                                     // this utterance's samples and frames; a.N / a.F are the pitches
  if (a.lens) {
    N = ragged_len(a.lens, b, a.N, a.min_len);
    F = ragged_frames(N, a.hop);
    if (f0 >= F) {                                          // workgroup wholly behind the utterance: no GEMM
      if (MODE == kFwdX || MODE == kFwdXSave) {             // the final kernel adds every partial
        const size_t blk = ((size_t)blockIdx.z * gridDim.y + blockIdx.y) * gridDim.x + blockIdx.x;
        if (tid < 3) a.part[blk * 3 + tid] = 0.0;
      }
      return;
    }
  }

  float cs = 0.0f, cm = 0.0f;
  if (MODE == kBwd) {
    const double S0 = a.sums[0], S1 = a.sums[1];
    const float gsc = (a.g[0] + a.fsc * a.g[2]) * a.inv_res, gmag = (a.g[1] + a.fmag * a.g[2]) * a.inv_res;
    cs = S0 > 0.0 ? (float)((double)gsc / (sqrt(S0) * sqrt(S1))) : 0.0f;
    cm = (float)((double)gmag * (a.cnt ? 1.0 / a.cnt[0] : a.inv_cnt));   // a running workgroup has cnt >= K
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
  float pv[kSt], pm[kStB], pm2 = 0.0f;
  const int nkc = a.KS / 32;
  if (MODE != kBwd) fetch_fwd(a, 0, f0, b, N, F, tid, pv);
  else fetch_bwd(a, 0, f0, b, F, tid, pv, pm, pm2);
  for (int kc = 0; kc < nkc; ++kc) {
    __syncthreads();
    if (MODE != kBwd) {
      // bt[frame][tap]: 64 consecutive taps of 64 frames
#pragma unroll
      for (int it = 0; it < kSt; ++it) {
        const int i = tid + 256 * it;
        bt[(i >> 6) * kLd + (i & 63)] = pv[it];
      }
    } else {
      // bt[frame][row]: d (re, im) of 32 bins x 64 frames
#pragma unroll
      for (int it = 0; it < kStB; ++it) {
        const int i = tid + 256 * it;
        const int fr = i & 63, pl = i >> 6;
        const float re = pv[it], im = pv[kStB + it];
        float gre, gim;
        if (kc == 0 && pl == 0) {                           // rows 0, 1: re of bin 0 and of bin n_fft/2
          gre = re * grad_factor(power(re, 0.0f), pm[it], a.eps, cs, cm);
          gim = im * grad_factor(power(im, 0.0f), pm2, a.eps, cs, cm);
        } else {
          const float s = grad_factor(power(re, im), pm[it], a.eps, cs, cm);
          gre = s * re;
          gim = s * im;
        }
        bt[fr * kLd + 2 * pl] = gre;
        bt[fr * kLd + 2 * pl + 1] = gim;
      }
    }
    __syncthreads();
    if (kc + 1 < nkc) {
      if (MODE != kBwd) fetch_fwd(a, kc + 1, f0, b, N, F, tid, pv);
      else fetch_bwd(a, kc + 1, f0, b, F, tid, pv, pm, pm2);
    }
    mma_chunk<TW, MODE == kBwd>(acc, bt, a.A + (size_t)kc * 32 * 64 + lane, toff, col, kk);
  }

  if (MODE == kBwd) {
    // accumulator: tap on the lane (col), frame (r & 3) + 8 (r >> 2) + 4 kk in the registers
#pragma unroll
    for (int t = 0; t < TW; ++t) {
      const int mt = m0 + wave + 4 * t;
      if (mt >= m1) continue;
#pragma unroll
      for (int n = 0; n < 2; ++n)
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          const int f = f0 + n * 32 + (r & 3) + 8 * (r >> 2) + 4 * kk;
          if (f < F) a.G[((size_t)b * a.F + f) * a.Wp + mt * 32 + col] = acc[t][n][r];
        }
    }
    return;
  }

  double s0 = 0.0, s1 = 0.0, s2 = 0.0;
  float* myb = a.my + (size_t)b * (half + 1) * a.Fp;
#pragma unroll
  for (int t = 0; t < TW; ++t) {
    const int mt = m0 + wave + 4 * t;
    if (mt >= m1) continue;
#pragma unroll
    for (int n = 0; n < 2; ++n) {
      const int f = f0 + n * 32 + col;
      if (f >= F) continue;
#pragma unroll
      for (int g = 0; g < 4; ++g)
#pragma unroll
        for (int e = 0; e < 2; ++e) {
          const int row = mt * 32 + 8 * g + 4 * kk + 2 * e, p = row >> 1;
          const float re = acc[t][n][4 * g + 2 * e], im = acc[t][n][4 * g + 2 * e + 1];
          if (MODE == kFwdXSave) {
            float* xr = a.xraw + ((size_t)b * a.n_fft + row) * a.Fp + f;
            xr[0] = re;
            xr[a.Fp] = im;
          }
          // pair 0 holds two real bins (0 and n_fft/2), every other pair one complex bin
          const int nb = p == 0 ? 2 : 1;
          for (int q = 0; q < nb; ++q) {
            const float pw = p == 0 ? power(q ? im : re, 0.0f) : power(re, im);
            const size_t at = (size_t)(p == 0 && q ? half : p) * a.Fp + f;
            const float m = sqrtf(fmaxf(pw, a.eps));
            if (MODE == kFwdY) {
              myb[at] = m;
            } else {
              const float y = myb[at];
              const float d = y - m;
              s0 += (double)d * (double)d;
              s1 += (double)y * (double)y;
              s2 += (double)fabsf(logf(y) - logf(m));
            }
          }
        }
    }
  }
  if (MODE == kFwdY) return;
  __syncthreads();                                          // bt is free: reuse it for the workgroup sums
  double* sh = reinterpret_cast<double*>(bt);               // [3][256]
  sh[tid] = s0;
  sh[256 + tid] = s1;
  sh[512 + tid] = s2;
  __syncthreads();
  for (int s = 128; s > 0; s >>= 1) {
    if (tid < s) {
      sh[tid] += sh[tid + s];
      sh[256 + tid] += sh[256 + tid + s];
      sh[512 + tid] += sh[512 + tid + s];
    }
    __syncthreads();
  }
  if (tid < 3) {
    const size_t blk = ((size_t)blockIdx.z * gridDim.y + blockIdx.y) * gridDim.x + blockIdx.x;
    a.part[blk * 3 + tid] = sh[256 * tid];
  }
}

struct GatherArgs {
  const float* G;     // [B][F][Wp]
  float* gx;          // [B][N]
  int n_fft, hop, win, lpad, N, F, Wp, accumulate;
  const int* lens;    // ragged batch: device [B] sample counts (N and F are then the pitches) or null
  int min_len;
};

// d loss / d x[s]: the padded positions that hold x[s] (its own, and up to two reflected ones), each the sum over the
// frames that cover it, ascending.  One thread per sample.  grid (ceil(N / 256), B).
__global__ void __launch_bounds__(256) sl_gather_kernel(const GatherArgs a) {
  const int s = blockIdx.x * 256 + threadIdx.x, b = blockIdx.y;
  if (s >= a.N) return;
  const float* Gb = a.G + (size_t)b * a.F * a.Wp;
  const int h = a.n_fft / 2;
  int N = a.N, F = a.F;                                     // this utterance's samples and frames
  if (a.lens) {
    N = ragged_len(a.lens, b, a.N, a.min_len);
    F = ragged_frames(N, a.hop);
  }
  auto at = [&](int p) -> float {
    const int u = p - a.lpad;                               // tap offset of frame f: u - f hop in [0, win)
    if (u < 0) return 0.0f;
    int fhi = u / a.hop;
    if (fhi > F - 1) fhi = F - 1;
    const int flo = u - a.win + 1 <= 0 ? 0 : (u - a.win + a.hop) / a.hop;
    float v = 0.0f;
    for (int f = flo; f <= fhi; ++f) v += Gb[(size_t)f * a.Wp + (u - f * a.hop)];
    return v;
  };
  float v = 0.0f;
  if (s < N) {                                              // behind the utterance: 0
    v = at(s + h);
    if (s >= 1 && s <= h) v += at(h - s);
    if (s >= N - 1 - h && s <= N - 2) v += at(2 * (N - 1) - s + h);
  }
  float* o = a.gx + (size_t)b * a.N + s;
  *o = a.accumulate ? *o + v : v;
}

struct FinalArgs {
  const double* part[kMaxRes];
  int nblk[kMaxRes];
  double cnt[kMaxRes];
  int n_res;
  float fsc, fmag;
  double* sums;     // [n_res][2], then from sums + 2 kMaxRes the term counts [n_res] of a ragged batch
  float* out;       // sc, mag, fsc sc + fmag mag
  const int* lens;  // ragged batch: device [B] sample counts, or null (cnt is then the host's B K F)
  int B, N, min_len;
  int hop[kMaxRes], K[kMaxRes];
};

__global__ void __launch_bounds__(256) sl_final_kernel(const FinalArgs a) {
  __shared__ double sh[3 * 256];
  const int tid = threadIdx.x;
  double sc = 0.0, mag = 0.0;
  for (int r = 0; r < a.n_res; ++r) {
    double s[3] = {0.0, 0.0, 0.0};
    for (int i = tid; i < a.nblk[r]; i += 256)
      for (int q = 0; q < 3; ++q) s[q] += a.part[r][(size_t)i * 3 + q];
    __syncthreads();
    for (int q = 0; q < 3; ++q) sh[256 * q + tid] = s[q];
    __syncthreads();
    for (int w = 128; w > 0; w >>= 1) {
      if (tid < w)
        for (int q = 0; q < 3; ++q) sh[256 * q + tid] += sh[256 * q + tid + w];
      __syncthreads();
    }
    if (!a.lens) {
      if (tid == 0) {
        a.sums[2 * r] = sh[0];
        a.sums[2 * r + 1] = sh[256];
        sc += sqrt(sh[0]) / sqrt(sh[256]);
        mag += sh[512] / a.cnt[r];
      }
      continue;
    }
    // ragged batch: the term count K sum_b F_b, exact integers in fp64 whatever the order
    const double S0 = sh[0], S1 = sh[256], S2 = sh[512];
    double nf = 0.0;
    for (int b = tid; b < a.B; b += 256) nf += (double)ragged_frames(ragged_len(a.lens, b, a.N, a.min_len), a.hop[r]);
    __syncthreads();
    sh[tid] = nf;
    __syncthreads();
    for (int w = 128; w > 0; w >>= 1) {
      if (tid < w) sh[tid] += sh[tid + w];
      __syncthreads();
    }
    if (tid == 0) {
      const double cnt = (double)a.K[r] * sh[0];
      a.sums[2 * r] = S0;
      a.sums[2 * r + 1] = S1;
      a.sums[2 * kMaxRes + r] = cnt;
      if (cnt > 0.0) {                                      // no valid utterance: both terms are 0, not NaN
        sc += sqrt(S0) / sqrt(S1);
        mag += S2 / cnt;
      }
    }
  }
  if (tid == 0) {
    sc /= a.n_res;
    mag /= a.n_res;
    a.out[0] = (float)sc;
    a.out[1] = (float)mag;
    a.out[2] = (float)((double)a.fsc * sc + (double)a.fmag * mag);
  }
}

// workspace, in floats; every block a multiple of 64 floats
struct Layout {
  int F[kMaxRes], Fp[kMaxRes], nbx[kMaxRes], nby[kMaxRes];
  size_t xraw[kMaxRes], my[kMaxRes], part[kMaxRes], G, sums, total;
};

}  // namespace wgsl
using namespace wgsl;

struct wg_stftloss {
  int device = -1, n_res = 0;
  float eps = 1e-7f;
  Geom res[kMaxRes];
};

static bool layout(const wg_stftloss* h, int B, int N, bool saved, Layout& L) {
  if (!h || B < 1 || N < 1) return false;
  size_t off = 0, gmax = 0;
  for (int i = 0; i < h->n_res; ++i) {
    const Geom& r = h->res[i];
    if (N <= r.n_fft / 2) return false;                     // reflect padding needs N > n_fft / 2
    frame_counts(N, r.hop, L.F[i], L.Fp[i], L.nbx[i]);
    L.nby[i] = gemm_nby(r.MTf);
    L.my[i] = off;
    off += up64((size_t)B * (r.n_fft / 2 + 1) * L.Fp[i]);
    L.part[i] = off;
    off += up64((size_t)L.nbx[i] * L.nby[i] * B * 3 * 2);  // doubles
    L.xraw[i] = off;
    if (saved) {
      off += up64((size_t)B * r.n_fft * L.Fp[i]);
      const size_t g = up64((size_t)B * L.F[i] * r.MTb * 32);
      if (g > gmax) gmax = g;
    }
  }
  L.sums = off;
  off += up64((size_t)2 * 2 * kMaxRes);
  L.G = off;
  off += gmax;
  L.total = off;
  return true;
}

// The out-of-line part of wg_stftconv.h.
namespace wgsc {

int check_geom(const char* prefix, int n_fft, int hop, int win) {
  if (n_fft < 32 || n_fft > kMaxFft || n_fft % 32)
    return wg::fail(WG_ERR_INVALID, "%sn_fft must be a multiple of 32 in [32, 2048]", prefix);
  if (hop < 1 || hop > n_fft) return wg::fail(WG_ERR_INVALID, "%shop must be in [1, n_fft]", prefix);
  if (win < 1 || win > n_fft) return wg::fail(WG_ERR_INVALID, "%swin must be in [1, n_fft]", prefix);
  return WG_OK;
}

int upload_bases(Geom& r, const float* fb) {
  std::vector<float> af, ab;
  pack_bases(r, fb, af, ab);
  HIP_TRY(hipMalloc((void**)&r.d_Af, af.size() * 4));
  HIP_TRY(hipMalloc((void**)&r.d_Ab, ab.size() * 4));
  HIP_TRY(hipMemcpy(r.d_Af, af.data(), af.size() * 4, hipMemcpyHostToDevice));
  HIP_TRY(hipMemcpy(r.d_Ab, ab.data(), ab.size() * 4, hipMemcpyHostToDevice));
  return WG_OK;
}

void free_bases(Geom& r) {
  if (r.d_Af) (void)hipFree(r.d_Af);
  if (r.d_Ab) (void)hipFree(r.d_Ab);
  r.d_Af = r.d_Ab = nullptr;
}

hipError_t launch_gather(const Geom& r, const float* G, float* gx, int B, int N, int F, bool accumulate, const int* lens,
                         int min_len, hipStream_t s) {
  const GatherArgs ga{G, gx, r.n_fft, r.hop, r.win, r.lpad, N, F, r.MTb * 32, accumulate, lens, min_len};
  hipLaunchKernelGGL(sl_gather_kernel, dim3((N + 255) / 256, B), dim3(256), 0, s, ga);
  return hipGetLastError();
}

}  // namespace wgsc

// device part of wg_stftloss_create: the packed bases of every resolution
static int upload_all(wg_stftloss* h, const float* const* fwd_basis) {
  wg::DeviceGuard dev_guard;
  HIP_TRY(hipGetDevice(&dev_guard.prev));
  HIP_TRY(hipSetDevice(h->device));
  for (int i = 0; i < h->n_res; ++i)
    if (int rc = upload_bases(h->res[i], fwd_basis[i])) return rc;
  return WG_OK;
}

extern "C" {

int wg_stftloss_create(int32_t n_res, const int32_t* n_fft, const int32_t* hop, const int32_t* win,
                       const float* const* fwd_basis, float eps, int32_t device_id, wg_stftloss** out) {
  if (!n_fft || !hop || !win || !out) return wg::fail(WG_ERR_INVALID, "null argument");
  if (n_res < 1 || n_res > kMaxRes) return wg::fail(WG_ERR_INVALID, "stft loss: 1 to 8 resolutions");
  if (!(eps > 0.0f)) return wg::fail(WG_ERR_INVALID, "stft loss: eps must be positive");
  for (int i = 0; i < n_res; ++i)
    if (int rc = check_geom("stft loss: ", n_fft[i], hop[i], win[i])) return rc;
  if (device_id >= 0) {
    if (!fwd_basis) return wg::fail(WG_ERR_INVALID, "null argument");
    for (int i = 0; i < n_res; ++i)
      if (!fwd_basis[i]) return wg::fail(WG_ERR_INVALID, "null basis");
  }
  wg_stftloss* h = new wg_stftloss();
  h->device = device_id;
  h->n_res = n_res;
  h->eps = eps;
  for (int i = 0; i < n_res; ++i) set_geom(h->res[i], n_fft[i], hop[i], win[i]);
  if (device_id < 0) {   // planning handle: geometry and workspace sizes only
    *out = h;
    return WG_OK;
  }
  const int rc = upload_all(h, fwd_basis);
  if (rc != WG_OK) {
    wg_stftloss_destroy(h);
    return rc;
  }
  *out = h;
  return WG_OK;
}

int wg_stftloss_destroy(wg_stftloss* h) {
  if (!h) return WG_OK;
  for (int i = 0; i < h->n_res; ++i) free_bases(h->res[i]);
  delete h;
  return WG_OK;
}

size_t wg_stftloss_workspace_bytes(const wg_stftloss* h, int32_t B, int32_t n_samples, int32_t saved) {
  Layout L;
  if (!layout(h, B, n_samples, saved != 0, L)) return 0;
  return L.total * 4;
}

// Argument checks shared by the forward and the backward: null arguments, then sizes, then the workspace size, then the
// planning-handle refusal (the order of wg_melloss_*).
static int loss_check(const wg_stftloss* h, bool any_null, int32_t B, int32_t N, int32_t saved, size_t workspace_bytes,
                      Layout& L) {
  if (!h || any_null) return wg::fail(WG_ERR_INVALID, "null argument");
  if (saved != 0 && saved != 1) return wg::fail(WG_ERR_INVALID, "stft loss: saved must be 0 or 1");
  if (!layout(h, B, N, saved != 0, L) || B > 65535)
    return wg::fail(WG_ERR_INVALID, "stft loss: bad B, or n_samples <= max n_fft / 2");
  if (workspace_bytes < L.total * 4) return wg::fail(WG_ERR_WORKSPACE, "stft loss workspace too small");
  if (h->device < 0) return wg::fail(WG_ERR_STATE, "stft loss: planning handle (device_id < 0) cannot compute");
  return WG_OK;
}

// lens == nullptr: every row has n_samples samples.  Otherwise lens is a device array read by the kernels only.
int wg_stftloss_forward(wg_stftloss* h, const float* audio, const float* target, const int32_t* lens, float factor_sc,
                        float factor_mag, float* out3, int32_t B, int32_t N, int32_t saved, void* workspace,
                        size_t workspace_bytes, void* stream) {
  Layout L;
  const int rc = loss_check(h, !audio || !target || !out3 || !workspace, B, N, saved, workspace_bytes, L);
  if (rc != WG_OK) return rc;
  hipStream_t s = (hipStream_t)stream;
  float* ws = (float*)workspace;
  FinalArgs fa{};
  fa.n_res = h->n_res;
  fa.fsc = factor_sc;
  fa.fmag = factor_mag;
  fa.sums = (double*)(ws + L.sums);
  fa.out = out3;
  fa.lens = lens;
  fa.B = B;
  fa.N = N;
  fa.min_len = ragged_min_len(h->res, h->n_res);
  for (int i = 0; i < h->n_res; ++i) {
    const Geom& r = h->res[i];
    GemmArgs a{};
    a.A = r.d_Af;
    a.MT = r.MTf;
    a.KS = r.KSf;
    a.nby = L.nby[i];
    a.n_fft = r.n_fft;
    a.hop = r.hop;
    a.lpad = r.lpad;
    a.N = N;
    a.F = L.F[i];
    a.Fp = L.Fp[i];
    a.eps = h->eps;
    a.my = ws + L.my[i];
    a.xraw = saved ? ws + L.xraw[i] : nullptr;
    a.part = (double*)(ws + L.part[i]);
    a.lens = lens;
    a.min_len = fa.min_len;
    const dim3 grid(L.nbx[i], L.nby[i], B);
    a.audio = target;
    hipLaunchKernelGGL((sl_gemm_kernel<kFwdY, kTW>), grid, dim3(256), 0, s, a);
    HIP_TRY(hipGetLastError());
    a.audio = audio;
    if (saved) hipLaunchKernelGGL((sl_gemm_kernel<kFwdXSave, kTW>), grid, dim3(256), 0, s, a);
    else hipLaunchKernelGGL((sl_gemm_kernel<kFwdX, kTW>), grid, dim3(256), 0, s, a);
    HIP_TRY(hipGetLastError());
    fa.part[i] = a.part;
    fa.nblk[i] = L.nbx[i] * L.nby[i] * B;
    fa.cnt[i] = (double)B * (r.n_fft / 2 + 1) * L.F[i];
    fa.hop[i] = r.hop;
    fa.K[i] = r.n_fft / 2 + 1;
  }
  hipLaunchKernelGGL(sl_final_kernel, dim3(1), dim3(256), 0, s, fa);
  HIP_TRY(hipGetLastError());
  return WG_OK;
}

int wg_stftloss_backward(wg_stftloss* h, const float* g_out3, const int32_t* lens, float factor_sc, float factor_mag,
                         float* audio_grad_out, int32_t B, int32_t N, void* workspace, size_t workspace_bytes,
                         void* stream) {
  Layout L;
  const int rc = loss_check(h, !g_out3 || !audio_grad_out || !workspace, B, N, 1, workspace_bytes, L);
  if (rc != WG_OK) return rc;
  hipStream_t s = (hipStream_t)stream;
  float* ws = (float*)workspace;
  for (int i = 0; i < h->n_res; ++i) {
    const Geom& r = h->res[i];
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
    a.eps = h->eps;
    a.my = ws + L.my[i];
    a.xraw = ws + L.xraw[i];
    a.sums = (const double*)(ws + L.sums) + 2 * i;
    a.g = g_out3;
    a.fsc = factor_sc;
    a.fmag = factor_mag;
    a.inv_res = 1.0f / h->n_res;
    a.inv_cnt = 1.0 / ((double)B * (r.n_fft / 2 + 1) * L.F[i]);
    a.G = ws + L.G;
    a.Wp = r.MTb * 32;
    a.lens = lens;
    a.min_len = ragged_min_len(h->res, h->n_res);
    a.cnt = lens ? (const double*)(ws + L.sums) + 2 * kMaxRes + i : nullptr;
    const dim3 grid(L.nbx[i], a.nby, B);
    WGSC_LAUNCH_GEMM(sl_gemm_kernel, kBwd, grid, s, a);
    HIP_TRY(hipGetLastError());
    HIP_TRY(launch_gather(r, a.G, audio_grad_out, B, N, L.F[i], i > 0, lens, a.min_len, s));
  }
  return WG_OK;
}

}  // extern "C"
