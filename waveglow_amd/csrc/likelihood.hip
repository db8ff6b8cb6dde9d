// gfx950 kernels of the per-utterance likelihood (include/waveglow_amd.h: wg_nll): the negative log-likelihood that
// WaveGlowLoss (src/waveglow/train.py:31-45) takes of a whole batch, per utterance and per mel frame, from the z and
// log_s of the no-grad forward (src/waveglow/model.py:178-221; wg_forward).
//
//   nll_frames_kernel   one workgroup per (utterance b, mel frame q): its 32 columns of the 8 z rows and of every log_s
//                       row (8 + sum_k h_k rows x 128 bytes, 5.6 KB at the default model) -> three fp64 partials
//   nll_rows_kernel     one workgroup per utterance: its frames' partials -> the row of eight figures
//
// All sums are fp64 in an order fixed by (row, column) alone -- per-thread serial sums, shuffle trees, no atomics -- so a
// call gives the same bits every time, and an utterance gives the bits of its own call whatever batch, pitch (n_frames) or
// neighbours it has.  Nothing here reads a count on the host.
#include "wg_likelihood.h"

namespace wg {

namespace {

// columns of utterance b: 32 * frames[b], 0 for a count outside [1, n_frames_max]; L without counts
__device__ __forceinline__ int nll_cols(const int* frames, int b, int L, int n_frames_max) {
  if (frames == nullptr) return L;
  const int f = frames[b];
  return (unsigned)f - 1u < (unsigned)n_frames_max ? kNllFrameCols * f : 0;
}

// sum over the 64 lanes of a wave (valid in lane 0), then over the 4 waves of the workgroup in wave order (valid in thread 0)
__device__ __forceinline__ double block_sum(double v, double* s_part) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o);
  __syncthreads();                       // s_part may still be read from the previous call
  if ((threadIdx.x & 63) == 0) s_part[threadIdx.x >> 6] = v;
  __syncthreads();
  return ((s_part[0] + s_part[1]) + s_part[2]) + s_part[3];
}

// Thread (slot = tid >> 3, piece = tid & 7) reads the 16-byte piece `piece` of the frame's 128 bytes of rows slot, slot + 32,
// ...: 8 consecutive lanes cover one row's 128 contiguous bytes, a wave covers 8 rows with 16-byte loads.  VEC: L % 4 == 0
// and 16-byte aligned planes (always so for a ragged batch, L = 32 n_frames); otherwise the same four values one by one.
template <bool VEC>
__global__ void __launch_bounds__(256) nll_frames_kernel(const float* __restrict__ z, const NllPlanes pl, const int* __restrict__ frames,
                                                         int L, int n_frames_max, double inv_2s2, double logdet_sum, int last,
                                                         double* __restrict__ part, double* __restrict__ frame_out) {
  __shared__ double s_part[4];
  const int q = blockIdx.x, b = blockIdx.y, NF = gridDim.x;
  const int Lb = nll_cols(frames, b, L, n_frames_max);
  const int col0 = q * kNllFrameCols;
  const size_t slot_out = (size_t)b * NF + q;
  if (col0 >= Lb) {                      // behind the utterance: nothing is read
    if (last && frame_out != nullptr && threadIdx.x == 0) frame_out[slot_out] = __longlong_as_double(0x7ff8000000000000ll);
    return;
  }
  const int slot = threadIdx.x >> 3, c = col0 + 4 * (threadIdx.x & 7);
  const int live = Lb - c < 4 ? (Lb - c < 0 ? 0 : Lb - c) : 4;       // VEC: 0 or 4
  auto load4 = [&](const float* row, float (&v)[4]) {
    if (VEC) {
      const float4 t = live ? *(const float4*)(row + c) : make_float4(0.f, 0.f, 0.f, 0.f);
      v[0] = t.x, v[1] = t.y, v[2] = t.z, v[3] = t.w;
    } else {
#pragma unroll
      for (int j = 0; j < 4; ++j) v[j] = j < live ? row[c + j] : 0.0f;
    }
  };
  double z2 = 0.0, zs = 0.0, ls = 0.0;
  float v[4];
  if (z != nullptr && slot < 8) {
    load4(z + ((size_t)b * 8 + slot) * L, v);
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      z2 += (double)v[j] * (double)v[j];
      zs += (double)v[j];
    }
  }
  // log_s rows in flow order: row r of the launch = (plane i, channel r - first row of plane i)
  int r0 = 0;
  for (int i = 0; i < pl.n; ++i) {
    const int h = pl.h[i];
    for (int r = slot; r < r0 + h; r += 32) {
      if (r < r0) continue;
      load4(pl.p[i] + ((size_t)b * h + (r - r0)) * L, v);
      ls += ((double)v[0] + (double)v[1]) + ((double)v[2] + (double)v[3]);
    }
    r0 += h;
  }
  const double t_z2 = block_sum(z2, s_part), t_zs = block_sum(zs, s_part), t_ls = block_sum(ls, s_part);
  if (threadIdx.x != 0) return;
  double* p = part + slot_out * kNllPart;
  double a_z2 = t_z2, a_ls = t_ls, a_zs = t_zs;
  if (z == nullptr) a_z2 = p[0], a_ls = p[1] + t_ls, a_zs = p[2];     // a later launch of the same call: more flows
  p[0] = a_z2, p[1] = a_ls, p[2] = a_zs;
  if (last && frame_out != nullptr) {
    const int cols = Lb - col0 < kNllFrameCols ? Lb - col0 : kNllFrameCols;
    frame_out[slot_out] = (a_z2 * inv_2s2 - a_ls - (double)cols * logdet_sum) / 256.0;
  }
}

__global__ void __launch_bounds__(256) nll_rows_kernel(const double* __restrict__ part, const int* __restrict__ frames, int L,
                                                       int n_frames_max, int NF, double inv_2s2, double half_log_2pis2,
                                                       double logdet_sum, double* __restrict__ rows) {
  __shared__ double s_part[4];
  const int b = blockIdx.x;
  const int Lb = nll_cols(frames, b, L, n_frames_max);
  const int nf = (Lb + kNllFrameCols - 1) / kNllFrameCols;
  double z2 = 0.0, ls = 0.0, zs = 0.0;
  for (int q = threadIdx.x; q < nf; q += 256) {
    const double* p = part + ((size_t)b * NF + q) * kNllPart;
    z2 += p[0], ls += p[1], zs += p[2];
  }
  const double t_z2 = block_sum(z2, s_part), t_ls = block_sum(ls, s_part), t_zs = block_sum(zs, s_part);
  if (threadIdx.x != 0) return;
  const double n = 8.0 * (double)Lb, log_det = (double)Lb * logdet_sum;
  const double nll = (t_z2 * inv_2s2 - t_ls - log_det) / n;            // train.py:43-44 of this utterance alone
  const double mean = t_zs / n;
  double* r = rows + (size_t)b * kNllRow;
  r[0] = nll;
  r[1] = (nll + half_log_2pis2) / 0.6931471805599453094;               // + the constant the training loss drops, in bits
  r[2] = t_z2;
  r[3] = t_ls;
  r[4] = log_det;
  r[5] = n;
  r[6] = mean;
  r[7] = t_z2 / n - mean * mean;
}

}  // namespace

hipError_t launch_nll_frames(const float* z, const NllPlanes& pl, const int* frames, int B, int L, int n_frames_max,
                             double inv_2s2, double logdet_sum, int last, double* part, double* frame_out, hipStream_t s) {
  if (B < 1 || B > 65535 || L < 1 || pl.n < 0 || pl.n > kNllMaxPlanes) return hipErrorInvalidValue;
  const int NF = (L + kNllFrameCols - 1) / kNllFrameCols;
  bool vec = L % 4 == 0 && (z == nullptr || (uintptr_t)z % 16 == 0);
  for (int i = 0; i < pl.n; ++i) {
    if (pl.p[i] == nullptr || pl.h[i] < 1) return hipErrorInvalidValue;
    vec = vec && (uintptr_t)pl.p[i] % 16 == 0;
  }
  const dim3 grid((unsigned)NF, (unsigned)B);
  if (vec)
    hipLaunchKernelGGL(nll_frames_kernel<true>, grid, dim3(256), 0, s, z, pl, frames, L, n_frames_max, inv_2s2, logdet_sum, last,
                       part, frame_out);
  else
    hipLaunchKernelGGL(nll_frames_kernel<false>, grid, dim3(256), 0, s, z, pl, frames, L, n_frames_max, inv_2s2, logdet_sum, last,
                       part, frame_out);
  return hipGetLastError();
}

hipError_t launch_nll_rows(const double* part, const int* frames, int B, int L, int n_frames_max, double inv_2s2,
                           double half_log_2pis2, double logdet_sum, double* rows, hipStream_t s) {
  if (B < 1 || L < 1) return hipErrorInvalidValue;
  const int NF = (L + kNllFrameCols - 1) / kNllFrameCols;
  hipLaunchKernelGGL(nll_rows_kernel, dim3((unsigned)B), dim3(256), 0, s, part, frames, L, n_frames_max, NF, inv_2s2,
                     half_log_2pis2, logdet_sum, rows);
  return hipGetLastError();
}

}  // namespace wg
