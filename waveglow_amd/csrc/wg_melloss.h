// Handle, buffer layouts and launch entry points of mel_loss.hip, shared with mel_loss_api.cpp (host).
#pragma once
#include <hip/hip_runtime.h>

#include <stddef.h>
#include <stdint.h>

#include "wg_stftconv.h"

namespace wgml {
using namespace wgsc;            // the projection kernels take kBN frames per workgroup, as the GEMM

constexpr int kMaxScales = 8;
constexpr int kMelRows = 16;     // mel rows (forward) or bins (backward) per workgroup of the projection kernels

struct Scale : Geom {
  int n_mels;
  float* d_W = nullptr;          // the dense bank [n_mels][n_fft/2 + 1]
  int* d_span = nullptr;         // [n_mels][2] first and last non-zero bin of a row (first > last: an empty row), then
                                 // [n_fft/2 + 1][2] lowest and highest row whose span covers a bin (lowest > highest: none)
};

// Offsets in floats; every block a multiple of 64 floats.
//   spectra: per scale r   [B][n_fft][Fp_r]          rows interleaved: row 0 = re of bin 0, row 1 = re of bin n_fft/2,
//                                                    rows 2p, 2p + 1 = (re, im) of bin p for 1 <= p < n_fft/2
//   mels:    per scale r   [B][n_mels][Fp_r] of the prediction, then the same of the target (linear mels);
//            then 64 floats: fp64 [8], element r the cell count n_mels sum_b F_b of scale r
struct Layout {
  int F[kMaxScales], Fp[kMaxScales], nbx[kMaxScales], nmy[kMaxScales];
  size_t spec[kMaxScales], spectra_total;
  size_t melx[kMaxScales], mely[kMaxScales], tail, mels_total;
  size_t part[kMaxScales], part_total;       // per-workgroup partial sums: fp64 [blocks][2], offsets in floats
  size_t plane_max, melp_max, g_max;         // largest transform plane, mel plane and frame-gradient block of any scale
};

}  // namespace wgml

struct wg_melloss {
  int device = -1, n_scales = 0;
  float clamp = 1e-5f;
  wgml::Scale sc[wgml::kMaxScales];
};

namespace wgml {

inline bool make_layout(const wg_melloss* h, int B, int N, Layout& L) {
  if (!h || B < 1 || B > 65535 || N < 1) return false;
  size_t so = 0, mo = 0, po = 0;
  L.plane_max = L.melp_max = L.g_max = 0;
  for (int i = 0; i < h->n_scales; ++i) {
    const Scale& r = h->sc[i];
    if (N <= r.n_fft / 2) return false;                     // reflect padding needs N > n_fft / 2
    frame_counts(N, r.hop, L.F[i], L.Fp[i], L.nbx[i]);
    L.nmy[i] = (r.n_mels + kMelRows - 1) / kMelRows;
    const size_t plane = up64((size_t)B * r.n_fft * L.Fp[i]), melp = up64((size_t)B * r.n_mels * L.Fp[i]);
    const size_t g = up64((size_t)B * L.F[i] * r.MTb * 32);
    L.spec[i] = so;
    so += plane;
    L.melx[i] = mo;
    L.mely[i] = mo + melp;
    mo += 2 * melp;
    L.part[i] = po;
    po += up64((size_t)L.nbx[i] * L.nmy[i] * B * 2 * 2);
    if (plane > L.plane_max) L.plane_max = plane;
    if (melp > L.melp_max) L.melp_max = melp;
    if (g > L.g_max) L.g_max = g;
  }
  L.spectra_total = so;
  L.tail = mo;
  L.mels_total = mo + 64;
  L.part_total = po;
  return true;
}

// Temporaries of one call, in floats (the caller takes them from the stream-ordered allocator).
//   forward:  one transform plane (the target's), the partial sums; without saved state also the prediction's plane,
//             both mel planes and the tail
//   backward: the (re, im) gradient plane, the mel gradient plane and the frame-gradient block
inline size_t forward_tmp_elems(const Layout& L, bool saved) {
  return L.plane_max + L.part_total + (saved ? 0 : L.plane_max + 2 * L.melp_max + 64);
}
inline size_t backward_tmp_elems(const Layout& L) { return L.plane_max + L.melp_max + L.g_max; }

hipError_t launch_ml_forward(const wg_melloss* h, const Layout& L, const float* audio, const float* target,
                             const int* lens, float factor_log, float factor_lin, float* out3, float* spectra,
                             float* mels, float* tmp, int B, int N, hipStream_t s);
hipError_t launch_ml_backward(const wg_melloss* h, const Layout& L, const float* g_out3, const int* lens,
                              float factor_log, float factor_lin, const float* spectra, const float* mels,
                              float* audio_grad_out, float* tmp, int B, int N, hipStream_t s);

}  // namespace wgml
