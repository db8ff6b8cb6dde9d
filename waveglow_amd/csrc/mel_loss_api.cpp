// C ABI of the multi-scale mel loss (include/waveglow_amd.h: wg_melloss_*).  Argument checks run before any device work.
#include <cmath>

#include "wg_host.h"
#include "wg_melloss.h"

using namespace wg;
using namespace wgml;

namespace {

// device part of wg_melloss_create: per scale the packed Fourier bases, the dense bank and the span tables of the sparse
// projection
int upload(wg_melloss* h, const float* const* fwd_basis, const float* const* mel_basis) {
  DeviceGuard dev_guard;
  HIP_TRY(hipGetDevice(&dev_guard.prev));
  HIP_TRY(hipSetDevice(h->device));
  for (int i = 0; i < h->n_scales; ++i) {
    Scale& r = h->sc[i];
    if (int rc = upload_bases(r, fwd_basis[i])) return rc;
    const int K = r.n_fft / 2 + 1;
    // spans: a row from its first to its last non-zero bin (an empty row: first = 1, last = 0); a bin from the lowest to
    // the highest row whose span covers it
    const float* w = mel_basis[i];
    std::vector<int> span((size_t)2 * (r.n_mels + K));
    int* cover = span.data() + 2 * r.n_mels;
    for (int k = 0; k < K; ++k) {
      cover[2 * k] = 1;
      cover[2 * k + 1] = 0;
    }
    for (int m = 0; m < r.n_mels; ++m) {
      int first = 1, last = 0;
      for (int k = 0; k < K; ++k)
        if (w[(size_t)m * K + k] != 0.0f) {
          if (first > last) first = k;
          last = k;
        }
      span[2 * m] = first;
      span[2 * m + 1] = last;
      for (int k = first; k <= last; ++k) {
        if (cover[2 * k] > cover[2 * k + 1]) cover[2 * k] = m;
        cover[2 * k + 1] = m;
      }
    }
    HIP_TRY(hipMalloc((void**)&r.d_W, (size_t)r.n_mels * K * 4));
    HIP_TRY(hipMalloc((void**)&r.d_span, span.size() * 4));
    HIP_TRY(hipMemcpy(r.d_W, w, (size_t)r.n_mels * K * 4, hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(r.d_span, span.data(), span.size() * 4, hipMemcpyHostToDevice));
  }
  return WG_OK;
}

// The checks the forward and the backward share, in the order of the STFT loss's ragged entry points: null arguments and
// bad sizes before the refusal of a planning handle.
int check_call(const wg_melloss* h, bool any_null, int32_t B, int32_t N, Layout& L) {
  if (!h || any_null) return fail(WG_ERR_INVALID, "null argument");
  if (!make_layout(h, B, N, L))
    return fail(WG_ERR_INVALID, "mel loss: B outside [1, 65535], or n_samples <= max n_fft / 2");
  if (h->device < 0) return fail(WG_ERR_STATE, "mel loss: planning handle (device_id < 0) cannot compute");
  return WG_OK;
}

}  // namespace

extern "C" {

int wg_melloss_create(int32_t n_scales, const int32_t* n_fft, const int32_t* hop, const int32_t* win,
                      const int32_t* n_mels, const float* const* fwd_basis, const float* const* mel_basis, float clamp,
                      int32_t device_id, wg_melloss** out) {
  if (!n_fft || !hop || !win || !n_mels || !out) return fail(WG_ERR_INVALID, "null argument");
  if (n_scales < 1 || n_scales > kMaxScales) return fail(WG_ERR_INVALID, "mel loss: 1 to 8 scales");
  if (!(clamp > 0.0f) || !std::isfinite(clamp)) return fail(WG_ERR_INVALID, "mel loss: clamp must be positive and finite");
  for (int i = 0; i < n_scales; ++i) {
    if (int rc = check_geom("mel loss: ", n_fft[i], hop[i], win[i])) return rc;
    if (n_mels[i] < 1 || n_mels[i] > n_fft[i] / 2 + 1)
      return fail(WG_ERR_INVALID, "mel loss: n_mels must be in [1, n_fft / 2 + 1]");
  }
  if (device_id >= 0) {
    if (!fwd_basis || !mel_basis) return fail(WG_ERR_INVALID, "null argument");
    for (int i = 0; i < n_scales; ++i)
      if (!fwd_basis[i] || !mel_basis[i]) return fail(WG_ERR_INVALID, "null basis");
  }
  wg_melloss* h = new wg_melloss();
  h->device = device_id;
  h->n_scales = n_scales;
  h->clamp = clamp;
  for (int i = 0; i < n_scales; ++i) {
    set_geom(h->sc[i], n_fft[i], hop[i], win[i]);
    h->sc[i].n_mels = n_mels[i];
  }
  if (device_id >= 0) {   // a planning handle holds geometry and buffer sizes only
    const int rc = upload(h, fwd_basis, mel_basis);
    if (rc != WG_OK) {
      wg_melloss_destroy(h);
      return rc;
    }
  }
  *out = h;
  return WG_OK;
}

int wg_melloss_destroy(wg_melloss* h) {
  if (!h) return WG_OK;
  for (int i = 0; i < h->n_scales; ++i) {
    Scale& r = h->sc[i];
    free_bases(r);
    if (r.d_W) (void)hipFree(r.d_W);
    if (r.d_span) (void)hipFree(r.d_span);
  }
  delete h;
  return WG_OK;
}

size_t wg_melloss_spectra_elems(const wg_melloss* h, int32_t B, int32_t n_samples) {
  Layout L;
  return make_layout(h, B, n_samples, L) ? L.spectra_total : 0;
}

size_t wg_melloss_mels_elems(const wg_melloss* h, int32_t B, int32_t n_samples) {
  Layout L;
  return make_layout(h, B, n_samples, L) ? L.mels_total : 0;
}

int wg_melloss_forward(wg_melloss* h, const float* audio, const float* target, const int32_t* lens, float factor_log,
                       float factor_lin, float* out3, float* spectra, float* mels, int32_t B, int32_t n_samples,
                       void* stream) {
  Layout L;
  if (h && !spectra != !mels) return fail(WG_ERR_INVALID, "mel loss: spectra and mels may be null only together");
  if (int rc = check_call(h, !audio || !target || !out3, B, n_samples, L)) return rc;
  hipStream_t s = (hipStream_t)stream;
  float* tmp = nullptr;
  HIP_TRY(hipMallocAsync((void**)&tmp, forward_tmp_elems(L, spectra != nullptr) * 4, s));   // stream-ordered, no sync
  hipError_t err = launch_ml_forward(h, L, audio, target, lens, factor_log, factor_lin, out3, spectra, mels, tmp, B,
                                     n_samples, s);
  const hipError_t ferr = hipFreeAsync(tmp, s);
  HIP_TRY(err == hipSuccess ? ferr : err);
  return WG_OK;
}

int wg_melloss_backward(wg_melloss* h, const float* g_out3, const int32_t* lens, float factor_log, float factor_lin,
                        const float* spectra, const float* mels, float* audio_grad_out, int32_t B, int32_t n_samples,
                        void* stream) {
  Layout L;
  if (int rc = check_call(h, !g_out3 || !spectra || !mels || !audio_grad_out, B, n_samples, L)) return rc;
  hipStream_t s = (hipStream_t)stream;
  float* tmp = nullptr;
  HIP_TRY(hipMallocAsync((void**)&tmp, backward_tmp_elems(L) * 4, s));
  hipError_t err = launch_ml_backward(h, L, g_out3, lens, factor_log, factor_lin, spectra, mels, audio_grad_out, tmp, B,
                                      n_samples, s);
  const hipError_t ferr = hipFreeAsync(tmp, s);
  HIP_TRY(err == hipSuccess ? ferr : err);
  return WG_OK;
}

}  // extern "C"
