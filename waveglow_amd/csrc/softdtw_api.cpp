// C ABI of the soft-DTW loss (include/waveglow_amd.h: wg_softdtw_*).  Argument checks run before any device work.
#include <cmath>

#include "wg_host.h"
#include "wg_softdtw.h"

using namespace wg;

namespace {

bool frames_ok(int t) { return t >= 1 && t <= kSdtwMaxFrames; }
bool band_ok(int w) { return w >= 1 && w <= kSdtwMaxBand; }

// The checks the two calls share; 0 when the arguments are accepted.
int check_common(const char* who, int B, int K, int tmax_a, int tmax_b, double gamma, int cost) {
  if (B < 1 || K < 1 || K > kSdtwMaxFeat) return fail(WG_ERR_INVALID, "%s: B >= 1 and 1 <= K <= %d", who, kSdtwMaxFeat);
  if (!frames_ok(tmax_a) || !frames_ok(tmax_b))
    return fail(WG_ERR_INVALID, "%s: tmax %d / %d outside [1, %d]", who, tmax_a, tmax_b, kSdtwMaxFrames);
  if (!(gamma > 0.0) || !std::isfinite(gamma)) return fail(WG_ERR_INVALID, "%s: gamma must be positive and finite", who);
  if (cost != WG_SDTW_L2 && cost != WG_SDTW_SQ) return fail(WG_ERR_INVALID, "%s: unknown cost %d", who, cost);
  return WG_OK;
}

}  // namespace

extern "C" {

size_t wg_softdtw_bytes(int32_t B, int32_t tmax_a, int32_t tmax_b) {
  if (B < 1 || !frames_ok(tmax_a) || !frames_ok(tmax_b)) return 0;
  return sdtw_r_elems(B, tmax_a, tmax_b) * sizeof(double);
}

int wg_softdtw_forward(const float* feat_a, const int32_t* frames_a, const float* feat_b, const int32_t* frames_b,
                       double gamma, int32_t cost, double* value_out, double* r_out, int32_t B, int32_t K,
                       int32_t tmax_a, int32_t tmax_b, void* stream) {
  if (!feat_a || !frames_a || !feat_b || !frames_b || !value_out) return fail(WG_ERR_INVALID, "null argument");
  if (int rc = check_common("softdtw forward", B, K, tmax_a, tmax_b, gamma, cost)) return rc;
  HIP_TRY(launch_sdtw_forward(feat_a, frames_a, feat_b, frames_b, gamma, cost, value_out, r_out, B, K, tmax_a, tmax_b,
                              (hipStream_t)stream));
  return WG_OK;
}

int wg_softdtw_backward(const float* feat_a, const int32_t* frames_a, const float* feat_b, const int32_t* frames_b,
                        double gamma, int32_t cost, const double* r, const double* g_value, double* e_out, float* g_a,
                        float* g_b, int32_t B, int32_t K, int32_t tmax_a, int32_t tmax_b, void* stream) {
  if (!feat_a || !frames_a || !feat_b || !frames_b || !r) return fail(WG_ERR_INVALID, "null argument");
  if ((g_a || g_b) && !g_value) return fail(WG_ERR_INVALID, "null argument: gradients need g_value");
  if (int rc = check_common("softdtw backward", B, K, tmax_a, tmax_b, gamma, cost)) return rc;
  if (!e_out && !g_a && !g_b) return WG_OK;                                  // nothing asked for
  hipStream_t s = (hipStream_t)stream;
  double* e = e_out;
  if (!e) HIP_TRY(hipMallocAsync((void**)&e, (size_t)B * tmax_a * tmax_b * sizeof(double), s));   // stream-ordered, no sync
  hipError_t err = launch_sdtw_backward(feat_a, frames_a, feat_b, frames_b, gamma, cost, r, e, B, K, tmax_a, tmax_b, s);
  if (err == hipSuccess && (g_a || g_b))
    err = launch_sdtw_grads(feat_a, frames_a, feat_b, frames_b, cost, e, g_value, g_a, g_b, B, K, tmax_a, tmax_b, s);
  if (!e_out) {
    const hipError_t ferr = hipFreeAsync(e, s);
    if (err == hipSuccess) err = ferr;
  }
  HIP_TRY(err);
  return WG_OK;
}

size_t wg_softdtw_banded_bytes(int32_t B, int32_t tmax_a, int32_t tmax_b, int32_t band) {
  if (B < 1 || !frames_ok(tmax_a) || !frames_ok(tmax_b) || !band_ok(band)) return 0;
  return sdtw_band_elems(B, tmax_a, tmax_b, band) * sizeof(double);
}

int wg_softdtw_banded_forward(const float* feat_a, const int32_t* frames_a, const float* feat_b, const int32_t* frames_b,
                              double gamma, int32_t cost, double* value_out, double* r_out, int32_t B, int32_t K,
                              int32_t tmax_a, int32_t tmax_b, int32_t band, void* stream) {
  if (!feat_a || !frames_a || !feat_b || !frames_b || !value_out) return fail(WG_ERR_INVALID, "null argument");
  if (int rc = check_common("softdtw banded forward", B, K, tmax_a, tmax_b, gamma, cost)) return rc;
  if (!band_ok(band)) return fail(WG_ERR_INVALID, "softdtw banded forward: band %d outside [1, %d]", band, kSdtwMaxBand);
  HIP_TRY(launch_sdtw_band_forward(feat_a, frames_a, feat_b, frames_b, gamma, cost, value_out, r_out, B, K, tmax_a,
                                   tmax_b, band, (hipStream_t)stream));
  return WG_OK;
}

int wg_softdtw_banded_backward(const float* feat_a, const int32_t* frames_a, const float* feat_b, const int32_t* frames_b,
                               double gamma, int32_t cost, const double* r, const double* g_value, double* e_out,
                               float* g_a, float* g_b, int32_t B, int32_t K, int32_t tmax_a, int32_t tmax_b, int32_t band,
                               void* stream) {
  if (!feat_a || !frames_a || !feat_b || !frames_b || !r) return fail(WG_ERR_INVALID, "null argument");
  if ((g_a || g_b) && !g_value) return fail(WG_ERR_INVALID, "null argument: gradients need g_value");
  if (int rc = check_common("softdtw banded backward", B, K, tmax_a, tmax_b, gamma, cost)) return rc;
  if (!band_ok(band)) return fail(WG_ERR_INVALID, "softdtw banded backward: band %d outside [1, %d]", band, kSdtwMaxBand);
  if (!e_out && !g_a && !g_b) return WG_OK;                                  // nothing asked for
  hipStream_t s = (hipStream_t)stream;
  double* e_band = nullptr;                                                  // the gradients read E in the band layout
  if (g_a || g_b)
    HIP_TRY(hipMallocAsync((void**)&e_band, sdtw_band_elems(B, tmax_a, tmax_b, band) * sizeof(double), s));
  hipError_t err = launch_sdtw_band_backward(feat_a, frames_a, feat_b, frames_b, gamma, cost, r, e_band, e_out, B, K,
                                             tmax_a, tmax_b, band, s);
  if (err == hipSuccess && e_band)
    err = launch_sdtw_band_grads(feat_a, frames_a, feat_b, frames_b, cost, e_band, g_value, g_a, g_b, B, K, tmax_a,
                                 tmax_b, band, s);
  if (e_band) {
    const hipError_t ferr = hipFreeAsync(e_band, s);
    if (err == hipSuccess) err = ferr;
  }
  HIP_TRY(err);
  return WG_OK;
}

}  // extern "C"
