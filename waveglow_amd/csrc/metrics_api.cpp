// C ABI of the validation metrics (include/waveglow_amd.h: wg_metrics_*).  Argument checks run before any device work.
#include "wg_host.h"
#include "wg_metrics.h"

using namespace wg;

namespace {

// Workspace: [basis fp64 n_mfcc x n_mel | mfcc of a | mfcc of b], each part aligned to 256 bytes.
struct MetricsLayout {
  size_t basis, fa, fb, total;   // byte offsets
};

bool frames_ok(int t) { return t >= 1 && t <= kMetricsMaxFrames; }
bool mfcc_ok(int n_mel, int n_mfcc) { return n_mfcc >= 1 && n_mfcc < n_mel && n_mel <= kMetricsMaxFeat; }

MetricsLayout metrics_layout(int B, int n_mel, int n_mfcc, int tmax_a, int tmax_b) {
  MetricsLayout L;
  L.basis = 0;
  L.fa = align_up((size_t)n_mfcc * n_mel * sizeof(double));
  L.fb = L.fa + align_up((size_t)B * n_mfcc * tmax_a * sizeof(float));
  L.total = L.fb + align_up((size_t)B * n_mfcc * tmax_b * sizeof(float));
  return L;
}

}  // namespace

extern "C" {

size_t wg_metrics_workspace_bytes(int32_t B, int32_t n_mel, int32_t n_mfcc, int32_t tmax_a, int32_t tmax_b) {
  if (B < 1 || !mfcc_ok(n_mel, n_mfcc) || !frames_ok(tmax_a) || !frames_ok(tmax_b)) return 0;
  return metrics_layout(B, n_mel, n_mfcc, tmax_a, tmax_b).total;
}

int wg_metrics_mfcc(const float* mel, const int32_t* frames, float* mfcc_out, int32_t B, int32_t n_mel, int32_t n_mfcc,
                    int32_t tmax, void* workspace, size_t workspace_bytes, void* stream) {
  if (!mel || !frames || !mfcc_out || !workspace) return fail(WG_ERR_INVALID, "null argument");
  if (B < 1 || !mfcc_ok(n_mel, n_mfcc)) return fail(WG_ERR_INVALID, "mfcc: B >= 1 and 1 <= n_mfcc < n_mel <= 128");
  if (!frames_ok(tmax)) return fail(WG_ERR_INVALID, "mfcc: tmax %d outside [1, %d]", tmax, kMetricsMaxFrames);
  if (workspace_bytes < (size_t)n_mfcc * n_mel * sizeof(double)) return fail(WG_ERR_WORKSPACE, "mfcc workspace too small");
  hipStream_t s = (hipStream_t)stream;
  HIP_TRY(launch_mfcc_basis((double*)workspace, n_mel, n_mfcc, s));
  HIP_TRY(launch_mfcc(mel, frames, (const double*)workspace, mfcc_out, B, n_mel, n_mfcc, tmax, s));
  return WG_OK;
}

int wg_metrics_dtw(const float* feat_a, const int32_t* frames_a, const float* feat_b, const int32_t* frames_b,
                   double* cost_out, int32_t* frames_out, int32_t B, int32_t K, int32_t tmax_a, int32_t tmax_b,
                   void* stream) {
  if (!feat_a || !frames_a || !feat_b || !frames_b || !cost_out || !frames_out) return fail(WG_ERR_INVALID, "null argument");
  if (B < 1 || K < 1 || K > kMetricsMaxFeat) return fail(WG_ERR_INVALID, "dtw: B >= 1 and 1 <= K <= 128");
  if (!frames_ok(tmax_a) || !frames_ok(tmax_b))
    return fail(WG_ERR_INVALID, "dtw: tmax %d / %d outside [1, %d]", tmax_a, tmax_b, kMetricsMaxFrames);
  HIP_TRY(launch_dtw(feat_a, frames_a, feat_b, frames_b, nullptr, cost_out, frames_out, B, K, tmax_a, tmax_b,
                     (hipStream_t)stream));
  return WG_OK;
}

int wg_metrics_mel(const float* mel_a, const int32_t* frames_a, const float* mel_b, const int32_t* frames_b,
                   double* rows_out, int32_t B, int32_t n_mel, int32_t n_mfcc, int32_t tmax_a, int32_t tmax_b,
                   void* workspace, size_t workspace_bytes, void* stream) {
  if (!mel_a || !frames_a || !mel_b || !frames_b || !rows_out || !workspace) return fail(WG_ERR_INVALID, "null argument");
  if (B < 1 || !mfcc_ok(n_mel, n_mfcc)) return fail(WG_ERR_INVALID, "metrics: B >= 1 and 1 <= n_mfcc < n_mel <= 128");
  if (!frames_ok(tmax_a) || !frames_ok(tmax_b))
    return fail(WG_ERR_INVALID, "metrics: tmax %d / %d outside [1, %d]", tmax_a, tmax_b, kMetricsMaxFrames);
  const MetricsLayout L = metrics_layout(B, n_mel, n_mfcc, tmax_a, tmax_b);
  if (workspace_bytes < L.total) return fail(WG_ERR_WORKSPACE, "metrics workspace too small");
  hipStream_t s = (hipStream_t)stream;
  char* ws = (char*)workspace;
  const double* basis = (const double*)(ws + L.basis);
  float *fa = (float*)(ws + L.fa), *fb = (float*)(ws + L.fb);
  HIP_TRY(launch_mfcc_basis((double*)(ws + L.basis), n_mel, n_mfcc, s));
  HIP_TRY(launch_mfcc(mel_a, frames_a, basis, fa, B, n_mel, n_mfcc, tmax_a, s));
  HIP_TRY(launch_mfcc(mel_b, frames_b, basis, fb, B, n_mel, n_mfcc, tmax_b, s));
  HIP_TRY(launch_dtw(fa, frames_a, fb, frames_b, rows_out, nullptr, nullptr, B, n_mfcc, tmax_a, tmax_b, s));
  HIP_TRY(launch_padded(mel_a, fa, frames_a, mel_b, fb, frames_b, rows_out, B, n_mel, n_mfcc, tmax_a, tmax_b, s));
  return WG_OK;
}

}  // extern "C"
