// C ABI of the per-utterance likelihood (include/waveglow_amd.h: wg_nll*).  Argument checks run before any device work;
// no entry reads a count on the host.  The handle gives the flow layout (h_k rows of log_s[k]) and the fp64 log|det W_k| per
// column that wg_forward multiplies by B * L (src/waveglow/model.py:63); the definition is WaveGlowLoss
// (src/waveglow/train.py:31-45) of one utterance alone.
#include <cmath>

#include "wg_host.h"
#include "wg_likelihood.h"

using namespace wg;

namespace {

bool geometry_ok(int B, int L) { return B >= 1 && B <= 65535 && L >= 1 && L <= (1 << 26); }
size_t part_bytes(int B, int L) { return align_up((size_t)B * ((L + kNllFrameCols - 1) / kNllFrameCols) * kNllPart * sizeof(double)); }

}  // namespace

extern "C" {

size_t wg_nll_workspace_bytes(const wg_handle* h, int32_t B, int32_t L) {
  if (!h || !geometry_ok(B, L)) {
    fail(WG_ERR_INVALID, "nll: a handle, 1 <= B <= 65535 and 1 <= L <= 2^26 expected");
    return 0;
  }
  return part_bytes(B, L);
}

int wg_nll(const wg_handle* h, const float* z, const float* const* log_s, const int32_t* frames, double sigma, int32_t B,
           int32_t L, double* rows_out, double* frame_out, void* workspace, size_t workspace_bytes, void* stream) {
  if (!h) return fail(WG_ERR_INVALID, "null handle");
  if (!z || !log_s || !rows_out || !workspace) return fail(WG_ERR_INVALID, "null argument");
  if (!(sigma > 0.0) || !std::isfinite(sigma)) return fail(WG_ERR_INVALID, "nll: sigma > 0 expected");
  if (!geometry_ok(B, L)) return fail(WG_ERR_INVALID, "nll: 1 <= B <= 65535 and 1 <= L <= 2^26 expected, got %d, %d", B, L);
  if (frames && L % kNllFrameCols != 0)
    return fail(WG_ERR_INVALID, "nll: with frame counts L is 32 columns per frame, got L = %d", L);
  if (!h->finalized) return fail(WG_ERR_STATE, "wg_finalize has not been called");
  const int n_flows = h->cfg.n_flows;
  for (int k = 0; k < n_flows; ++k)
    if (!log_s[k]) return fail(WG_ERR_INVALID, "null log_s[%d]", k);
  if (workspace_bytes < part_bytes(B, L)) return fail(WG_ERR_WORKSPACE, "nll workspace too small");
  double logdet_sum = 0.0;                                             // train.py:37,41: flow order
  for (int k = 0; k < n_flows; ++k) logdet_sum += h->flows[k].logdet;
  const double inv_2s2 = 1.0 / (2.0 * sigma * sigma);                  // train.py:43
  const double half_log_2pis2 = 0.5 * std::log(2.0 * 3.14159265358979323846 * sigma * sigma);
  hipStream_t s = (hipStream_t)stream;
  double* part = (double*)workspace;
  const int n_frames_max = L / kNllFrameCols;
  for (int k0 = 0; k0 < n_flows; k0 += kNllMaxPlanes) {
    NllPlanes pl;
    pl.n = n_flows - k0 < kNllMaxPlanes ? n_flows - k0 : kNllMaxPlanes;
    for (int i = 0; i < kNllMaxPlanes; ++i) {
      pl.p[i] = i < pl.n ? log_s[k0 + i] : nullptr;
      pl.h[i] = i < pl.n ? h->flows[k0 + i].h : 0;
    }
    HIP_TRY(launch_nll_frames(k0 == 0 ? z : nullptr, pl, (const int*)frames, B, L, n_frames_max, inv_2s2, logdet_sum,
                              k0 + kNllMaxPlanes >= n_flows, part, frame_out, s));
  }
  HIP_TRY(launch_nll_rows(part, (const int*)frames, B, L, n_frames_max, inv_2s2, half_log_2pis2, logdet_sum, rows_out, s));
  return WG_OK;
}

}  // extern "C"
