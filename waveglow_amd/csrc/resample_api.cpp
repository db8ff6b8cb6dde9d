// C ABI of the device resampler (include/waveglow_amd.h: wg_resample_*).  Argument checks run before any device work; no
// entry reads a length or a tap on the host.
#include <climits>

#include "wg_host.h"
#include "wg_resample.h"

using namespace wg;

namespace {

int gcd(int a, int b) {
  while (b) { const int t = a % b; a = b; b = t; }
  return a;
}

// null when the ratio, the filter half-width and the row pitch are inside the limits, the complaint otherwise
const char* geom_error(int up, int down, int half, int n_in) {
  if (up < 1 || down < 1) return "resample: up >= 1 and down >= 1 expected";
  if (up > kResampleMaxRate || down > kResampleMaxRate) return "resample: max(up, down) <= 1024 expected";
  if (gcd(up, down) != 1) return "resample: up / down must be reduced (gcd 1)";
  if (half < 0 || half > 10 * kResampleMaxRate) return "resample: half outside [0, 10240]";
  if (n_in < 1 || n_in > kResampleMaxIn) return "resample: n_in outside [1, 2^26]";
  if (resample_out_len(n_in, up, down) > INT_MAX) return "resample: out_len(n_in) does not fit 31 bits";
  return nullptr;
}

int row_taps(int up, int half) { return (2 * half + 1 + up - 1) / up; }

}  // namespace

extern "C" {

int wg_resample_plan(int32_t up, int32_t down, int32_t half, int32_t n_in, int32_t* out_len, int32_t* taps_per_phase,
                     int32_t* tile, int32_t* staged) {
  if (const char* e = geom_error(up, down, half, n_in)) return fail(WG_ERR_INVALID, "%s", e);
  if (out_len) *out_len = (int32_t)resample_out_len(n_in, up, down);
  if (taps_per_phase) *taps_per_phase = row_taps(up, half);
  if (tile) *tile = kResampleTile;
  if (staged) *staged = (up == 1 && down == 1) ? 0 : resample_staged(up, down, row_taps(up, half));
  return WG_OK;
}

int wg_resample(const void* in, int32_t in_dtype, const int32_t* lens, float* out, const double* taps, int32_t up,
                int32_t down, int32_t half, int32_t flags, int32_t B, int32_t n_in, int32_t n_out, void* stream) {
  if (!in || !lens || !out || !taps) return fail(WG_ERR_INVALID, "null argument");
  if (in_dtype != WG_PCM_I16 && in_dtype != WG_PCM_F32) return fail(WG_ERR_INVALID, "resample: bad in_dtype");
  if (flags & ~WG_RESAMPLE_CLIP) return fail(WG_ERR_INVALID, "resample: unknown flags %d", flags);
  if (B < 1) return fail(WG_ERR_INVALID, "resample: B >= 1 expected, got %d", B);
  if (const char* e = geom_error(up, down, half, n_in)) return fail(WG_ERR_INVALID, "%s", e);
  if (n_out < resample_out_len(n_in, up, down))
    return fail(WG_ERR_INVALID, "resample: n_out %d below the %lld outputs of %d samples", n_out,
                (long long)resample_out_len(n_in, up, down), n_in);
  if (n_out > INT_MAX - kResampleTile)
    return fail(WG_ERR_INVALID, "resample: n_out %d above 2^31 - 1 - %d", n_out, kResampleTile);
  ResampleGeom g;
  g.up = up, g.down = down, g.half = half, g.K = row_taps(up, half), g.clip = (flags & WG_RESAMPLE_CLIP) != 0;
  HIP_TRY(launch_resample(in, in_dtype == WG_PCM_I16, lens, out, taps, g, B, n_in, n_out, (hipStream_t)stream));
  return WG_OK;
}

int wg_resample_backward(const void* d_out, int32_t d_out_dtype, const int32_t* lens, float* d_in, const double* taps_t,
                         int32_t up, int32_t down, int32_t half, int32_t B, int32_t n_in, int32_t n_out, void* stream) {
  if (!d_out || !lens || !d_in || !taps_t) return fail(WG_ERR_INVALID, "null argument");
  if (d_out_dtype != WG_PCM_F32 && d_out_dtype != WG_PCM_F64)
    return fail(WG_ERR_INVALID, "resample backward: d_out_dtype must be WG_PCM_F32 or WG_PCM_F64");
  if (B < 1) return fail(WG_ERR_INVALID, "resample: B >= 1 expected, got %d", B);
  if (const char* e = geom_error(up, down, half, n_in)) return fail(WG_ERR_INVALID, "%s", e);
  if (n_out < resample_out_len(n_in, up, down))
    return fail(WG_ERR_INVALID, "resample: n_out %d below the %lld outputs of %d samples", n_out,
                (long long)resample_out_len(n_in, up, down), n_in);
  if (n_out > INT_MAX - kResampleTile)
    return fail(WG_ERR_INVALID, "resample: n_out %d above 2^31 - 1 - %d", n_out, kResampleTile);
  ResampleGeom g;
  g.up = up, g.down = down, g.half = half, g.K = row_taps(up, half), g.clip = false;
  HIP_TRY(launch_resample_backward(d_out, d_out_dtype == WG_PCM_F64, lens, d_in, taps_t, g, row_taps(down, half), B, n_in,
                                   n_out, (hipStream_t)stream));
  return WG_OK;
}

}  // extern "C"
