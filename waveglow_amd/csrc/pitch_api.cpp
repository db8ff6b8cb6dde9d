// C ABI of the pitch metrics (include/waveglow_amd.h: wg_pitch_*).  Argument checks run before any device work; no
// entry reads a length on the host.
#include "wg_host.h"
#include "wg_pitch.h"

using namespace wg;

namespace {

// Workspace of the fused call: [f0 a | aperiodicity a | f0 b | aperiodicity b | frames a | frames b], each part aligned
// to 256 bytes.
struct PitchLayout {
  size_t f0_a, ap_a, f0_b, ap_b, fr_a, fr_b, total;   // byte offsets
  int fmax_a, fmax_b;
};

// null when the parameters are inside the limits, the complaint otherwise
const char* params_error(const wg_pitch_params* p) {
  if (!p) return "null parameters";
  if (!(p->sampling_rate > 0.0) || !(p->sampling_rate < 1e9)) return "pitch: sampling_rate outside (0, 1e9)";
  if (p->frame_length < kPitchMinFrame || p->frame_length > kPitchMaxFrame) return "pitch: frame_length outside [16, 2048]";
  if (p->hop_length < 1) return "pitch: hop_length < 1";
  if (p->tau_min < 2 || p->tau_min >= p->tau_max || p->tau_max > kPitchMaxTau)
    return "pitch: 2 <= tau_min < tau_max <= 1024 expected";
  if (!(p->threshold > 0.0) || !(p->threshold < 1.0)) return "pitch: threshold outside (0, 1)";
  return nullptr;
}

PitchGeom geom(const wg_pitch_params* p) {
  PitchGeom g;
  g.sr = p->sampling_rate, g.threshold = p->threshold;
  g.W = p->frame_length, g.H = p->hop_length, g.tau_min = p->tau_min, g.tau_max = p->tau_max;
  return g;
}

bool batch_ok(int B) { return B >= 1 && B <= 65535; }

int track_frames(const wg_pitch_params* p, int n) {                  // columns of a track of n-sample rows, at least 1
  const int f = pitch_frames(n, p->frame_length, p->hop_length, p->tau_max);
  return f < 1 ? 1 : f;
}

PitchLayout pitch_layout(const wg_pitch_params* p, int B, int n_a, int n_b) {
  PitchLayout L;
  L.fmax_a = track_frames(p, n_a), L.fmax_b = track_frames(p, n_b);
  const size_t ta = align_up((size_t)B * L.fmax_a * sizeof(double)), tb = align_up((size_t)B * L.fmax_b * sizeof(double));
  L.f0_a = 0;
  L.ap_a = L.f0_a + ta;
  L.f0_b = L.ap_a + ta;
  L.ap_b = L.f0_b + tb;
  L.fr_a = L.ap_b + tb;
  L.fr_b = L.fr_a + align_up((size_t)B * sizeof(int32_t));
  L.total = L.fr_b + align_up((size_t)B * sizeof(int32_t));
  return L;
}

}  // namespace

extern "C" {

int32_t wg_pitch_frames(const wg_pitch_params* params, int32_t n_samples) {
  if (const char* e = params_error(params)) return fail(WG_ERR_INVALID, "%s", e);
  if (n_samples < 0) return fail(WG_ERR_INVALID, "pitch: n_samples %d < 0", n_samples);
  return pitch_frames(n_samples, params->frame_length, params->hop_length, params->tau_max);
}

size_t wg_pitch_workspace_bytes(const wg_pitch_params* params, int32_t B, int32_t n_a, int32_t n_b) {
  if (params_error(params) || !batch_ok(B) || n_a < 1 || n_b < 1) return 0;
  return pitch_layout(params, B, n_a, n_b).total;
}

int wg_pitch_yin(const float* audio, const int32_t* lens, const wg_pitch_params* params, double* f0_out,
                 double* aperiodicity_out, int32_t* frames_out, int32_t B, int32_t N, int32_t fmax, void* stream) {
  if (!audio || !lens || !f0_out || !aperiodicity_out || !frames_out) return fail(WG_ERR_INVALID, "null argument");
  if (const char* e = params_error(params)) return fail(WG_ERR_INVALID, "%s", e);
  if (!batch_ok(B) || N < 1) return fail(WG_ERR_INVALID, "pitch: 1 <= B <= 65535 and N >= 1 expected, got %d, %d", B, N);
  if (fmax < track_frames(params, N))
    return fail(WG_ERR_INVALID, "pitch: fmax %d below the %d frames of %d samples", fmax, track_frames(params, N), N);
  HIP_TRY(launch_yin(audio, lens, f0_out, aperiodicity_out, frames_out, geom(params), B, N, fmax, (hipStream_t)stream));
  return WG_OK;
}

int wg_pitch_compare(const double* f0_a, const int32_t* frames_a, const double* f0_b, const int32_t* frames_b,
                     double* rows_out, int32_t B, int32_t fmax_a, int32_t fmax_b, void* stream) {
  if (!f0_a || !frames_a || !f0_b || !frames_b || !rows_out) return fail(WG_ERR_INVALID, "null argument");
  if (!batch_ok(B) || fmax_a < 1 || fmax_b < 1)
    return fail(WG_ERR_INVALID, "pitch: 1 <= B <= 65535 and fmax >= 1 expected, got %d, %d, %d", B, fmax_a, fmax_b);
  HIP_TRY(launch_pitch_compare(f0_a, frames_a, f0_b, frames_b, rows_out, B, fmax_a, fmax_b, (hipStream_t)stream));
  return WG_OK;
}

int wg_pitch_metrics(const float* audio_a, const int32_t* lens_a, int32_t n_a, const float* audio_b, const int32_t* lens_b,
                     int32_t n_b, const wg_pitch_params* params, double* rows_out, int32_t B, void* workspace,
                     size_t workspace_bytes, void* stream) {
  if (!audio_a || !lens_a || !audio_b || !lens_b || !rows_out || !workspace) return fail(WG_ERR_INVALID, "null argument");
  if (const char* e = params_error(params)) return fail(WG_ERR_INVALID, "%s", e);
  if (!batch_ok(B) || n_a < 1 || n_b < 1)
    return fail(WG_ERR_INVALID, "pitch: 1 <= B <= 65535 and N >= 1 expected, got %d, %d, %d", B, n_a, n_b);
  const PitchLayout L = pitch_layout(params, B, n_a, n_b);
  if (workspace_bytes < L.total) return fail(WG_ERR_WORKSPACE, "pitch workspace too small");
  hipStream_t s = (hipStream_t)stream;
  char* ws = (char*)workspace;
  double *f0_a = (double*)(ws + L.f0_a), *f0_b = (double*)(ws + L.f0_b);
  int *fr_a = (int*)(ws + L.fr_a), *fr_b = (int*)(ws + L.fr_b);
  const PitchGeom g = geom(params);
  HIP_TRY(launch_yin(audio_a, lens_a, f0_a, (double*)(ws + L.ap_a), fr_a, g, B, n_a, L.fmax_a, s));
  HIP_TRY(launch_yin(audio_b, lens_b, f0_b, (double*)(ws + L.ap_b), fr_b, g, B, n_b, L.fmax_b, s));
  HIP_TRY(launch_pitch_compare(f0_a, fr_a, f0_b, fr_b, rows_out, B, L.fmax_a, L.fmax_b, s));
  return WG_OK;
}

}  // extern "C"
