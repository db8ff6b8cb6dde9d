// C ABI of the intelligibility metrics (include/waveglow_amd.h: wg_stoi*).  Argument checks run before any device work; no
// entry reads a length or a table on the host.
#include "wg_host.h"
#include "wg_stoi.h"

using namespace wg;

namespace {

// Workspace: [energies | kept-frame lists | counts | band spectra | segment sums], each part aligned to 256 bytes.
struct StoiLayout {
  size_t energy, kept, counts, bands, seg, total;   // byte offsets
};

bool geometry_ok(int B, int pitch) { return B >= 1 && B <= 65535 && pitch >= 1 && pitch <= kStoiMaxPitch; }

StoiLayout stoi_layout(const StoiGeom& g) {
  StoiLayout L;
  const size_t B = (size_t)g.B;
  L.energy = 0;
  L.kept = L.energy + align_up(B * g.F0max * sizeof(double));
  L.counts = L.kept + align_up(B * g.F0max * sizeof(int32_t));
  L.bands = L.counts + align_up(B * 4 * sizeof(int32_t));
  L.seg = L.bands + align_up(B * 2 * kStoiBands * g.Fmax * sizeof(double));
  L.total = L.seg + align_up(B * g.Jmax * 2 * sizeof(double));
  return L;
}

// What wg_stoi_forward keeps for wg_stoi_backward: [counts | kept-frame lists | band spectra].
struct StoiSavedLayout {
  size_t counts, kept, bands, total;
};

StoiSavedLayout stoi_saved_layout(const StoiGeom& g) {
  StoiSavedLayout L;
  const size_t B = (size_t)g.B;
  L.counts = 0;
  L.kept = L.counts + align_up(B * 4 * sizeof(int32_t));
  L.bands = L.kept + align_up(B * g.F0max * sizeof(int32_t));
  L.total = L.bands + align_up(B * 2 * kStoiBands * g.Fmax * sizeof(double));
  return L;
}

// Scratch of wg_stoi_backward: [inverse kept list | segment blocks | band gradients | frame gradients].
struct StoiGradLayout {
  size_t inv, blocks, dband, dframe, total;
};

StoiGradLayout stoi_grad_layout(const StoiGeom& g) {
  StoiGradLayout L;
  const size_t B = (size_t)g.B;
  L.inv = 0;
  L.blocks = L.inv + align_up(B * g.F0max * sizeof(int32_t));
  L.dband = L.blocks + align_up(B * g.Jmax * kStoiBands * kStoiSeg * sizeof(double));
  L.dframe = L.dband + align_up(B * kStoiBands * g.Fmax * sizeof(double));
  L.total = L.dframe + align_up(B * g.Fmax * kStoiW * sizeof(double));
  return L;
}

const char* params_error(const wg_stoi_params* params) {
  if (!params) return "null parameters";
  if (!params->window || !params->bands || !params->cossin) return "stoi: null table in the parameters";
  if ((uintptr_t)params->cossin % 16 != 0) return "stoi: the cos/sin table must be aligned to 16 bytes";
  return nullptr;
}

StoiBuffers saved_parts(void* saved, const StoiSavedLayout& S) {
  char* sv = (char*)saved;
  StoiBuffers w;
  w.energy = nullptr, w.seg = nullptr;
  w.counts = (int*)(sv + S.counts);
  w.kept = (int*)(sv + S.kept);
  w.bands = (double*)(sv + S.bands);
  return w;
}

}  // namespace

extern "C" {

size_t wg_stoi_workspace_bytes(int32_t B, int32_t n_max) {
  if (!geometry_ok(B, n_max)) return 0;
  return stoi_layout(stoi_geom(B, n_max)).total;
}

int wg_stoi(const float* x, const int32_t* len_x, const float* y, const int32_t* len_y, int32_t B, int32_t pitch,
            const wg_stoi_params* params, double* rows_out, void* workspace, size_t workspace_bytes, void* stream) {
  if (!x || !len_x || !y || !len_y || !rows_out || !workspace) return fail(WG_ERR_INVALID, "null argument");
  if (!params) return fail(WG_ERR_INVALID, "null parameters");
  if (!params->window || !params->bands || !params->cossin) return fail(WG_ERR_INVALID, "stoi: null table in the parameters");
  if ((uintptr_t)params->cossin % 16 != 0) return fail(WG_ERR_INVALID, "stoi: the cos/sin table must be aligned to 16 bytes");
  if (!geometry_ok(B, pitch))
    return fail(WG_ERR_INVALID, "stoi: 1 <= B <= 65535 and 1 <= pitch <= %d expected, got %d, %d", kStoiMaxPitch, B, pitch);
  const StoiGeom g = stoi_geom(B, pitch);
  const StoiLayout L = stoi_layout(g);
  if (workspace_bytes < L.total) return fail(WG_ERR_WORKSPACE, "stoi workspace too small");
  char* ws = (char*)workspace;
  StoiBuffers w;
  w.energy = (double*)(ws + L.energy);
  w.kept = (int*)(ws + L.kept);
  w.counts = (int*)(ws + L.counts);
  w.bands = (double*)(ws + L.bands);
  w.seg = (double*)(ws + L.seg);
  HIP_TRY(launch_stoi(x, len_x, y, len_y, params->window, params->bands, params->cossin, rows_out, g, w,
                      (hipStream_t)stream));
  return WG_OK;
}

size_t wg_stoi_saved_bytes(int32_t B, int32_t pitch) {
  if (!geometry_ok(B, pitch)) return 0;
  return stoi_saved_layout(stoi_geom(B, pitch)).total;
}

size_t wg_stoi_backward_workspace_bytes(int32_t B, int32_t pitch) {
  if (!geometry_ok(B, pitch)) return 0;
  return stoi_grad_layout(stoi_geom(B, pitch)).total;
}

int wg_stoi_forward(const float* x, const int32_t* len_x, const float* y, const int32_t* len_y, int32_t B, int32_t pitch,
                    const wg_stoi_params* params, double* rows_out, void* saved, size_t saved_bytes, void* workspace,
                    size_t workspace_bytes, void* stream) {
  if (!x || !len_x || !y || !len_y || !rows_out || !saved || !workspace) return fail(WG_ERR_INVALID, "null argument");
  if (const char* e = params_error(params)) return fail(WG_ERR_INVALID, "%s", e);
  if ((uintptr_t)saved % 8 != 0) return fail(WG_ERR_INVALID, "stoi: the saved buffer must be aligned to 8 bytes");
  if (!geometry_ok(B, pitch))
    return fail(WG_ERR_INVALID, "stoi: 1 <= B <= 65535 and 1 <= pitch <= %d expected, got %d, %d", kStoiMaxPitch, B, pitch);
  const StoiGeom g = stoi_geom(B, pitch);
  const StoiLayout L = stoi_layout(g);
  const StoiSavedLayout S = stoi_saved_layout(g);
  if (saved_bytes < S.total) return fail(WG_ERR_WORKSPACE, "stoi saved buffer too small");
  if (workspace_bytes < L.total) return fail(WG_ERR_WORKSPACE, "stoi workspace too small");
  char* ws = (char*)workspace;
  StoiBuffers w = saved_parts(saved, S);
  w.energy = (double*)(ws + L.energy);
  w.seg = (double*)(ws + L.seg);
  HIP_TRY(launch_stoi(x, len_x, y, len_y, params->window, params->bands, params->cossin, rows_out, g, w,
                      (hipStream_t)stream));
  return WG_OK;
}

int wg_stoi_backward(const float* y, int32_t B, int32_t pitch, const wg_stoi_params* params, const double* g_rows,
                     const void* saved, size_t saved_bytes, double* d_y, void* workspace, size_t workspace_bytes,
                     void* stream) {
  if (!y || !g_rows || !saved || !d_y || !workspace) return fail(WG_ERR_INVALID, "null argument");
  if (const char* e = params_error(params)) return fail(WG_ERR_INVALID, "%s", e);
  if ((uintptr_t)saved % 8 != 0) return fail(WG_ERR_INVALID, "stoi: the saved buffer must be aligned to 8 bytes");
  if (!geometry_ok(B, pitch))
    return fail(WG_ERR_INVALID, "stoi: 1 <= B <= 65535 and 1 <= pitch <= %d expected, got %d, %d", kStoiMaxPitch, B, pitch);
  const StoiGeom g = stoi_geom(B, pitch);
  const StoiSavedLayout S = stoi_saved_layout(g);
  const StoiGradLayout L = stoi_grad_layout(g);
  if (saved_bytes < S.total) return fail(WG_ERR_WORKSPACE, "stoi saved buffer too small");
  if (workspace_bytes < L.total) return fail(WG_ERR_WORKSPACE, "stoi backward workspace too small");
  char* ws = (char*)workspace;
  StoiGradBuffers w;
  w.inv = (int*)(ws + L.inv);
  w.blocks = (double*)(ws + L.blocks);
  w.dband = (double*)(ws + L.dband);
  w.dframe = (double*)(ws + L.dframe);
  HIP_TRY(launch_stoi_backward(y, params->window, params->bands, params->cossin, g_rows,
                               saved_parts(const_cast<void*>(saved), S), d_y, g, w, (hipStream_t)stream));
  return WG_OK;
}

}  // extern "C"
