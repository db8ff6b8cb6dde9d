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

}  // extern "C"
