// Host-side internals shared by api.cpp, train_api.cpp, stft_api.cpp and the host part of stft_loss.hip: the handle, error
// reporting, and the small helpers every C-ABI file needs.  Not installed; the public interface is include/waveglow_amd.h.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdio>
#include <cstdlib>
#include <map>
#include <string>
#include <vector>

#include "../../include/waveglow_amd.h"
#include "wg_common.h"

namespace wg {

// Sets the calling thread's message (wg_last_error) and returns `code`.  Defined in api.cpp.
int fail(int code, const char* fmt, ...) __attribute__((format(printf, 2, 3)));

// The message is only built when the call fails: nothing is formatted or allocated on the per-launch path.
#define HIP_TRY(expr)                                                                          \
  do {                                                                                         \
    hipError_t _e = (expr);                                                                    \
    if (_e != hipSuccess) return wg::fail(WG_ERR_HIP, "%s: %s", #expr, hipGetErrorString(_e)); \
  } while (0)

// WG_DEBUG_SYNC=1: synchronise after every launch and name it on stderr (fault localisation only)
inline bool dbg_sync() {
  static int v = -1;
  if (v < 0) { const char* e = getenv("WG_DEBUG_SYNC"); v = e && *e == '1'; }
  return v == 1;
}

// The library works on a handle's device without changing the caller's current device for good: fill `prev` with
// hipGetDevice before the hipSetDevice; every exit path restores it.
struct DeviceGuard {
  int prev = -1;
  ~DeviceGuard() { if (prev >= 0) (void)hipSetDevice(prev); }
};

inline size_t align_up(size_t x, size_t a = 256) { return (x + a - 1) / a * a; }

inline bool is_early(const wg_config& c, int k) { return k % c.n_early_every == 0 && k > 0; }
inline int n_early_flows(const wg_config& c) {
  int n = 0;
  for (int k = 0; k < c.n_flows; ++k) n += is_early(c, k);
  return n;
}

inline RowGeom make_geom(const wg_config& c, int B, int L, int T) {
  RowGeom g;
  g.frames = nullptr;
  g.B = B;
  g.L = L;
  g.F = (L + kPhases - 1) / kPhases;
  // guard frames: a dilated tap reaches (phase + dilation) >> 5 frames past an utterance's ends; dilation <= 2^(n_layers-1)
  // (model.py:97): 4 frames up to 8 layers, 8 / 16 for 9 / 10 layers
  const int max_dil = 1 << (c.n_layers - 1);
  g.Gf = (kPhases - 1 + max_dil) / kPhases;
  if (g.Gf < 4) g.Gf = 4;
  g.Fp = g.Gf + g.F + g.Gf;
  g.Rp = (B * g.Fp + 127) / 128 * 128;
  g.R = kPhases * g.Rp + 2 * kRowPad;
  g.T = T;
  return g;
}

// The accepted size range of wg_infer / wg_forward (DESIGN.md sections 2 and 8).  A 64-channel chunk
// plane holds R * 128 bytes, and the first layer of every WN keeps a byte offset into the a0 plane in an unsigned 32-bit
// register (wn_layer_kernel A0G), so R * 128 < 2^32: with R = 32 Rp + 32 and Rp a multiple of 128 that is
// Rp <= 2^20 - 128, i.e. B * Fp <= 1 048 448 rows per phase block.  Every other 32-bit quantity of the two directions
// (B * L * 8 state elements, B * L rows of flow_kernel, mel rows, tile counts) stays far below its type's range inside
// this limit, so this is the only size check.  Evaluated in 64 bits, before make_geom's int arithmetic.
constexpr int64_t kMaxRowsPerPhase = (1ll << 20) - 128;
inline int64_t rows_per_phase(const wg_config& c, int64_t B, int64_t L) {
  const int64_t max_dil = 1ll << (c.n_layers - 1);
  int64_t Gf = (kPhases - 1 + max_dil) / kPhases;
  if (Gf < 4) Gf = 4;
  return B * ((L + kPhases - 1) / kPhases + 2 * Gf);
}

struct HostTensor {
  std::vector<int64_t> shape;
  std::vector<float> data;
};

// byte offsets into wg_handle::d_blob
struct LayerOffsets {
  size_t wA1, bias1, wA2, bias2, wEs;
  size_t wA1f = 0;   // layer 0 only: in_layers[0] o start folded onto the a0 plane, one gathered K-step ([tap][8] along K)
  size_t wA1x = 0, wA1fx = 0;   // the same two as 16x16x32 fragments (wn_frag16: the 128-column tile's K loop)
};
struct FlowOffsets {
  std::vector<LayerOffsets> layers;
  size_t wstart, bstart, out_init, winv, wfwd;
  size_t wStA = 0;   // start weights as the A fragment of the first layer's residual step (wn_res_a0)
  int c, h;
  double logdet;   // log|det W_k|, NaN when det < 0 (torch.logdet semantics, model.py:63)
};

}  // namespace wg

struct wg_handle {
  wg_config cfg;
  int device;
  int NS;                 // n_mel * n_group
  std::vector<int> c_k;   // remaining channels per flow (model.py:160-176)
  std::vector<std::string> expected;
  std::map<std::string, wg::HostTensor> tensors;
  bool finalized = false;
  char* d_blob = nullptr;
  size_t blob_bytes = 0;
  char* d_cond = nullptr;   // derived: folded cond_layer o upsample A fragments [flow][layer][phase]...
  char* d_cond16 = nullptr; // ... as 16x16x32 fragments (wn_frag16), same sizes
  size_t cond_layer_bytes = 0, cond_flow_bytes = 0;
  std::vector<wg::FlowOffsets> flows;
  int n_cu = 256;         // multiProcessorCount of `device` (wg_create, wg_finalize)
  int force_bn = 0;       // WG_FORCE_BN=64|128 (tests): pin the WN tile width instead of choosing by workload size
  bool fold_start = true; // WG_NO_START_FOLD=1 (tests / A-B runs): first WN layer reads x_0 like every other layer
  unsigned long long* dbg_stamps = nullptr;   // diagnostic builds only
  // profiling
  bool prof = false;
  unsigned prof_mask = ~0u;
  std::vector<hipEvent_t> ev;
  std::vector<int> ev_class;
  size_t ev_used = 0;
  double prof_ms[8] = {0, 0, 0, 0, 0, 0, 0, 0};
  int64_t prof_n[8] = {0, 0, 0, 0, 0, 0, 0, 0};
  // library-owned streams of the training direction (independent chains of one call run side by side, joined back into
  // the caller's stream before the call returns) and a ring of ordering events for them
  hipStream_t aux[3] = {nullptr, nullptr, nullptr};
  std::vector<hipEvent_t> sync_ev;
  size_t sync_next = 0;
  // events of wg_train_backward's long-lived marks (recorded on one stream, waited on one or two flows later): a pool of
  // their own, one event per role, so that no number of ring events consumed in between can re-record one under a wait
  hipEvent_t mark_ev[16] = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr,
                            nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};
  // pinned staging buffers for small host -> device table uploads (wg_train_prepare / wg_train_param_grads): a rotating set,
  // each guarded by an event recorded behind its copy, so a buffer is never rewritten while a copy out of it is pending
  static constexpr int kPins = 4;
  void* pin[kPins] = {nullptr, nullptr, nullptr, nullptr};
  size_t pin_bytes[kPins] = {0, 0, 0, 0};
  hipEvent_t pin_ev[kPins] = {nullptr, nullptr, nullptr, nullptr};
  int pin_next = 0;
};

// ---- services of the handle with logic of their own (bodies and full comments in api.cpp)
void wg_internal_prof_event(wg_handle* h, void* stream, int cls);   // one profiling event of class cls (begin/end pairs)
hipStream_t wg_internal_aux_stream(wg_handle* h, int i);            // library-owned stream i of the handle's device
hipEvent_t wg_internal_sync_event(wg_handle* h);                    // next event of the ordering ring
hipEvent_t wg_internal_mark_event(wg_handle* h, int slot);          // event `slot` of the mark pool
hipError_t wg_internal_upload(wg_handle* h, void* dst, const void* src, size_t bytes, hipStream_t s);   // pinned H2D copy

namespace wg {
// data.hip: the one launch of wg_data_gather (arguments as in include/waveglow_amd.h, checked by data_api.cpp)
hipError_t launch_data_gather(const void* pool, bool is_i16, int64_t pool_elems, const int64_t* offsets, int n_utt,
                              const int* picks, float* out, int* status, int B, int N, hipStream_t s);
}  // namespace wg

// W_k^-1 of the finalised handle on the device (fp32 of the fp64 inverse, the matrix wg_infer uses), null before wg_finalize
inline const float* wg_internal_winv(const wg_handle* h, int k) {
  if (!h || !h->finalized || k < 0 || k >= (int)h->flows.size()) return nullptr;
  return (const float*)(h->d_blob + h->flows[k].winv);
}
