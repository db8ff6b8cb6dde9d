// Host side of libwaveglow_amd: C ABI (include/waveglow_amd.h), weight packing, launch sequencing.
#include <cmath>
#include <cstdarg>
#include <cstring>

#include "wg_host.h"

using namespace wg;

namespace {
thread_local std::string g_err;
}

int wg::fail(int code, const char* fmt, ...) {
  char buf[512];
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(buf, sizeof buf, fmt, ap);
  va_end(ap);
  g_err = buf;
  return code;
}

namespace {

// fp64 Gauss-Jordan inverse with partial pivoting; also log|det| and sign.
bool invert(const std::vector<double>& A, int n, std::vector<double>& inv, double& logabsdet, int& sign) {
  std::vector<double> M(A);
  inv.assign((size_t)n * n, 0.0);
  for (int i = 0; i < n; ++i) inv[(size_t)i * n + i] = 1.0;
  logabsdet = 0.0;
  sign = 1;
  for (int c = 0; c < n; ++c) {
    int piv = c;
    for (int r = c + 1; r < n; ++r)
      if (std::fabs(M[(size_t)r * n + c]) > std::fabs(M[(size_t)piv * n + c])) piv = r;
    if (M[(size_t)piv * n + c] == 0.0) return false;
    if (piv != c) {
      for (int k = 0; k < n; ++k) {
        std::swap(M[(size_t)piv * n + k], M[(size_t)c * n + k]);
        std::swap(inv[(size_t)piv * n + k], inv[(size_t)c * n + k]);
      }
      sign = -sign;
    }
    const double d = M[(size_t)c * n + c];
    logabsdet += std::log(std::fabs(d));
    if (d < 0) sign = -sign;
    for (int k = 0; k < n; ++k) {
      M[(size_t)c * n + k] /= d;
      inv[(size_t)c * n + k] /= d;
    }
    for (int r = 0; r < n; ++r) {
      if (r == c) continue;
      const double f = M[(size_t)r * n + c];
      if (f == 0.0) continue;
      for (int k = 0; k < n; ++k) {
        M[(size_t)r * n + k] -= f * M[(size_t)c * n + k];
        inv[(size_t)r * n + k] -= f * inv[(size_t)c * n + k];
      }
    }
  }
  return true;
}

// tanh(a) = 1 - 2/(1 + 2^(a*kTanhScale)), sigmoid(b) = 1/(1 + 2^(b*kSigmScale)): folded into GEMM-1 rows
constexpr float kTanhScale = 2.8853900817779268f;    // 2*log2(e)
constexpr float kSigmScale = -1.4426950408889634f;   // -log2(e)

// fp16 hi / lo split of a weight (v ~ hi + lo): the two parts ride as two rows / lane halves of one fp16 MFMA operand.
// hi is v rounded ONCE to fp16 (written as one conversion from double: hipcc merges a double -> float -> fp16 chain into it
// in some contexts and not in others, so spelling the chain would make the packed bits depend on the surrounding code); lo
// is what fp32 has left.
_Float16 f16_split(double v, bool lo_part) {
  const _Float16 hi = (_Float16)v;
  return lo_part ? (_Float16)((float)v - (float)hi) : hi;
}

std::vector<int> flow_channels(const wg_config& c) {
  std::vector<int> out;
  int rem = c.n_group;
  for (int k = 0; k < c.n_flows; ++k) {
    if (is_early(c, k)) rem -= c.n_early_size;
    out.push_back(rem);
  }
  return out;
}

struct Workspace {
  _Float16 *melT, *X0, *X1, *A0;
  float *Z, *OUT;
  size_t bytes;
  size_t x_bytes, mel_bytes, a0_bytes;
};

Workspace carve(const wg_handle* h, const RowGeom& g, char* base) {
  Workspace w;
  size_t off = 0;
  const int C = h->cfg.n_channels;
  w.mel_bytes = align_up((size_t)(3 + g.B * (g.T + 6)) * h->cfg.n_mel_channels * 2);
  w.x_bytes = align_up((size_t)C * g.R * 2);
  w.melT = (_Float16*)(base + off); off += w.mel_bytes;
  w.X0 = (_Float16*)(base + off); off += w.x_bytes;
  w.X1 = (_Float16*)(base + off); off += w.x_bytes;
  w.a0_bytes = align_up((size_t)g.R * 128);
  w.A0 = (_Float16*)(base + off); off += w.a0_bytes;
  w.Z = (float*)(base + off); off += align_up((size_t)g.B * g.L * 8 * 4);
  w.OUT = (float*)(base + off); off += align_up((size_t)g.B * g.L * 8 * 4);
  w.bytes = off;
  return w;
}

// The one size check of the inference and no-grad-forward calls and of their workspace queries (kMaxRowsPerPhase,
// wg_host.h): made before the workspace-size check, so that a caller learns the limit without first allocating a
// workspace of tens of GB for a call that would be refused anyway.
static int check_envelope(const wg_config& c, int B, int L) {
  const int64_t rows = rows_per_phase(c, B, L), F = (L + kPhases - 1) / kPhases, guard = rows / B - F;
  if (rows > kMaxRowsPerPhase)
    return fail(WG_ERR_INVALID,
                "batch too large: %d utterances x (%lld + %lld guard) frames = %lld rows per phase, the limit is B * (T + %lld) <= "
                "%lld (one 64-channel activation plane must stay below 4 GiB)",
                B, (long long)F, (long long)guard, (long long)rows, (long long)guard, (long long)kMaxRowsPerPhase);
  return WG_OK;
}

const HostTensor* find(const wg_handle* h, const std::string& name) {
  auto it = h->tensors.find(name);
  return it == h->tensors.end() ? nullptr : &it->second;
}

// WG_DEBUG_SYNC=1 (dbg_sync): synchronise after every launch and name it on stderr
#define WG_DBG(stream, what) do { if (dbg_sync()) { hipError_t _e = hipStreamSynchronize(stream); fprintf(stderr, "[wg] %s -> %s\n", what, hipGetErrorString(_e)); fflush(stderr); } } while (0)

struct Prof {
  wg_handle* h;
  hipStream_t s;
  int cls;
  Prof(wg_handle* h_, hipStream_t s_, int cls_) : h(h_), s(s_), cls(cls_) {
    if (h->prof) rec();
  }
  ~Prof() {
    if (h->prof) rec();
  }
  void rec() {
    if (h->ev_used == h->ev.size()) {
      hipEvent_t e;
      if (hipEventCreate(&e) != hipSuccess) return;
      h->ev.push_back(e);
      h->ev_class.push_back(0);
    }
    h->ev_class[h->ev_used] = cls;
    hipEventRecord(h->ev[h->ev_used++], s);
  }
};

}  // namespace

namespace wg { extern unsigned long long* g_wgrad_stamps; }   // train.hip

// ---- services of the handle for the other translation units (prototypes in wg_host.h)
// one profiling event of class cls on stream s (a no-op unless wg_profile_enable is on); events come in begin/end pairs
void wg_internal_prof_event(wg_handle* h, void* s, int cls) {
  if (!h || !h->prof || !((h->prof_mask >> cls) & 1u)) return;
  if (h->ev_used == h->ev.size()) {
    hipEvent_t e;
    if (hipEventCreate(&e) != hipSuccess) return;
    h->ev.push_back(e);
    h->ev_class.push_back(0);
  }
  h->ev_class[h->ev_used] = cls;
  hipEventRecord(h->ev[h->ev_used++], (hipStream_t)s);
}

// Library-owned stream i (0: second chain, normal priority; 1, 2: work with slack, lowest priority) of the handle's device.
hipStream_t wg_internal_aux_stream(wg_handle* h, int i) {
  if (!h || i < 0 || i > 2) return nullptr;
  if (!h->aux[i]) {
    int lo = 0, hi = 0, prev = -1;
    hipStream_t st = nullptr;
    if (hipGetDevice(&prev) != hipSuccess) prev = -1;
    if (prev != h->device) (void)hipSetDevice(h->device);
    if (i >= 1 && hipDeviceGetStreamPriorityRange(&lo, &hi) == hipSuccess && lo != hi) {
      if (hipStreamCreateWithPriority(&st, hipStreamNonBlocking, lo) != hipSuccess) st = nullptr;
    }
    if (!st && hipStreamCreateWithFlags(&st, hipStreamNonBlocking) != hipSuccess) st = nullptr;
    if (prev >= 0 && prev != h->device) (void)hipSetDevice(prev);
    h->aux[i] = st;
  }
  return h->aux[i];
}
// Copies `bytes` of host memory to `dst` (device) on stream `s` through a pinned staging buffer of the handle: the caller's
// source may be freed or rewritten as soon as this returns, and the copy itself is asynchronous.
hipError_t wg_internal_upload(wg_handle* h, void* dst, const void* src, size_t bytes, hipStream_t s) {
  if (!h) return hipErrorInvalidValue;
  const int i = h->pin_next;
  h->pin_next = (i + 1) % wg_handle::kPins;
  hipError_t e;
  if (h->pin_ev[i] && (e = hipEventSynchronize(h->pin_ev[i])) != hipSuccess) return e;     // its last copy has run
  if (h->pin_bytes[i] < bytes) {
    if (h->pin[i]) (void)hipHostFree(h->pin[i]);
    h->pin[i] = nullptr;
    h->pin_bytes[i] = 0;
    const size_t cap = bytes < 65536 ? 65536 : bytes;
    if ((e = hipHostMalloc(&h->pin[i], cap, hipHostMallocDefault)) != hipSuccess) return e;
    h->pin_bytes[i] = cap;
  }
  if (!h->pin_ev[i] && (e = hipEventCreateWithFlags(&h->pin_ev[i], hipEventDisableTiming)) != hipSuccess) return e;
  memcpy(h->pin[i], src, bytes);
  if ((e = hipMemcpyAsync(dst, h->pin[i], bytes, hipMemcpyHostToDevice, s)) != hipSuccess) return e;
  return hipEventRecord(h->pin_ev[i], s);
}
// Event `slot` of the mark pool (no timing), created on first use.
hipEvent_t wg_internal_mark_event(wg_handle* h, int slot) {
  if (!h || slot < 0 || slot >= 16) return nullptr;
  if (!h->mark_ev[slot] && hipEventCreateWithFlags(&h->mark_ev[slot], hipEventDisableTiming) != hipSuccess) h->mark_ev[slot] = nullptr;
  return h->mark_ev[slot];
}
// Next event of the ordering ring (no timing).  A wait captures the record that precedes it in host order, so an event
// may be recorded again while earlier waits on it are still pending on the device.  Ring events are for record-then-wait
// pairs issued back to back (order_after); anything waited on LATER uses wg_internal_mark_event.
hipEvent_t wg_internal_sync_event(wg_handle* h) {
  constexpr size_t kRing = 1024;
  if (!h) return nullptr;
  if (h->sync_ev.size() < kRing) {
    hipEvent_t e;
    if (hipEventCreateWithFlags(&e, hipEventDisableTiming) != hipSuccess) return nullptr;
    h->sync_ev.push_back(e);
    return e;
  }
  hipEvent_t e = h->sync_ev[h->sync_next];
  h->sync_next = (h->sync_next + 1) % kRing;
  return e;
}

extern "C" {

const char* wg_version(void) { return "waveglow_amd 0.3 (gfx950)"; }
const char* wg_last_error(void) { return g_err.c_str(); }

int wg_create(const wg_config* cfg, int device_id, wg_handle** out) {
  if (!cfg || !out) return fail(WG_ERR_INVALID, "null argument");
  const wg_config& c = *cfg;
  if (c.n_group != 8) return fail(WG_ERR_INVALID, "n_group=%d unsupported (only 8)", c.n_group);
  if (c.kernel_size != 3) return fail(WG_ERR_INVALID, "kernel_size=%d unsupported (only 3)", c.kernel_size);
  if (c.n_channels != 64 && c.n_channels != 128 && c.n_channels != 256 && c.n_channels != 512)
    return fail(WG_ERR_INVALID, "n_channels=%d unsupported (64, 128, 256, 512)", c.n_channels);
  if (c.n_layers < 1 || c.n_layers > 10) return fail(WG_ERR_INVALID, "n_layers=%d unsupported (1..10)", c.n_layers);
  if (c.upsample_kernel != 1024 || c.upsample_stride != 256)
    return fail(WG_ERR_INVALID, "upsample geometry %d/%d unsupported (1024/256)", c.upsample_kernel, c.upsample_stride);
  if (c.n_mel_channels < 16 || c.n_mel_channels > 80 || c.n_mel_channels % 16 != 0)
    return fail(WG_ERR_INVALID, "n_mel_channels=%d unsupported (multiple of 16, <= 80)", c.n_mel_channels);
  if (c.n_flows < 1 || c.n_early_every < 1 || c.n_early_size < 0 || c.n_early_size % 2 != 0)
    return fail(WG_ERR_INVALID, "bad flow configuration");
  // zero-channel early outputs (the reference runs them as empty tensors) are outside the envelope: an empty tensor has no
  // device pointer to hand over, and the flow-step kernels have never run with n_extra = n_peel = 0 at an early flow
  if (c.n_early_size == 0) return fail(WG_ERR_INVALID, "n_early_size=0 unsupported (even, >= 2)");
  std::vector<int> ck = flow_channels(c);
  if (ck.back() < 2 || ck.back() % 2 != 0) return fail(WG_ERR_INVALID, "flow configuration leaves %d channels", ck.back());
  wg_handle* h = new wg_handle();
  h->cfg = c;
  h->device = device_id;
  {
    int ncu = 0;   // of THIS device, whatever the caller's current device is
    if (hipDeviceGetAttribute(&ncu, hipDeviceAttributeMultiprocessorCount, device_id) == hipSuccess && ncu > 0) h->n_cu = ncu;
  }
  h->NS = c.n_mel_channels * c.n_group;
  h->c_k = ck;
  if (const char* e = getenv("WG_FORCE_BN")) h->force_bn = atoi(e);
  if (const char* e = getenv("WG_NO_START_FOLD")) h->fold_start = !(*e == '1');
  h->expected.push_back("upsample.weight");
  h->expected.push_back("upsample.bias");
  for (int k = 0; k < c.n_flows; ++k) {
    const std::string ks = std::to_string(k);
    h->expected.push_back("convinv." + ks + ".conv.weight");
    const std::string p = "WN." + ks + ".";
    for (const char* n : {"start", "cond_layer", "end"}) {
      h->expected.push_back(p + n + ".weight");
      h->expected.push_back(p + n + ".bias");
    }
    for (int i = 0; i < c.n_layers; ++i) {
      const std::string is = std::to_string(i);
      h->expected.push_back(p + "in_layers." + is + ".weight");
      h->expected.push_back(p + "in_layers." + is + ".bias");
      h->expected.push_back(p + "res_skip_layers." + is + ".weight");
      h->expected.push_back(p + "res_skip_layers." + is + ".bias");
    }
  }
  *out = h;
  return WG_OK;
}

int wg_destroy(wg_handle* h) {
  if (!h) return WG_OK;
  if (h->d_blob) hipFree(h->d_blob);
  if (h->d_cond) hipFree(h->d_cond);
  if (h->d_cond16) hipFree(h->d_cond16);
  for (hipEvent_t e : h->ev) hipEventDestroy(e);
  for (hipEvent_t e : h->sync_ev) hipEventDestroy(e);
  for (hipEvent_t e : h->mark_ev)
    if (e) hipEventDestroy(e);
  for (int i = 0; i < wg_handle::kPins; ++i) {
    if (h->pin_ev[i]) hipEventDestroy(h->pin_ev[i]);
    if (h->pin[i]) (void)hipHostFree(h->pin[i]);
  }
  for (hipStream_t st : h->aux)
    if (st) hipStreamDestroy(st);
  delete h;
  return WG_OK;
}

int wg_num_expected_tensors(const wg_handle* h) { return h ? (int)h->expected.size() : 0; }
const char* wg_expected_tensor_name(const wg_handle* h, int32_t i) {
  if (!h || i < 0 || i >= (int)h->expected.size()) return nullptr;
  return h->expected[i].c_str();
}

int wg_set_tensor(wg_handle* h, const char* name, const float* data, const int64_t* shape, int32_t ndim) {
  if (!h || !name || !data || !shape || ndim < 1 || ndim > 4) return fail(WG_ERR_INVALID, "bad argument to wg_set_tensor");
  bool known = false;
  for (const auto& e : h->expected) known |= (e == name);
  if (!known) return fail(WG_ERR_INVALID, "unexpected tensor name '%s'", name);
  HostTensor t;
  size_t n = 1;
  for (int i = 0; i < ndim; ++i) {
    if (shape[i] <= 0) return fail(WG_ERR_INVALID, "bad shape for '%s'", name);
    t.shape.push_back(shape[i]);
    n *= (size_t)shape[i];
  }
  t.data.assign(data, data + n);
  h->tensors[name] = std::move(t);
  h->finalized = false;
  return WG_OK;
}

static int check_shape(const wg_handle* h, const std::string& name, std::initializer_list<int64_t> want,
                       const HostTensor** out) {
  const HostTensor* t = find(h, name);
  if (!t) return fail(WG_ERR_STATE, "missing tensor '%s'", name.c_str());
  std::vector<int64_t> w(want);
  if (t->shape != w) {
    std::string got, exp;
    for (auto v : t->shape) got += std::to_string(v) + ",";
    for (auto v : w) exp += std::to_string(v) + ",";
    return fail(WG_ERR_INVALID, "tensor '%s' has shape [%s] expected [%s]", name.c_str(), got.c_str(), exp.c_str());
  }
  *out = t;
  return WG_OK;
}

// wg_finalize, first half: checks the tensors and packs every host-packed weight into `blob` (pure host arithmetic; the
// offsets go to h->flows)
static int build_blob(wg_handle* h, std::vector<char>& blob) {
  const wg_config& c = h->cfg;
  const int C = c.n_channels, M = c.n_mel_channels, NS = h->NS, NL = c.n_layers;
  const int NW = wn_waves(C), MB = C / (32 * NW), MT = 2 * MB, CC = C / 64, K2 = C / 16, nKx = 3 * CC;
  auto reserve = [&](size_t bytes) {
    size_t off = align_up(blob.size());
    blob.resize(off + bytes, 0);
    return off;
  };
  int rc;
  // ---- upsample weights: folded into the conditioning GEMM on the device (finalize_device: cond_fold_kernel)
  const HostTensor *upw, *upb;
  if ((rc = check_shape(h, "upsample.weight", {M, M, c.upsample_kernel}, &upw))) return rc;
  if ((rc = check_shape(h, "upsample.bias", {M}, &upb))) return rc;
  // GEMM-1 A fragments of the 32x32x16 MFMA, [half K-step u][NW][MT][2 k16][64 lanes][8]; wave w owns 32-channel blocks
  // w*MB .. w*MB+MB-1: M-tiles mt < MB are their tanh rows, mt >= MB their sigmoid rows (+C).  value(m, ksx, kk) is the
  // unscaled weight of row m at K index kk of K-step ksx (a double is scaled in double and rounded once to fp16, see
  // f16_split); K indices from k_live up carry no weight and stay zero.
  auto pack32 = [&](size_t off, int n_half, int k_live, auto&& value) {
    _Float16* dst = (_Float16*)(blob.data() + off);
    for (int u = 0; u < n_half; ++u)
      for (int w = 0; w < NW; ++w)
        for (int mt = 0; mt < MT; ++mt)
          for (int k2 = 0; k2 < 2; ++k2)
            for (int lane = 0; lane < 64; ++lane) {
              const int ksx = u >> 1, k16 = (u & 1) * 2 + k2;
              const int r = lane & 31, hh = lane >> 5;
              const bool tanh_row = mt < MB;
              const int m = (tanh_row ? 0 : C) + 32 * (w * MB + (tanh_row ? mt : mt - MB)) + r;
              const float rs = tanh_row ? kTanhScale : kSigmScale;   // gate pre-scale (kernels.hip gate_act)
              _Float16* d = dst + (((((size_t)u * NW + w) * MT + mt) * 2 + k2) * 64 + lane) * 8;
              for (int j = 0; j < 8; ++j) {
                const int kk = k16 * 16 + 8 * hh + j;
                if (kk < k_live) d[j] = (_Float16)(value(m, ksx, kk) * rs);
              }
            }
  };
  h->flows.assign(c.n_flows, FlowOffsets());
  for (int k = 0; k < c.n_flows; ++k) {
    FlowOffsets& fo = h->flows[k];
    const int ck = h->c_k[k], hk = ck / 2;
    fo.c = ck;
    fo.h = hk;
    const std::string ks = std::to_string(k), p = "WN." + ks + ".";
    const HostTensor *wci, *wst, *bst, *wcond, *bcond, *wend, *bend;
    if ((rc = check_shape(h, "convinv." + ks + ".conv.weight", {ck, ck, 1}, &wci))) return rc;
    if ((rc = check_shape(h, p + "start.weight", {C, hk, 1}, &wst))) return rc;
    if ((rc = check_shape(h, p + "start.bias", {C}, &bst))) return rc;
    if ((rc = check_shape(h, p + "cond_layer.weight", {2 * C * NL, NS, 1}, &wcond))) return rc;
    if ((rc = check_shape(h, p + "cond_layer.bias", {2 * C * NL}, &bcond))) return rc;
    if ((rc = check_shape(h, p + "end.weight", {2 * hk, C, 1}, &wend))) return rc;
    if ((rc = check_shape(h, p + "end.bias", {2 * hk}, &bend))) return rc;
    // 1x1 invertible conv: forward matrix, fp64 inverse, log|det|
    {
      std::vector<double> A((size_t)ck * ck), inv;
      for (int i = 0; i < ck * ck; ++i) A[i] = wci->data[i];
      double lad;
      int sign;
      if (!invert(A, ck, inv, lad, sign)) return fail(WG_ERR_INVALID, "convinv.%d weight is singular", k);
      fo.logdet = sign > 0 ? lad : std::nan("");
      fo.winv = reserve((size_t)ck * ck * 4);
      fo.wfwd = reserve((size_t)ck * ck * 4);
      float* wi = (float*)(blob.data() + fo.winv);
      float* wf = (float*)(blob.data() + fo.wfwd);
      for (int i = 0; i < ck * ck; ++i) {
        wi[i] = (float)inv[i];
        wf[i] = wci->data[i];
      }
    }
    // start conv, position-major rows
    fo.wstart = reserve((size_t)C * hk * 4);
    fo.bstart = reserve((size_t)C * 4);
    {
      float* ws = (float*)(blob.data() + fo.wstart);
      float* bs = (float*)(blob.data() + fo.bstart);
      for (int P = 0; P < C; ++P) {
        const int ch = pos_to_chan(P);
        for (int j = 0; j < hk; ++j) ws[P * hk + j] = wst->data[(size_t)ch * hk + j];
        bs[P] = bst->data[ch];
      }
    }
    if (wn_res_a0(C)) {
      // A fragment of the 32x32x16 MFMA, [wave][lane = (row r, half)][8]: row r = channel 32 w + r; lanes 0-31 hold the fp16
      // hi parts of (W_start[ch][0..h-1], b_start[ch] at k = 4), lanes 32-63 the lo parts -- against the a0 plane row, which
      // carries (a0 | 1 | 0 0 0) at positions 0-7 and again at 8-15 (flow_kernel)
      fo.wStA = reserve((size_t)(C / 32) * 64 * 8 * 2);
      _Float16* d = (_Float16*)(blob.data() + fo.wStA);
      for (int w = 0; w < C / 32; ++w)
        for (int lane = 0; lane < 64; ++lane) {
          const int ch = 32 * w + (lane & 31);
          for (int j = 0; j < 8; ++j) {
            const float v = j < hk ? wst->data[(size_t)ch * hk + j] : j == 4 ? bst->data[ch] : 0.0f;
            d[((size_t)w * 64 + lane) * 8 + j] = f16_split(v, lane >= 32);
          }
        }
    }
    std::vector<double> out_bias(8, 0.0);
    for (int r = 0; r < 2 * hk; ++r) out_bias[r] = bend->data[r];
    fo.layers.assign(NL, LayerOffsets());
    for (int i = 0; i < NL; ++i) {
      LayerOffsets& lo = fo.layers[i];
      const std::string is = std::to_string(i);
      const bool has_res = i < NL - 1;
      const int RS = has_res ? 2 * C : C;
      const HostTensor *win, *bin, *wrs, *brs;
      if ((rc = check_shape(h, p + "in_layers." + is + ".weight", {2 * C, C, 3}, &win))) return rc;
      if ((rc = check_shape(h, p + "in_layers." + is + ".bias", {2 * C}, &bin))) return rc;
      if ((rc = check_shape(h, p + "res_skip_layers." + is + ".weight", {RS, C, 1}, &wrs))) return rc;
      if ((rc = check_shape(h, p + "res_skip_layers." + is + ".bias", {RS}, &brs))) return rc;
      // the three taps: K-step ksx = (tap, 64-channel chunk), K index kk = position inside the chunk
      auto tap_weight = [&](int m, int ksx, int kk) {
        const int tap = ksx / CC, cc = ksx % CC;
        return win->data[((size_t)m * C + pos_to_chan(cc * 64 + kk)) * 3 + tap];
      };
      lo.wA1 = reserve((size_t)nKx * 2 * NW * MT * 2 * 64 * 8 * 2);
      pack32(lo.wA1, 2 * nKx, 64, tap_weight);
      const bool f16 = wn_frag16(C, wn_block_n(C));
      // 16x16x32 fragments [half K-step u][wave][tile m][64 lanes = (row i = lane & 15, K group lane >> 4)][8]: tile m of
      // wave w = rows 32 w + 16 (m & 1) + i of the tanh (m < 2) / sigmoid half; K = 32 (u & 1) + 8 (lane >> 4) + j of the step
      auto pack16 = [&](size_t off, int n_half, auto&& value) {
        _Float16* dst = (_Float16*)(blob.data() + off);
        for (int u = 0; u < n_half; ++u)
          for (int w = 0; w < NW; ++w)
            for (int m4 = 0; m4 < 4; ++m4)
              for (int lane = 0; lane < 64; ++lane) {
                const int m = (m4 < 2 ? 0 : C) + 32 * w + 16 * (m4 & 1) + (lane & 15);
                const float rs = m4 < 2 ? kTanhScale : kSigmScale;
                _Float16* d = dst + ((((size_t)u * NW + w) * 4 + m4) * 64 + lane) * 8;
                for (int j = 0; j < 8; ++j) d[j] = (_Float16)(value(m, u >> 1, 32 * (u & 1) + 8 * (lane >> 4) + j) * rs);
              }
      };
      if (f16) {
        lo.wA1x = reserve((size_t)nKx * 2 * NW * 4 * 64 * 8 * 2);
        pack16(lo.wA1x, 2 * nKx, tap_weight);
      }
      if (i == 0) {
        // in_layers[0] o start (model.py:117, :123): column kk of tap `tap` on the a0 plane row (a0 | 1 | 0...):
        //   kk < h: sum_ch W_in[m][ch][tap] W_start[ch][kk];  kk == 4: sum_ch W_in[m][ch][tap] b_start[ch]
        std::vector<double> fold((size_t)2 * C * 3 * 8, 0.0);
        for (int m = 0; m < 2 * C; ++m)
          for (int tap = 0; tap < 3; ++tap) {
            double* fr = &fold[((size_t)m * 3 + tap) * 8];
            for (int ch = 0; ch < C; ++ch) {
              const double wv = win->data[((size_t)m * C + ch) * 3 + tap];
              for (int j = 0; j < hk; ++j) fr[j] += wv * wst->data[(size_t)ch * hk + j];
              fr[4] += wv * bst->data[ch];
            }
          }
        // ONE K-step for the three taps (wn_layer_kernel A0G): K index kk = 8 tap + j against a B tile whose 16-byte chunk
        // `tap` is the first chunk (a0 | 1 | 0 0 0) of that tap's a0-plane row
        lo.wA1f = reserve((size_t)2 * NW * MT * 2 * 64 * 8 * 2);
        // Both packings take the fold as ONE float value per weight: the gate scale is then applied and the product rounded to
        // fp16 by the same float arithmetic in pack32 and pack16.  (wA1f used to take the double itself: the scaled value
        // then landed on the neighbouring fp16 number for a few weights per flow, and the 64-column tiles differed in bits
        // from the 128-column ones at 256 channels -- tests/test_gpu_dispatch_identity.py)
        auto fold_weight = [&](int m, int, int kk) { return kk < 24 ? (float)fold[((size_t)m * 3 + (kk >> 3)) * 8 + (kk & 7)] : 0.0f; };
        pack32(lo.wA1f, 2, 24, fold_weight);
        if (f16) {
          lo.wA1fx = reserve((size_t)2 * NW * 4 * 64 * 8 * 2);
          pack16(lo.wA1fx, 2, fold_weight);
        }
      }
      lo.bias1 = reserve((size_t)2 * C * 4);
      {
        float* b1 = (float*)(blob.data() + lo.bias1);
        for (int m = 0; m < 2 * C; ++m) {
          // constant part of the folded conditioning: W_cond . (upsample bias broadcast over the 8 group phases)
          double cb = 0.0;
          const float* wr = &wcond->data[((size_t)(2 * C * i + m)) * NS];
          for (int sch = 0; sch < NS; ++sch) cb += (double)wr[sch] * upb->data[sch >> 3];
          b1[m] = (float)((bin->data[m] + bcond->data[2 * C * i + m] + cb) * (m < C ? kTanhScale : kSigmScale));
        }
      }
      // GEMM2 (res) A fragments [NW][MB][K2][64][8], bias2
      lo.wA2 = reserve((size_t)NW * MB * K2 * 64 * 8 * 2);
      lo.bias2 = reserve((size_t)C * 4);
      if (has_res) {
        _Float16* dst = (_Float16*)(blob.data() + lo.wA2);
        for (int w = 0; w < NW; ++w)
          for (int mb = 0; mb < MB; ++mb)
            for (int k16 = 0; k16 < K2; ++k16)
              for (int lane = 0; lane < 64; ++lane) {
                const int r = lane & 31, hh = lane >> 5;
                const int m = 32 * (w * MB + mb) + r;
                _Float16* d = dst + ((((size_t)w * MB + mb) * K2 + k16) * 64 + lane) * 8;
                for (int j = 0; j < 8; ++j) {
                  const int ch = pos_to_chan(k16 * 16 + 8 * hh + j);
                  d[j] = (_Float16)wrs->data[(size_t)m * C + ch];
                }
              }
        float* b2 = (float*)(blob.data() + lo.bias2);
        for (int m = 0; m < C; ++m) b2[m] = brs->data[m];
      }
      // folded end x skip: Wes = W_end (2h x C) * W_skip_i (C x C), fp64; hi/lo fp16 split
      const int skip_row0 = has_res ? C : 0;
      std::vector<double> Wes((size_t)8 * C, 0.0);
      for (int r = 0; r < 2 * hk; ++r) {
        for (int m = 0; m < C; ++m) {
          const double we = wend->data[(size_t)r * C + m];
          const float* wrow = &wrs->data[(size_t)(skip_row0 + m) * C];
          for (int cch = 0; cch < C; ++cch) Wes[(size_t)r * C + cch] += we * wrow[cch];
          out_bias[r] += we * brs->data[skip_row0 + m];
        }
      }
      lo.wEs = reserve((size_t)(C / 32) * 64 * 8 * 2);
      {
        _Float16* dst = (_Float16*)(blob.data() + lo.wEs);
        for (int s = 0; s < C / 32; ++s)
          for (int lane = 0; lane < 64; ++lane) {
            const int row = lane & 15, l4 = lane >> 4;
            for (int j = 0; j < 8; ++j) {
              const int ch = pos_to_chan(32 * s + 8 * l4 + j);
              dst[((size_t)s * 64 + lane) * 8 + j] = f16_split(Wes[(size_t)(row & 7) * C + ch], row >= 8);
            }
          }
      }
    }
    fo.out_init = reserve(8 * 4);
    {
      float* oi = (float*)(blob.data() + fo.out_init);
      for (int r = 0; r < 8; ++r) oi[r] = (float)out_bias[r];
    }
  }
  return WG_OK;
}

// wg_finalize, second half: the blob goes to the device, and cond_layer o upsample is folded there, flow by flow
static int finalize_device(wg_handle* h, const std::vector<char>& blob) {
  const wg_config& c = h->cfg;
  const int C = c.n_channels, M = c.n_mel_channels, NS = h->NS, NL = c.n_layers;
  const int NW = wn_waves(C), MT = 2 * (C / (32 * NW));
  const HostTensor* upw = find(h, "upsample.weight");
  DeviceGuard dev_guard;
  HIP_TRY(hipGetDevice(&dev_guard.prev));
  HIP_TRY(hipSetDevice(h->device));
  {
    int ncu = 0;
    HIP_TRY(hipDeviceGetAttribute(&ncu, hipDeviceAttributeMultiprocessorCount, h->device));
    if (ncu > 0) h->n_cu = ncu;
  }
  if (h->d_blob) {
    HIP_TRY(hipDeviceSynchronize());
    HIP_TRY(hipFree(h->d_blob));
    h->d_blob = nullptr;
  }
  HIP_TRY(hipMalloc((void**)&h->d_blob, blob.size()));
  HIP_TRY(hipMemcpy(h->d_blob, blob.data(), blob.size(), hipMemcpyHostToDevice));
  h->blob_bytes = blob.size();
  // ---- derived weights: cond_layer o upsample, one matrix per (flow, layer, phase), built on the device
  {
    if (h->d_cond) {
      HIP_TRY(hipFree(h->d_cond));
      h->d_cond = nullptr;
    }
    const int n_half = 2 * (M / 16);
    h->cond_layer_bytes = (size_t)kPhases * n_half * NW * MT * 2 * 64 * 8 * 2;
    h->cond_flow_bytes = h->cond_layer_bytes * NL;
    HIP_TRY(hipMalloc((void**)&h->d_cond, h->cond_flow_bytes * c.n_flows));
    if (h->d_cond16) {
      HIP_TRY(hipFree(h->d_cond16));
      h->d_cond16 = nullptr;
    }
    if (wn_frag16(C, wn_block_n(C))) HIP_TRY(hipMalloc((void**)&h->d_cond16, h->cond_flow_bytes * c.n_flows));
    float *d_wc = nullptr, *d_up = nullptr;
    const size_t wc_bytes = (size_t)2 * C * NL * NS * 4, up_bytes = (size_t)M * M * c.upsample_kernel * 4;
    HIP_TRY(hipMalloc((void**)&d_wc, wc_bytes));
    HIP_TRY(hipMalloc((void**)&d_up, up_bytes));
    HIP_TRY(hipMemcpy(d_up, upw->data.data(), up_bytes, hipMemcpyHostToDevice));
    for (int k = 0; k < c.n_flows; ++k) {
      const HostTensor* wcond = find(h, "WN." + std::to_string(k) + ".cond_layer.weight");
      HIP_TRY(hipMemcpy(d_wc, wcond->data.data(), wc_bytes, hipMemcpyHostToDevice));
      HIP_TRY(launch_cond_fold(d_wc, d_up, (_Float16*)(h->d_cond + h->cond_flow_bytes * k), C, NW, M, NL,
                               c.upsample_kernel, kTanhScale, kSigmScale, 0, nullptr));
      if (h->d_cond16)
        HIP_TRY(launch_cond_fold(d_wc, d_up, (_Float16*)(h->d_cond16 + h->cond_flow_bytes * k), C, NW, M, NL,
                                 c.upsample_kernel, kTanhScale, kSigmScale, 1, nullptr));
      HIP_TRY(hipDeviceSynchronize());
      if (dbg_sync()) { fprintf(stderr, "[wg] cond_fold flow %d ok\n", k); fflush(stderr); }
    }
    HIP_TRY(hipFree(d_wc));
    HIP_TRY(hipFree(d_up));
  }
  h->finalized = true;
  return WG_OK;
}

int wg_finalize(wg_handle* h) {
  if (!h) return fail(WG_ERR_INVALID, "null handle");
  std::vector<char> blob;
  const int rc = build_blob(h, blob);
  return rc != WG_OK ? rc : finalize_device(h, blob);
}

size_t wg_infer_workspace_bytes(const wg_handle* h, int32_t B, int32_t n_frames) {
  if (!h || B < 1 || n_frames < 1) {
    fail(WG_ERR_INVALID, "bad B/n_frames");
    return 0;
  }
  const int L = n_frames * h->cfg.upsample_stride / h->cfg.n_group;
  if (check_envelope(h->cfg, B, L) != WG_OK) return 0;   // the call would refuse it: wg_last_error names the limit
  RowGeom g = make_geom(h->cfg, B, L, n_frames);
  return carve(h, g, nullptr).bytes;
}

size_t wg_forward_workspace_bytes(const wg_handle* h, int32_t B, int32_t n_frames, int32_t audio_len) {
  if (!h || B < 1 || n_frames < 1 || audio_len < h->cfg.n_group || audio_len % h->cfg.n_group) {
    fail(WG_ERR_INVALID, "bad B/n_frames, or audio_len is not a positive multiple of n_group");
    return 0;
  }
  if (check_envelope(h->cfg, B, audio_len / h->cfg.n_group) != WG_OK) return 0;
  RowGeom g = make_geom(h->cfg, B, audio_len / h->cfg.n_group, n_frames);
  return carve(h, g, nullptr).bytes;
}

static int run_wn(wg_handle* h, int k, const RowGeom& g, Workspace& w, _Float16*& cur, _Float16*& oth, hipStream_t s) {
  const wg_config& c = h->cfg;
  const int C = c.n_channels;
  const int BN = plan_infer_bn(C, g.Rp, h->n_cu, h->force_bn);   // 64-column tiles for small workloads: wg_plan.h
  const FlowOffsets& fo = h->flows[k];
  for (int i = 0; i < c.n_layers; ++i) {
    const LayerOffsets& lo = fo.layers[i];
    WnLayerArgs a;
    a.x_in = cur;
    a.x_out = oth;
    const bool fold0 = (i == 0) && h->fold_start;       // in_layers[0] o start on the a0 plane (one gathered K-step)
    a.x_tap = fold0 ? w.A0 : cur;
    a.x_chunks_per_tap = fold0 ? 1 : C / 64;
    a.melT = w.melT;
    a.frag16 = wn_frag16(C, BN) ? 1 : 0;
    a.wStA = fold0 && wn_res_a0(C) ? (const _Float16*)(h->d_blob + fo.wStA) : nullptr;
    a.a0_fold = fold0 ? 1 : 0;
    a.wA1c = (const _Float16*)((a.frag16 ? h->d_cond16 : h->d_cond) + h->cond_flow_bytes * k + h->cond_layer_bytes * i);
    a.wA1 = (const _Float16*)(h->d_blob + (a.frag16 ? (fold0 ? lo.wA1fx : lo.wA1x) : (fold0 ? lo.wA1f : lo.wA1)));
    a.bias1 = (const float*)(h->d_blob + lo.bias1);
    a.wA2 = (const _Float16*)(h->d_blob + lo.wA2);
    a.bias2 = (const float*)(h->d_blob + lo.bias2);
    a.wEs = (const _Float16*)(h->d_blob + lo.wEs);
    a.out = w.OUT;
    a.g = g;
    a.dil = 1 << i;
    a.n_cond_steps = c.n_mel_channels / 16;
    a.M = c.n_mel_channels;
    a.has_res = i < c.n_layers - 1;
    a.row0 = 0;
    a.tiles_per_phase = g.Rp / BN;
    a.sp = nullptr;
    a.save_t = a.save_s = a.save_a = nullptr;
    a.in0 = a.in1 = nullptr;
    a.out0 = nullptr;
    a.n_tiles = kPhases * a.tiles_per_phase;
    a.stamps = h->dbg_stamps;
    a.n_cu = h->n_cu;
    {
      Prof p(h, s, 2);
      HIP_TRY(launch_wn_layer(a, C, BN, s));
    }
    WG_DBG(s, "wn_layer");
    if (a.has_res) std::swap(cur, oth);
  }
  return WG_OK;
}

// `frames` (device, or null): per-utterance mel-frame counts of a ragged batch.
int wg_infer(wg_handle* h, const void* mel, const int32_t* frames, const void* z_init, const void* const* z_early,
             int32_t n_z_early, float sigma, void* audio, int32_t B, int32_t n_frames, int32_t io_dtype, void* workspace,
             size_t workspace_bytes, void* stream) {
  if (!h) return fail(WG_ERR_INVALID, "null handle");
  if (!h->finalized) return fail(WG_ERR_STATE, "wg_finalize has not been called");
  if (!mel || !z_init || !audio || !workspace) return fail(WG_ERR_INVALID, "null buffer");
  if (B < 1 || n_frames < 1) return fail(WG_ERR_INVALID, "bad B/n_frames");
  if (io_dtype != WG_F32 && io_dtype != WG_F16) return fail(WG_ERR_INVALID, "bad io_dtype");
  const wg_config& c = h->cfg;
  const int n_early = n_early_flows(c);
  if (n_z_early != n_early || (n_early && !z_early)) return fail(WG_ERR_INVALID, "expected %d early-noise tensors", n_early);
  const int L = n_frames * c.upsample_stride / c.n_group;
  // size range first, workspace size second.  (The [B*L][8] state, indexed with 32-bit rows in flow_kernel, needs no check
  // of its own: B * L * 8 <= 256 * B * T < 2^28 inside the envelope, the plane limit always binds first.)
  if (int rc = check_envelope(c, B, L)) return rc;
  RowGeom g = make_geom(c, B, L, n_frames);
  g.frames = (const int*)frames;
  Workspace w = carve(h, g, (char*)workspace);
  if (w.bytes > workspace_bytes) return fail(WG_ERR_WORKSPACE, "workspace %zu < required %zu", workspace_bytes, w.bytes);
  hipStream_t s = (hipStream_t)stream;
  const int C = c.n_channels;
  {
    Prof p(h, s, 3);
    // guard rows / rows >= L of both x planes must read as zero padding (model.py:98-102)
    HIP_TRY(launch_zero_fill(w.X0, 2 * w.x_bytes + w.a0_bytes, s));
  }
  {
    MelPackArgs u;
    u.mel = mel;
    u.frames = g.frames;
    u.melT = w.melT;
    u.B = B;
    u.M = c.n_mel_channels;
    u.T = n_frames;
    u.io_f16 = io_dtype == WG_F16;
    Prof p(h, s, 0);
    HIP_TRY(launch_mel_pack(u, s));
  }
  WG_DBG(s, "mel_pack");
  _Float16 *cur = w.X0, *oth = w.X1;
  int ze_idx = 0;
  auto base_flow_args = [&]() {
    FlowArgs f;
    memset(&f, 0, sizeof f);
    f.direction = 0;
    f.sigma = sigma;
    f.Z = w.Z;
    f.out = w.OUT;
    f.Z_w = w.Z;
    f.out_w = w.OUT;
    f.g = g;
    f.C = C;
    f.io_f16 = io_dtype == WG_F16;
    return f;
  };
  {
    const int k = c.n_flows - 1;
    FlowArgs f = base_flow_args();
    f.first = 1;
    f.z_extra = z_init;
    f.c_next = h->c_k[k];
    f.h_next = f.c_next / 2;
    f.wstart = (const float*)(h->d_blob + h->flows[k].wstart);
    f.bstart = (const float*)(h->d_blob + h->flows[k].bstart);
    f.out_init = (const float*)(h->d_blob + h->flows[k].out_init);
    f.x = cur;
    f.a0p = w.A0;
    f.skip_x = h->fold_start && wn_res_a0(C);
    Prof p(h, s, 1);
    HIP_TRY(launch_flow(f, s));
  }
  WG_DBG(s, "flow");
  for (int k = c.n_flows - 1; k >= 0; --k) {
    int rc = run_wn(h, k, g, w, cur, oth, s);
    if (rc) return rc;
    FlowArgs f = base_flow_args();
    f.c_in = h->c_k[k];
    f.h_in = f.c_in / 2;
    f.winv = (const float*)(h->d_blob + h->flows[k].winv);
    if (is_early(c, k)) {
      f.z_extra = z_early[ze_idx++];
      f.n_extra = c.n_early_size;
      if (!f.z_extra) return fail(WG_ERR_INVALID, "null early-noise tensor");
    }
    f.c_next = f.c_in + f.n_extra;
    f.last = (k == 0);
    if (f.last) {
      if (f.c_next != c.n_group) return fail(WG_ERR_STATE, "flow bookkeeping error");
      f.audio_out = audio;
    } else {
      f.h_next = h->c_k[k - 1] / 2;
      if (h->c_k[k - 1] != f.c_next) return fail(WG_ERR_STATE, "flow bookkeeping error");
      f.wstart = (const float*)(h->d_blob + h->flows[k - 1].wstart);
      f.bstart = (const float*)(h->d_blob + h->flows[k - 1].bstart);
      f.out_init = (const float*)(h->d_blob + h->flows[k - 1].out_init);
      f.x = cur;
      f.a0p = w.A0;
      f.skip_x = h->fold_start && wn_res_a0(C);
    }
    Prof p(h, s, 1);
    HIP_TRY(launch_flow(f, s));
  }
  WG_DBG(s, "flow");
  return WG_OK;
}

// `frames` (device, or null): per-utterance mel-frame counts of a ragged batch, which fixes the geometry to whole frames.
int wg_forward(wg_handle* h, const void* mel, const int32_t* frames, const void* audio, float* z, float* const* log_s,
               float* log_det_W, int32_t B, int32_t n_frames, int32_t audio_len, int32_t io_dtype, void* workspace,
               size_t workspace_bytes, void* stream) {
  if (!h) return fail(WG_ERR_INVALID, "null handle");
  if (!mel || !audio || !z || !log_s || !workspace || (!frames && !log_det_W)) return fail(WG_ERR_INVALID, "null buffer");
  if (frames && (n_frames < 1 || n_frames > (INT32_MAX >> 8))) return fail(WG_ERR_INVALID, "bad B/n_frames");
  if (frames && audio_len != n_frames * 256)
    return fail(WG_ERR_INVALID, "with frame counts audio_len must be 256 * n_frames (%d), got %d", n_frames * 256, audio_len);
  if (!h->finalized) return fail(WG_ERR_STATE, "wg_finalize has not been called");
  if (io_dtype != WG_F32 && io_dtype != WG_F16) return fail(WG_ERR_INVALID, "bad io_dtype");
  const wg_config& c = h->cfg;
  if (B < 1 || n_frames < 1 || audio_len < c.n_group || audio_len % c.n_group)
    return fail(WG_ERR_INVALID, "audio_len must be a positive multiple of n_group");
  // assert spect.size(2) >= audio.size(1)   (model.py:187)
  if ((int64_t)(n_frames - 1) * c.upsample_stride + c.upsample_kernel < audio_len)
    return fail(WG_ERR_INVALID, "upsampled mel (%d frames) shorter than audio (%d)", n_frames, audio_len);
  const int L = audio_len / c.n_group;
  if (int rc = check_envelope(c, B, L)) return rc;   // as in wg_infer: the one size check, before the workspace's
  RowGeom g = make_geom(c, B, L, n_frames);
  g.frames = (const int*)frames;   // the mel pack, the WN layers and the flow steps all take the padding columns from here
  Workspace w = carve(h, g, (char*)workspace);
  if (w.bytes > workspace_bytes) return fail(WG_ERR_WORKSPACE, "workspace %zu < required %zu", workspace_bytes, w.bytes);
  hipStream_t s = (hipStream_t)stream;
  const int C = c.n_channels;
  HIP_TRY(launch_zero_fill(w.X0, 2 * w.x_bytes + w.a0_bytes, s));
  {
    MelPackArgs u;
    u.mel = mel;
    u.frames = g.frames;
    u.melT = w.melT;
    u.B = B;
    u.M = c.n_mel_channels;
    u.T = n_frames;
    u.io_f16 = io_dtype == WG_F16;
    Prof p(h, s, 0);
    HIP_TRY(launch_mel_pack(u, s));
  }
  WG_DBG(s, "mel_pack");
  _Float16 *cur = w.X0, *oth = w.X1;
  int z_ch = 0;
  for (int k = 0; k <= c.n_flows; ++k) {
    FlowArgs f;
    memset(&f, 0, sizeof f);
    f.direction = 1;
    f.Z = w.Z;
    f.out = w.OUT;
    f.Z_w = w.Z;
    f.out_w = w.OUT;
    f.g = g;
    f.C = C;
    f.io_f16 = io_dtype == WG_F16;
    f.z_out = z;
    f.z_out_ch0 = z_ch;
    f.first = (k == 0);
    f.last = (k == c.n_flows);
    if (f.first) {
      f.audio_in = audio;
      f.c_in = c.n_group;
    } else {
      f.c_in = h->c_k[k - 1];
      f.h_in = f.c_in / 2;
      f.log_s_out = log_s[k - 1];
      if (!f.log_s_out) return fail(WG_ERR_INVALID, "null log_s[%d]", k - 1);
    }
    if (!f.last) {
      f.n_peel = is_early(c, k) ? c.n_early_size : 0;
      f.c_next = h->c_k[k];
      f.h_next = f.c_next / 2;
      if (f.c_in - f.n_peel != f.c_next) return fail(WG_ERR_STATE, "flow bookkeeping error");
      f.winv = (const float*)(h->d_blob + h->flows[k].wfwd);
      f.wstart = (const float*)(h->d_blob + h->flows[k].wstart);
      f.bstart = (const float*)(h->d_blob + h->flows[k].bstart);
      f.out_init = (const float*)(h->d_blob + h->flows[k].out_init);
      f.x = cur;
      f.a0p = w.A0;
      f.skip_x = h->fold_start && wn_res_a0(C);
      z_ch += f.n_peel;
    }
    {
      Prof p(h, s, 1);
      HIP_TRY(launch_flow(f, s));
    }
    if (!f.last) {
      int rc = run_wn(h, k, g, w, cur, oth, s);
      if (rc) return rc;
    }
  }
  if (log_det_W)
    for (int k = 0; k < c.n_flows; ++k) log_det_W[k] = (float)((double)B * L * h->flows[k].logdet);   // model.py:63
  return WG_OK;
}

static int loss_impl(const float* z, int64_t z_elems, const float* const* log_s, const int64_t* log_s_elems, int32_t n_flows,
                     const float* log_det_host, const float* log_det_dev, float sigma, float* loss_out, void* workspace,
                     size_t workspace_bytes, void* stream) {
  if (!z || !log_s || !log_s_elems || (!log_det_host && !log_det_dev) || !loss_out || !workspace) return fail(WG_ERR_INVALID, "null buffer");
  if (z_elems < 1 || n_flows < 1 || !(sigma > 0.f)) return fail(WG_ERR_INVALID, "bad sizes/sigma");
  if (workspace_bytes < 16) return fail(WG_ERR_WORKSPACE, "workspace %zu < required 16", workspace_bytes);
  hipStream_t s = (hipStream_t)stream;
  double* acc = (double*)workspace;
  HIP_TRY(hipMemsetAsync(acc, 0, 16, s));
  HIP_TRY(launch_reduce_sum(z, (size_t)z_elems, 1, acc, s));                              // sum z*z      train.py:43
  double log_det_total = 0.0;
  for (int k = 0; k < n_flows; ++k) {
    if (!log_s[k] || log_s_elems[k] < 1) return fail(WG_ERR_INVALID, "bad log_s[%d]", k);
    HIP_TRY(launch_reduce_sum(log_s[k], (size_t)log_s_elems[k], 0, acc + 1, s));          // sum log_s    train.py:36-40
    if (log_det_host) log_det_total += (double)log_det_host[k];                           // train.py:37,41
  }
  HIP_TRY(launch_loss_final(acc, log_det_total, log_det_dev, log_det_dev ? n_flows : 0, sigma, (double)z_elems, loss_out, s));   // train.py:43-44
  return WG_OK;
}

int wg_loss(const float* z, int64_t z_elems, const float* const* log_s, const int64_t* log_s_elems, int32_t n_flows,
            const float* log_det_W, float sigma, float* loss_out, void* workspace, size_t workspace_bytes, void* stream) {
  return loss_impl(z, z_elems, log_s, log_s_elems, n_flows, log_det_W, nullptr, sigma, loss_out, workspace, workspace_bytes, stream);
}

int wg_loss_dev(const float* z, int64_t z_elems, const float* const* log_s, const int64_t* log_s_elems, int32_t n_flows,
                const float* log_det_W_dev, float sigma, float* loss_out, void* workspace, size_t workspace_bytes, void* stream) {
  return loss_impl(z, z_elems, log_s, log_s_elems, n_flows, nullptr, log_det_W_dev, sigma, loss_out, workspace, workspace_bytes, stream);
}

double wg_macs_per_group_step(const wg_handle* h) {
  if (!h) return 0.0;
  const wg_config& c = h->cfg;
  const double C = c.n_channels, NS = h->NS, M = c.n_mel_channels;
  double macs = 8.0 * M * M * 4.0;   // upsample: 8 samples x M x M x 4 taps
  for (int k = 0; k < c.n_flows; ++k) {
    const double ck = h->c_k[k], hk = ck / 2;
    macs += hk * C + NS * 2 * C * c.n_layers + c.n_layers * (C * 2 * C * c.kernel_size) +
            (c.n_layers - 1) * (C * 2 * C) + C * C + C * 2 * hk + ck * ck;
  }
  return macs;
}

int wg_plan(const wg_config* cfg, int32_t direction, int32_t B, int32_t n_frames, int32_t n_cu, wg_plan_result* out) {
  if (!cfg || !out) return fail(WG_ERR_INVALID, "null argument");
  const wg_config& c = *cfg;
  if (wn_block_n(c.n_channels) == 0 || c.n_layers < 1 || c.n_layers > 10 || c.n_group != 8 || c.upsample_stride != 256 ||
      c.n_mel_channels < 16 || c.n_mel_channels % 16 != 0)
    return fail(WG_ERR_INVALID, "wg_plan: unsupported configuration (see wg_create)");
  if (direction != WG_PLAN_INFER && direction != WG_PLAN_FORWARD && direction != WG_PLAN_TRAIN)
    return fail(WG_ERR_INVALID, "wg_plan: bad direction");
  if (B < 1 || n_frames < 1 || n_cu < 1) return fail(WG_ERR_INVALID, "wg_plan: bad B / n_frames / n_cu");
  const int L = n_frames * c.upsample_stride / c.n_group;
  if (int rc = check_envelope(c, B, L)) return rc;
  RowGeom g = make_geom(c, B, L, n_frames);
  const PlanSwitches sw = read_plan_switches();
  const int C = c.n_channels;
  memset(out, 0, sizeof *out);
  out->halves = 1;
  if (direction == WG_PLAN_TRAIN) {
    // train_api.cpp: setup, then fwd_block_n on the (padded) rows; every layer is one single-tile launch per half
    int fp, rp;
    out->halves = plan_train_halves(B, g.Fp, g.Rp, n_cu, sw.train_halves, fp, rp);
    g.Fp = fp;
    g.Rp = rp;
    out->block_n = plan_train_bn(C, g.Rp, n_cu, sw.force_bn);
    out->form = WG_PLAN_SINGLE;
    out->n_tiles = kPhases * (g.Rp / out->halves / out->block_n);
  } else {
    // run_wn, then launch_wn_layer on 32 Rp / BN tiles: the same for every layer of every flow
    out->block_n = plan_infer_bn(C, g.Rp, n_cu, sw.force_bn);
    out->n_tiles = kPhases * (g.Rp / out->block_n);
    const WnLaunchPlan p = plan_wn_launch(C, out->block_n, out->n_tiles, n_cu, c.n_mel_channels / 16, sw);
    out->form = p.form == kPlanResident ? WG_PLAN_RESIDENT : p.form == kPlanPair ? WG_PLAN_PAIR : WG_PLAN_SINGLE;
    out->resident_wgs = 8 * p.resident_wgs;
    out->deep = p.deep ? 1 : 0;
  }
  out->frag16 = direction != WG_PLAN_TRAIN && wn_frag16(C, out->block_n) ? 1 : 0;
  out->rows_per_utterance = g.Fp;
  out->rows_per_phase = g.Rp;
  return WG_OK;
}

int wg_debug_set_stamp_buffer(wg_handle* h, void* device_buffer) {
  if (!h) return fail(WG_ERR_INVALID, "null handle");
  h->dbg_stamps = (unsigned long long*)device_buffer;
  wg::g_wgrad_stamps = (unsigned long long*)device_buffer;
  return WG_OK;
}

int wg_profile_enable(wg_handle* h, int32_t on) {
  if (!h) return fail(WG_ERR_INVALID, "null handle");
  h->prof = on != 0;
  h->prof_mask = on == 1 ? ~0u : (unsigned)on;      // on > 1: bit c set = class c is timed (fewer events per step)
  h->ev_used = 0;
  for (int i = 0; i < 8; ++i) {
    h->prof_ms[i] = 0;
    h->prof_n[i] = 0;
  }
  return WG_OK;
}

int wg_profile_read(wg_handle* h, double* ms, int64_t* n, int32_t n_classes) {
  if (!h || !ms || !n || n_classes < 4) return fail(WG_ERR_INVALID, "bad argument");
  for (size_t i = 0; i + 1 < h->ev_used; i += 2) {
    HIP_TRY(hipEventSynchronize(h->ev[i + 1]));
    float t = 0.f;
    HIP_TRY(hipEventElapsedTime(&t, h->ev[i], h->ev[i + 1]));
    h->prof_ms[h->ev_class[i]] += t;
    h->prof_n[h->ev_class[i]] += 1;
  }
  h->ev_used = 0;
  for (int i = 0; i < (n_classes < 8 ? n_classes : 8); ++i) {
    ms[i] = h->prof_ms[i];
    n[i] = h->prof_n[i];
  }
  return WG_OK;
}

}  // extern "C"
