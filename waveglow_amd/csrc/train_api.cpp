// C ABI of the training direction (include/waveglow_amd.h: wg_train_*): launch sequencing of train.hip.
// Reference: WaveGlow.forward under autograd (src/waveglow/model.py:178-221) and loss.backward() (train.py:190-199).
#include <cstring>

#include "wg_host.h"
#include "wg_train.h"

using namespace wg;

namespace {

// A training launch: HIP_TRY, and under WG_DEBUG_SYNC=1 a device synchronise and a stderr line per call.
#define TR_TRY(expr)                                                                         \
  do {                                                                                       \
    HIP_TRY(expr);                                                                           \
    if (dbg_sync()) {                                                                        \
      hipError_t _s = hipDeviceSynchronize();                                                \
      fprintf(stderr, "[wg-train] %s -> %s\n", #expr, hipGetErrorString(_s));                \
      fflush(stderr);                                                                        \
      if (_s != hipSuccess) return fail(WG_ERR_HIP, "%s", hipGetErrorString(_s));            \
    }                                                                                        \
  } while (0)

// per-class device timing of the training launches (wg_profile_enable / wg_profile_read, classes 4..7)
#define TR_PROF(st, cls, stmt)                      \
  do {                                             \
    wg_internal_prof_event(h, (void*)(st), cls);   \
    stmt;                                          \
    wg_internal_prof_event(h, (void*)(st), cls);   \
  } while (0)

size_t max_sz(size_t a, size_t b) { return a > b ? a : b; }

struct TrainWs {
  // fp16 planes (elements).  Layer planes: one set per layer of `slots` flows -- every flow (full save), or two flow slots
  // k & 1 (WG_TRAIN_RECOMPUTE: the backward replays a flow's forward into its slot), see plane_layer
  _Float16 *X, *T, *S, *A;      // [slots * n_layers] x C/64 chunks each (plane_c elements per layer)
  _Float16 *GP;                 // [slots * n_layers] x 2C/64 chunks, contiguous: the K operand of the cond_layer dgrad
  _Float16 *GXL;                // [n_layers] x C/64 chunks: d x_i of the flow in flight (one buffer per layer: see chains)
  _Float16 *GO[2], *SP, *MELP, *GSP;   // d out plane (per flow parity), spectrogram planes, mel planes, d spect planes
  float *Zpost, *OUT;           // [n_flows][B*L*8]
  float *GZ;                    // [B*L*8]
  float *slab[2], *slab2[2];    // blocked wgrad slabs (dW1 | dW2), two sets: a layer's slabs are reduced beside the NEXT layer's launch
  float *part[2], *part2[2];    // column-sum partials of the two weight-gradient jobs (two sets)
  float *ext[2], *extb[2];      // d (W_end W_skip) partials [n_slabs][16][C] and their column sums [n_slabs][16]
  float *slab_up, *part3;       // d upsample slabs (one per phase) / partials of the row kernels of a flow and of d upsample
  float *DSP;                   // WG_TRAIN_RECOMPUTE only: fp32 d spect accumulator planes [M8/64][R][64] (per-flow GEMMs)
  float *OUTs;                  // WG_TRAIN_RECOMPUTE only: [B*L*8] skip sums of the replayed flows (OUT[k] is saved state)
  int slots;                    // flows whose layer planes the workspace holds at once
  size_t plane_c;               // elements of one C-channel plane set
  size_t rows8;                 // B*L*8
  size_t zero_bytes;            // prefix that `fresh` clears (all planes)
  size_t bytes;
};

TrainWs carve(const wg_config& c, const RowGeom& g, const int* n_slabs, char* base, bool recompute) {
  TrainWs w;
  const int C = c.n_channels, M8 = c.n_mel_channels * 8;
  w.slots = recompute ? 2 : c.n_flows;
  const int SL = w.slots * c.n_layers;             // layers with planes of their own
  const size_t chunk = (size_t)g.R * 64;           // elements of one 64-channel plane
  w.plane_c = (size_t)(C / 64) * chunk;
  size_t off = 0;
  auto take = [&](size_t bytes) { char* p = base + off; off += align_up(bytes); return p; };
  w.X = (_Float16*)take((size_t)SL * w.plane_c * 2);
  w.T = (_Float16*)take((size_t)SL * w.plane_c * 2);
  w.S = (_Float16*)take((size_t)SL * w.plane_c * 2);
  w.A = (_Float16*)take((size_t)SL * w.plane_c * 2);
  w.GP = (_Float16*)take((size_t)SL * 2 * w.plane_c * 2);
  w.GXL = (_Float16*)take((size_t)c.n_layers * w.plane_c * 2);
  w.GO[0] = (_Float16*)take(chunk * 2);
  w.GO[1] = (_Float16*)take(chunk * 2);
  w.SP = (_Float16*)take((size_t)(M8 / 64) * chunk * 2);
  w.MELP = (_Float16*)take(2 * chunk * 2);
  w.GSP = (_Float16*)take((size_t)(M8 / 64) * chunk * 2);
  w.zero_bytes = off;
  w.rows8 = (size_t)g.B * g.L * 8;
  w.Zpost = (float*)take((size_t)c.n_flows * w.rows8 * 4);
  w.OUT = (float*)take((size_t)c.n_flows * w.rows8 * 4);
  w.GZ = (float*)take(w.rows8 * 4);
  w.DSP = recompute ? (float*)take((size_t)(M8 / 64) * chunk * 4) : nullptr;     // every entry it reads it has written
  w.OUTs = recompute ? (float*)take(w.rows8 * 4) : nullptr;
  const int cc = C / 64, mc = M8 / 64;
  const size_t t1 = (size_t)wgrad_tiles(2 * cc, 3 * cc + mc), t2 = (size_t)wgrad_tiles(cc, cc);
  for (int q = 0; q < 2; ++q) {
    w.slab[q] = (float*)take((size_t)n_slabs[0] * t1 * kWgradTileFloats * 4);
    w.slab2[q] = (float*)take((size_t)n_slabs[1] * t2 * kWgradTileFloats * 4);
    w.part[q] = (float*)take((size_t)n_slabs[0] * 2 * C * 4);
    w.part2[q] = (float*)take((size_t)n_slabs[1] * C * 4);
    w.ext[q] = (float*)take((size_t)n_slabs[1] * 16 * C * 4);
    w.extb[q] = (float*)take((size_t)n_slabs[1] * 16 * 4);
  }
  w.slab_up = (float*)take((size_t)kPhases * wgrad_tiles(mc, 8) * kWgradTileFloats * 4);
  w.part3 = (float*)take(max_sz(max_sz((size_t)flow_bwd_workgroups(g) * 64, (size_t)start_wgrad_workgroups(g) * 5 * C),
                                (size_t)kPhases * M8) * 4);
  w.bytes = off;
  return w;
}

struct Ctx {
  const wg_config* c;
  const int* ck;
  RowGeom g;
  TrainWs w;
  int C, FL, M8, K1, nl;
  int n_cu;
  int halves;      // 2: the batch runs as two independent half-batch chains (see setup)
  int n_slabs[2];  // row ranges of the two jobs of a weight-gradient launch (see setup)
  bool serial;     // WG_TRAIN_SERIAL=1: everything on the caller's stream (profiling of single kernels, A/B runs)
  bool recompute;  // WG_TRAIN_RECOMPUTE: two flow slots of layer planes, the backward replays the others (see carve)
};

// index of the plane set of layer i of flow k: its own (full save) or its flow slot's (WG_TRAIN_RECOMPUTE)
size_t plane_layer(const Ctx& x, int k, int i) { return (size_t)(x.recompute ? (k & 1) : k) * x.nl + i; }

// `to` continues after everything enqueued on `from` so far
hipError_t order_after(wg_handle* h, hipStream_t from, hipStream_t to) {
  if (from == to) return hipSuccess;
  hipEvent_t e = wg_internal_sync_event(h);
  if (!e) return hipErrorOutOfMemory;
  hipError_t r = hipEventRecord(e, from);
  return r != hipSuccess ? r : hipStreamWaitEvent(to, e, 0);
}

int setup(wg_handle* h, int32_t B, int32_t n_frames, int32_t audio_len, void* workspace, size_t workspace_bytes, int32_t flags,
          Ctx& x) {
  if (!h) return fail(WG_ERR_INVALID, "null handle");
  if (flags & ~WG_TRAIN_RECOMPUTE) return fail(WG_ERR_INVALID, "unknown wg_train flags");
  x.recompute = (flags & WG_TRAIN_RECOMPUTE) != 0;
  x.c = &h->cfg;
  x.ck = h->c_k.data();
  const wg_config& c = *x.c;
  if (B < 1 || n_frames < 1 || audio_len < c.n_group || audio_len % c.n_group)
    return fail(WG_ERR_INVALID, "audio_len must be a positive multiple of n_group");
  if ((int64_t)(n_frames - 1) * c.upsample_stride + c.upsample_kernel < audio_len)    // model.py:187
    return fail(WG_ERR_INVALID, "upsampled mel shorter than audio");
  const int L = audio_len / c.n_group;
  x.g = make_geom(h->cfg, B, L, n_frames);
  x.n_cu = h->n_cu;     // of the handle's device: decides the chain geometry (workspace layout) below
  // Chains: the two halves of an even batch as two chains of half-size launches on two streams where that fills idle CUs
  // (plan_train_halves, wg_plan.h; WG_TRAIN_HALVES = 1: never, 2: always (tests)).  The rows per utterance Fp are then
  // padded up so that the first B/2 utterances end on a tile boundary.  Rows past an utterance's last frame are guard rows
  // like the others: never valid, always written as zeros -- the only rows of the other half a chain's dilated taps can reach.
  {
    int fp, rp;
    x.halves = plan_train_halves(B, x.g.Fp, x.g.Rp, x.n_cu, read_plan_switches().train_halves, fp, rp);
    if (x.halves == 2) {
      x.g.Fp = fp;
      x.g.Rp = rp;
      x.g.R = kPhases * rp + 2 * kRowPad;
    }
    const char* se = getenv("WG_TRAIN_SERIAL");
    x.serial = se && *se == '1';
  }
  // Slabs of the weight-gradient launches (train.hip: wgrad_kernel): a layer's workgroups -- tiles of d W1 x its slabs + tiles
  // of d W2 x its slabs -- should be ONE round of one workgroup per CU, all equally long.  d W1 gets CUs / (all tiles) slabs;
  // d W2, whose steps cost ~17 % more (the extra d out plane, its column sums), gets the CUs that are left: more, shorter
  // slabs (config 4: 11 tiles x 21 slabs + 1 tile x 25 slabs = 256 workgroups of 110 / 92 steps).
  {
    const int cc = c.n_channels / 64, mc = c.n_mel_channels * 8 / 64;
    const int t1 = wgrad_tiles(2 * cc, 3 * cc + mc), t2 = wgrad_tiles(cc, cc);
    const long long total_steps = (long long)kPhases * (x.g.Rp / 32);
    long long s1 = x.n_cu / (t1 + t2), s2;
    if (s1 < 1) s1 = 1;
    s2 = ((long long)x.n_cu - s1 * t1) / t2;
    if (s2 < s1) s2 = s1;
    if (const char* e = getenv("WG_TRAIN_SLABS")) {      // tests: pin the number of slabs, "<d W1>[,<d W2>]"
      int a_ = 0, b_ = 0;
      const int n = sscanf(e, "%d,%d", &a_, &b_);
      if (n >= 1 && a_ >= 1) { s1 = a_; s2 = (n == 2 && b_ >= 1) ? b_ : a_; }
    }
    if (s1 > total_steps) s1 = total_steps;
    if (s2 > total_steps) s2 = total_steps;
    x.n_slabs[0] = (int)s1;
    x.n_slabs[1] = (int)s2;
  }
  x.w = carve(c, x.g, x.n_slabs, (char*)workspace, x.recompute);
  // A workspace keeps one layout from its forward to its backward.  Where the two sizes differ they tell the layouts apart:
  // a recompute workspace is then smaller than a full-save one, so a call whose flags do not match the size it is given is
  // refused.  At a depth where recomputation saves nothing (one or two flows: the two slots hold every flow and nothing is
  // replayed; one layer per flow: the fp32 d spect accumulator outweighs the planes saved) the flag still runs, on a
  // workspace of its own size, and only the flags say which layout a workspace has.
  const size_t full = x.recompute ? carve(c, x.g, x.n_slabs, nullptr, false).bytes : x.w.bytes;
  const size_t rec = x.recompute ? x.w.bytes : carve(c, x.g, x.n_slabs, nullptr, true).bytes;
  if (workspace && rec < full) {
    if (x.recompute && workspace_bytes >= full)
      return fail(WG_ERR_INVALID, "WG_TRAIN_RECOMPUTE with a full-save training workspace: flags and workspace size do not match");
    if (!x.recompute && workspace_bytes < full && workspace_bytes >= rec)
      return fail(WG_ERR_INVALID, "training workspace of the WG_TRAIN_RECOMPUTE size without the flag: flags and workspace size do not match");
  }
  if (workspace) {
    if (x.w.bytes > workspace_bytes) return fail(WG_ERR_WORKSPACE, "training workspace too small");
  }
  if ((size_t)x.g.R * 128 >= (1ull << 32)) return fail(WG_ERR_INVALID, "plane too large for 32-bit offsets");
  x.C = c.n_channels;
  x.nl = c.n_layers;
  x.FL = c.n_flows * c.n_layers;
  x.M8 = c.n_mel_channels * 8;
  x.K1 = 3 * x.C + x.M8;
  return WG_OK;
}

// every pointer of the weight / gradient blocks that the call sequence dereferences
int check_weights(const wg_train_weights* w, int n_flows) {
  if (!w->a1 || !w->a1c || !w->b1 || !w->a2 || !w->b2 || !w->es || !w->wat || !w->wbt || !w->wct || !w->wup || !w->bup ||
      !w->wstart || !w->bstart || !w->out_init || !w->w1x1)
    return fail(WG_ERR_INVALID, "wg_train_weights has a null member");
  for (int k = 0; k < n_flows; ++k)
    if (!w->wstart[k] || !w->bstart[k] || !w->out_init[k] || !w->w1x1[k])
      return fail(WG_ERR_INVALID, "wg_train_weights has a null per-flow pointer");
  return WG_OK;
}
int check_grads(const wg_train_grads* g, int n_flows) {
  if (!g->dw1 || !g->db1 || !g->dw2 || !g->db2 || !g->dwes || !g->dwup || !g->dbup || !g->dstart || !g->dout_init ||
      !g->dw1x1)
    return fail(WG_ERR_INVALID, "wg_train_grads has a null member");
  for (int k = 0; k < n_flows; ++k)
    if (!g->dstart[k] || !g->dout_init[k] || !g->dw1x1[k])
      return fail(WG_ERR_INVALID, "wg_train_grads has a null per-flow pointer");
  return WG_OK;
}

// One WN-layer-kernel GEMM over part `part` of `parts` equal row ranges of every phase (parts = 1: every column).
// (Measured and dropped: splitting a layer whose tile count is not a multiple of the CU count into a whole-rounds
// launch of 128-column tiles and a tail launch of 64-column tiles on the same stream.  A 64-column tile streams the same
// A fragments and takes ~80 % of a 128-column tile's time, so 2 + 0.8 rounds plus a second launch is no faster than 3.)
template <class Launch>
hipError_t launch_part(WnLayerArgs a, const RowGeom& g, int bn, int part, int parts, Launch launch) {
  const int rows = g.Rp / parts;
  a.row0 = part * rows;
  a.tiles_per_phase = rows / bn;
  a.n_tiles = kPhases * a.tiles_per_phase;
  return launch(a, bn);
}

SlabSeg make_seg(const float* slabs, int n_slabs, size_t stride, size_t n, float scale, float* out, int row_len, int perm) {
  SlabSeg g;
  g.slabs = slabs; g.out = out; g.stride = stride; g.n = n; g.n_slabs = n_slabs; g.scale = scale;
  g.row_len = row_len; g.perm = perm;
  g.blocked = 0; g.m_chunks = 0; g.k_chunks = 0; g.n_groups = 1; g.out_group_stride = 0;
  return g;
}

PRun run_of(const _Float16* base, int n_chunks, int dt) {
  PRun r;
  r.base = base;
  r.n_chunks = n_chunks;
  r.dt = dt;
  return r;
}


// tile width of the fused layer kernel in the training forward and the gradient paths (plan_train_bn, wg_plan.h); WG_FORCE_BN
// is read on every call
int fwd_block_n(const Ctx& x) { return plan_train_bn(x.C, x.g.Rp, x.n_cu, read_plan_switches().force_bn); }

// stream of the forward's second chain (the caller's stream `s` is the first): see setup
int second_chain_stream(wg_handle* h, const Ctx& x, hipStream_t s, hipStream_t& sB) {
  sB = s;
  if (x.halves == 2 && !x.serial && !(sB = wg_internal_aux_stream(h, 0)))
    return fail(WG_ERR_HIP, "cannot create the second chain's stream");
  return WG_OK;
}

// mel planes, then upsample (ConvTranspose1d 1024/256, model.py:145-150, :186-189) + squeeze (:191-193): one matrix per
// phase -> the SP planes every layer's conditioning K-segment reads
int spect_planes(const Ctx& x, const wg_train_weights* wt, const void* mel, hipStream_t s) {
  const RowGeom& g = x.g;
  const TrainWs& w = x.w;
  TR_TRY(launch_mel_plane(mel, 0, x.c->n_mel_channels, g, w.MELP, s));
  PGemmArgs a;
  memset(&a, 0, sizeof a);
  a.n_runs = 4;
  for (int j = 0; j < 4; ++j) a.run[j] = run_of(w.MELP, 2, -32 * j);
  a.A = (const _Float16*)wt->wup;
  a.a_phase_stride = (long long)x.M8 * 512;
  a.ktot = 512;
  a.n_blk = x.M8 / 32;
  a.M = x.M8;
  a.bias = wt->bup;
  a.g = g;
  a.o0 = w.SP;
  TR_TRY(launch_plane_gemm(a, s));
  return WG_OK;
}

// The WN of flow k with saved activations (X / T / S / A planes of its layers, plane_layer), its output accumulated into
// `out` = OUT[k] (initialised by the flow step before it; a replay passes the scratch OUTs).  The flow step's writes on `s`
// come first; sB (the second chain, = s for one) is joined back into `s` at the end.
int wn_flow_forward(wg_handle* h, const Ctx& x, const wg_train_weights* wt, int k, int BNw, float* out, hipStream_t s,
                    hipStream_t sB) {
  const wg_config& c = *x.c;
  const RowGeom& g = x.g;
  const TrainWs& w = x.w;
  const int C = x.C, nl = x.nl, M8 = x.M8;
  const int cc = C / 64, mc = M8 / 64;
  // per-layer sizes (fp16 elements) of the forward fragment tensors (include/waveglow_amd.h: wg_train_weights)
  const int NW = wn_waves(C), MBw = C / (32 * NW), MTw = 2 * MBw;
  const size_t a1_n = (size_t)2 * (3 * cc) * NW * MTw * 2 * 64 * 8, a1c_n = (size_t)2 * mc * NW * MTw * 2 * 64 * 8;
  const size_t a2_n = (size_t)NW * MBw * (C / 16) * 64 * 8, es_n = (size_t)(C / 32) * 64 * 8;
  HIP_TRY(order_after(h, s, sB));
  for (int i = 0; i < nl; ++i) {
    const int fl = k * nl + i, d = 1 << i;
    const size_t pl = plane_layer(x, k, i);
    const _Float16* Xi = w.X + pl * w.plane_c;
    _Float16* Ai = w.A + pl * w.plane_c;
    // ONE fused launch per layer (kernels.hip: wn_layer_kernel<..., TR = true>): in_layers[i] + cond_layer slice as one
    // K-extended GEMM, gate in registers (tanh / sigmoid / acts saved as planes for the backward pass), res rows +
    // residual add -> x_{i+1}, skip rows folded through WN.end -> OUT   (model.py:123-137)
    WnLayerArgs a;
    memset(&a, 0, sizeof a);
    a.x_in = Xi;
    a.x_tap = Xi;
    a.x_chunks_per_tap = cc;
    a.x_out = (i < nl - 1) ? w.X + (pl + 1) * w.plane_c : nullptr;
    a.wA1 = (const _Float16*)wt->a1 + (size_t)fl * a1_n;
    a.wA1c = (const _Float16*)wt->a1c + (size_t)fl * a1c_n;
    a.bias1 = wt->b1 + (size_t)fl * 2 * C;
    a.wA2 = (const _Float16*)wt->a2 + (size_t)fl * a2_n;
    a.bias2 = wt->b2 + (size_t)fl * C;
    a.wEs = (const _Float16*)wt->es + (size_t)fl * es_n;
    a.out = out;
    a.g = g;
    a.dil = d;
    a.n_cond_steps = mc;
    a.M = c.n_mel_channels;
    a.has_res = i < nl - 1;
    a.n_cu = x.n_cu;
    a.sp = w.SP;
    a.save_t = w.T + pl * w.plane_c;
    a.save_s = w.S + pl * w.plane_c;
    a.save_a = Ai;
    for (int half = 0; half < x.halves; ++half) {
      hipStream_t sh = half ? sB : s;
      TR_PROF(sh, 4, TR_TRY(launch_part(a, g, BNw, half, x.halves, [&](const WnLayerArgs& q, int bn) { return launch_wn_layer_train(q, C, bn, sh); })));
    }
  }
  HIP_TRY(order_after(h, sB, s));
  return WG_OK;
}

// WG_TRAIN_RECOMPUTE: flow k's forward once more, into its plane slot.  x_0 comes from the saved state Zpost[k] (the
// post-1x1 state in the training direction, the state entering inverse step k in synthesis) through start_replay, which
// shares flow_kernel's x_0 arithmetic; then wn_flow_forward's launches with the forward's tile width (fwd_block_n) and
// half-batch split, their skip sums into the scratch OUTs.  X / T / S / A come out bit-identical to the forward's.
// chains: the second half-batch chain on its own stream, as in the forward (false: both halves on `s`, same launches).
int replay_flow(wg_handle* h, const Ctx& x, const wg_train_weights* wt, int k, bool chains, hipStream_t s) {
  hipStream_t sB = s;
  if (chains && x.halves == 2 && !x.serial) {
    sB = wg_internal_aux_stream(h, 0);
    if (!sB) return fail(WG_ERR_HIP, "cannot create the second chain's stream");
  }
  FlowArgs f;
  memset(&f, 0, sizeof f);
  f.g = x.g;
  f.C = x.C;
  f.Z = x.w.Zpost + (size_t)k * x.w.rows8;
  f.h_next = x.ck[k] / 2;
  f.wstart = wt->wstart[k];
  f.bstart = wt->bstart[k];
  f.x = x.w.X + plane_layer(x, k, 0) * x.w.plane_c;
  TR_TRY(launch_start_replay(f, s));
  return wn_flow_forward(h, x, wt, k, fwd_block_n(x), x.w.OUTs, s, sB);
}

// WG_TRAIN_RECOMPUTE: d spect += cond_layer^T d pre over the layers of flow k -- K = n_layers * 2C of its slot's GP planes
// (contiguous) against the matching K range of wct -- in the fp32 DSP planes: stored by the first flow of the backward,
// added by the others; the last one also writes the loss-scaled fp16 GSP planes that dmel and the d upsample job read.
int dspect_flow(const Ctx& x, const wg_train_weights* wt, int k, bool first, bool last, hipStream_t s) {
  const int cc = x.C / 64;
  PGemmArgs a;
  memset(&a, 0, sizeof a);
  a.n_runs = 1;
  a.run[0] = run_of(x.w.GP + plane_layer(x, k, 0) * 2 * x.w.plane_c, x.nl * 2 * cc, 0);
  a.n_blk = x.M8 / 32;
  a.A = (const _Float16*)wt->wct + (size_t)k * x.nl * 2 * cc * a.n_blk * 2048;     // K offset of flow k's first layer
  a.ktot = x.nl * 2 * x.C;
  a.M = x.M8;
  a.g = x.g;
  a.acc = x.w.DSP;
  a.acc_in = !first;
  a.o0 = last ? x.w.GSP : nullptr;
  TR_TRY(launch_plane_gemm(a, s));
  return WG_OK;
}

// where entry fl of a per-layer gradient tensor lives: dense, or in interleaved per-layer records (wg_train_grads)
size_t grad_ofs(const wg_train_grads* gr, int nl, int fl, size_t dense) {
  return gr->layer_stride ? (size_t)(fl / nl) * (size_t)gr->flow_stride + (size_t)(fl % nl) * (size_t)gr->layer_stride
                          : (size_t)fl * dense;
}

// ---------------------------------------------------------------------------------------------
// What the two backward drivers share (wg_train_backward: training direction, flows descending;
// wg_train_infer_backward: synthesis direction, flows ascending): the plan of one call, the WN data-gradient chain
// of one flow (wn_flow_backward) and the d spect tail behind the last flow (dspect_finish).
//
// Streams of one backward call.  The caller's stream `s` carries chain 0 (d acts / gate derivative and d x of the first
// half of the batch, or of all of it) and the row kernels of every flow; sB carries chain 1 (the second half, see setup:
// training direction only); sW (lowest priority) carries the weight-gradient launches (and the per-flow d spect GEMMs of
// WG_TRAIN_RECOMPUTE) and sR (lowest priority too) their slab reductions, which nothing downstream in the same call waits
// for: they fill the CUs the chains leave idle.  Everything is joined back into `s` before the call returns, so the caller
// sees the usual stream semantics.  Without parameter gradients sW = sR = s; WG_TRAIN_SERIAL=1: all four are `s`.
// (Two chains pay in the forward pass, -23 % per layer at config 4; in the backward pass the weight-gradient stream
//  already fills the idle CUs and a second chain measured +0.7 ms per step: off unless WG_TRAIN_BWD_HALVES=2, tests.)
//
// Buffers the streams share and what orders their reuse.  Every reuse is by the NEXT flow processed (k - 1 descending,
// k + 1 ascending) or by the one AFTER it (k -+ 2: the same parity), so the rules hold for both loop directions:
//   GXL[i] (d x_i)   written by the chains' d x launch of layer i, read by their layer i-1 launches (same stream) and by
//                    sW's second job of layer i-1: the next flow's layer-i launch waits for that job (w_done[i-1], not yet
//                    re-marked by the next flow at that point: its layer i-1 comes later);
//   GO[k & 1]        written by flow k's pre kernel on s, read by the chains and by all of flow k's jobs on sW: the pre
//                    kernel of the flow after the next waits for the last of them (w_flow[k & 1]);
//   GP, X, T, S, A   full save: one set per layer of the whole model, no reuse inside a call (GP is read by the final
//                    d spect GEMM on s).  WG_TRAIN_RECOMPUTE: one set per layer of flow slot k & 1, read by flow k's chain
//                    launches (s / sB, joined into s at the end of the flow) and by its weight-gradient jobs and d spect
//                    GEMM on sW (X, A, GP): the replay of the flow after the next into the slot runs on s behind the same
//                    w_flow[k & 1] wait as its pre kernel.  The forward leaves the first two flows of the backward in
//                    their slots: they are not replayed;
//   slab sets        a layer's slabs are reduced by a launch of its own on sR -- HBM-bound and small in registers and LDS,
//                    so its workgroups run beside the NEXT layer's weight-gradient workgroups on sW (MFMA / L2-bound, one
//                    per CU).  Two sets: launch n + 2 on sW waits for the reduction of launch n (r_done), the reduction of
//                    launch n for launch n itself (l_done);
//   GZ, part3        row kernels and their reductions, on s alone.
// Without parameter gradients everything but chain 1 runs on `s` and is reused in stream order.  Across the calls of a flow
// range (training direction) everything is joined into s at the end of a call.
// Marks are waited on one or two flows / launches after their record: events of their own (wg_internal_mark_event, slots
// 0-9 = w_done[layer], 10-11 = w_flow[parity], 12-13 = l_done[set], 14-15 = r_done[set]); a null entry = not recorded in
// this call, nothing to wait for.
// ---------------------------------------------------------------------------------------------
struct BwdPlan {
  const _Float16 *wat, *wbt;       // fragment tensors of the two dgrad GEMMs (include/waveglow_amd.h: wat, wbt)
  size_t kstep_n, wat_n, wbt_n;    // their elements per 64-deep K-step and per layer
  bool fuse;                       // false (WG_TRAIN_NO_FUSE=1: tests, A/B): d acts + gate derivative as launches of their own
  int BNw;                         // tile width of the chain launches
  int bh;                          // chains: 1, or the forward's 2 half-batch chains
  float inv;                       // 1 / loss scale
  hipStream_t s, sB, sW, sR;
  bool serial;                     // sW = sR = s: no marks
  int n_wgrad;                     // weight-gradient launches so far (slab set = its parity)
  hipEvent_t w_done[10], w_flow[2], l_done[2], r_done[2];
};

hipError_t mark_on(wg_handle* h, bool serial, hipStream_t st, hipEvent_t& e, int slot) {
  e = nullptr;
  if (serial) return hipSuccess;
  e = wg_internal_mark_event(h, slot);
  return e ? hipEventRecord(e, st) : hipErrorOutOfMemory;
}
hipError_t wait_on(hipStream_t st, hipEvent_t e) { return e ? hipStreamWaitEvent(st, e, 0) : hipSuccess; }

// tile width of the backward chain launches: the forward's, or WG_TRAIN_BWD_BN (A/B runs of the backward alone)
int bwd_block_n(const Ctx& x) {
  if (const char* e = getenv("WG_TRAIN_BWD_BN")) {
    const int f = atoi(e);
    if (f == 64 || (f == 128 && wn_block_n(x.C) == 128)) return f;
  }
  return fwd_block_n(x);
}

// The plan of one backward call on stream `s`; gr null: no parameter gradients.  second_chain: the training direction,
// which may run the forward's two half-batch chains (WG_TRAIN_BWD_HALVES=2).  The environment is read on every call.
int bwd_plan(wg_handle* h, const Ctx& x, const wg_train_weights* wt, const wg_train_grads* gr, float scale, hipStream_t s,
             bool second_chain, BwdPlan& p) {
  if (gr && ((gr->layer_stride == 0) != (gr->flow_stride == 0) || gr->layer_stride < 0 || gr->flow_stride < 0))
    return fail(WG_ERR_INVALID, "wg_train_grads: layer_stride and flow_stride must both be 0 or both positive");
  memset(&p, 0, sizeof p);
  const int cc = x.C / 64, NW = wn_waves(x.C), MBw = x.C / (32 * NW);
  p.wat = (const _Float16*)wt->wat;
  p.wbt = (const _Float16*)wt->wbt;
  p.kstep_n = (size_t)2 * NW * MBw * 2 * 64 * 8;
  p.wat_n = (size_t)(cc + 1) * p.kstep_n;
  p.wbt_n = (size_t)(6 * cc) * p.kstep_n;
  const char* e = getenv("WG_TRAIN_NO_FUSE");
  p.fuse = !(e && *e == '1');
  p.BNw = bwd_block_n(x);
  p.bh = 1;
  if (second_chain && (e = getenv("WG_TRAIN_BWD_HALVES")) && atoi(e) == 2) p.bh = x.halves;
  p.inv = 1.0f / scale;
  p.s = p.sB = p.sW = p.sR = s;
  p.serial = x.serial || !gr;
  if (p.bh == 2 && !x.serial && !(p.sB = wg_internal_aux_stream(h, 0)))
    return fail(WG_ERR_HIP, "cannot create the second chain's stream");
  if (!p.serial) {
    if (!(p.sW = wg_internal_aux_stream(h, 1))) return fail(WG_ERR_HIP, "cannot create the weight-gradient stream");
    if (!(p.sR = wg_internal_aux_stream(h, 2))) return fail(WG_ERR_HIP, "cannot create the slab-reduction stream");
  }
  return WG_OK;
}

// The weight gradients of layer i of flow k, once d pre of the layer (GP) and gx = d x_{i+1} (null: the flow's last layer)
// are on sW's side of the stream order:
// d W1 = d pre x [x taps | spect]^T, d b1;
// d W2 = d x_{i+1} x acts^T, d b2  and  d (W_end W_skip_i) = d out x acts^T  share the X operand (acts): one
// job with the d out plane as the `extra` 16 rows (the last layer has no d x: the d out plane stands in as the
// job's G as well, and that part of the result is not used).
// Both jobs in ONE launch over the same slab partition (train.hip: wgrad_kernel), then the reduction of everything the
// launch left behind; layer 0 also leaves d out_init of the flow.
int layer_wgrad(wg_handle* h, const Ctx& x, BwdPlan& p, const wg_train_grads* gr, int k, int i, const _Float16* gx,
                const _Float16* GOk) {
  const RowGeom& g = x.g;
  const TrainWs& w = x.w;
  const int C = x.C, nl = x.nl, K1 = x.K1;
  const int cc = C / 64, mc = x.M8 / 64;
  const int fl = k * nl + i, d = 1 << i;
  const size_t pl = plane_layer(x, k, i);
  const _Float16* Xi = w.X + pl * w.plane_c;
  const _Float16* Ai = w.A + pl * w.plane_c;
  const _Float16* GPi = w.GP + pl * 2 * w.plane_c;
  const int* const n_slabs = x.n_slabs;
  hipStream_t sW = p.sW, sR = p.sR;
  const float inv = p.inv;
  WgradJob jb[2];
  const int set = p.n_wgrad++ & 1;
  memset(jb, 0, sizeof jb);
  jb[0].G = GPi;
  jb[0].m_chunks = 2 * cc;
  jb[0].n_runs = 4;
  jb[0].run[0] = run_of(Xi, cc, -d);
  jb[0].run[1] = run_of(Xi, cc, 0);
  jb[0].run[2] = run_of(Xi, cc, d);
  jb[0].run[3] = run_of(w.SP, mc, 0);
  jb[0].k_chunks = 3 * cc + mc;
  jb[0].slabs = w.slab[set];
  jb[0].bias_out = w.part[set];
  jb[1].G = gx ? gx : GOk;
  jb[1].m_chunks = gx ? cc : 1;
  jb[1].G_extra = GOk;
  jb[1].n_runs = 1;
  jb[1].run[0] = run_of(Ai, cc, 0);
  jb[1].k_chunks = cc;
  jb[1].slabs = w.slab2[set];
  jb[1].bias_out = w.part2[set];
  jb[1].extra_out = w.ext[set];
  jb[1].extra_bias_out = w.extb[set];
  HIP_TRY(wait_on(sW, p.r_done[set]));          // the reduction of the launch before last has read this slab set
  TR_PROF(sW, 6, TR_TRY(launch_wgrad(jb, 2, g, n_slabs, sW)));
  HIP_TRY(mark_on(h, p.serial, sW, p.l_done[set], 12 + set));
  // ---- reduction of everything this launch left behind, in NATURAL channel order (SlabSeg: perm bit 0 = rows are
  // channels, bit 1 = columns are)
  SlabSeg seg[kMaxSlabSegs];
  int n_seg = 0;
  const size_t n1 = (size_t)2 * C * K1;
  auto add_flat = [&](int job, const float* slabs, size_t stride, size_t n, float* out, int row_len, int perm) {
    seg[n_seg++] = make_seg(slabs, n_slabs[job], stride, n, inv, out, row_len, perm);
  };
  auto add_blocked = [&](int job, const float* slabs, int m_ch, int k_ch, float* out) {
    SlabSeg sg = make_seg(slabs, n_slabs[job], (size_t)wgrad_tiles(m_ch, k_ch) * kWgradTileFloats,
                          (size_t)wgrad_tiles(m_ch, k_ch) * kWgradTileFloats, inv, out, k_ch * 64, 3);
    sg.blocked = 1; sg.m_chunks = m_ch; sg.k_chunks = k_ch; sg.n_groups = 1;
    seg[n_seg++] = sg;
  };
  add_blocked(0, w.slab[set], 2 * cc, 3 * cc + mc, gr->dw1 + grad_ofs(gr, nl, fl, n1));
  add_flat(0, w.part[set], (size_t)2 * C, (size_t)2 * C, gr->db1 + grad_ofs(gr, nl, fl, (size_t)2 * C), 2 * C, 2);
  if (gx) {
    add_blocked(1, w.slab2[set], cc, cc, gr->dw2 + grad_ofs(gr, nl, fl, (size_t)C * C));
    add_flat(1, w.part2[set], (size_t)C, (size_t)C, gr->db2 + grad_ofs(gr, nl, fl, (size_t)C), C, 2);
  }
  add_flat(1, w.ext[set], (size_t)16 * C, (size_t)8 * C, gr->dwes + grad_ofs(gr, nl, fl, (size_t)8 * C), C, 2);
  // d out_init = sum over columns of (d b | d log_s), once per flow
  if (i == 0) add_flat(1, w.extb[set], 16, 8, gr->dout_init[k], 0, 0);
  HIP_TRY(wait_on(sR, p.l_done[set]));
  TR_TRY(launch_slab_reduce_multi(seg, n_seg, sR));
  HIP_TRY(mark_on(h, p.serial, sR, p.r_done[set], 14 + set));
  return WG_OK;
}

// d Wstart / d bstart of flow k from d x_0 (gx) and the state whose first h_k channels entered the start conv
int start_wgrad(const Ctx& x, const wg_train_grads* gr, int k, const _Float16* gx, const float* Zpost, float inv, hipStream_t s) {
  StartWgradArgs a;
  a.g = x.g;
  a.C = x.C;
  a.h = x.ck[k] / 2;
  a.GX = gx;
  a.Zpost = Zpost;
  a.partial = x.w.part3;
  TR_TRY(launch_start_wgrad(a, s));
  const SlabSeg sg = make_seg(x.w.part3, start_wgrad_workgroups(x.g), (size_t)5 * x.C, (size_t)5 * x.C, inv, gr->dstart[k], x.C, 2);
  TR_TRY(launch_slab_reduce_multi(&sg, 1, s));
  return WG_OK;
}

// d upsample: per phase, d spect (GSP) x mel frames q..q-3 (no sum over phases: one slab = one phase = one result)
int upsample_wgrad(const Ctx& x, const wg_train_grads* gr, float inv, hipStream_t s) {
  const TrainWs& w = x.w;
  const int M8 = x.M8, mc = M8 / 64;
  WgradJob a;
  memset(&a, 0, sizeof a);
  a.G = w.GSP;
  a.m_chunks = mc;
  a.n_runs = 4;
  for (int j = 0; j < 4; ++j) a.run[j] = run_of(w.MELP, 2, -32 * j);
  a.k_chunks = 8;
  a.slabs = w.slab_up;
  a.bias_out = w.part3;
  const int up_slabs = kPhases;
  TR_TRY(launch_wgrad(&a, 1, x.g, &up_slabs, s));
  SlabSeg sg[2];
  const size_t tile_n = (size_t)wgrad_tiles(mc, 8) * kWgradTileFloats;
  sg[0] = make_seg(w.slab_up, kPhases, tile_n, tile_n, inv, gr->dwup, 512, 1);      // rows to natural order, columns are mel taps
  sg[0].blocked = 1; sg[0].m_chunks = mc; sg[0].k_chunks = 8; sg[0].n_groups = kPhases; sg[0].out_group_stride = (size_t)M8 * 512;
  sg[1] = make_seg(w.part3, kPhases, M8, M8, inv, gr->dbup, M8, 2);
  TR_TRY(launch_slab_reduce_multi(sg, 2, s));
  return WG_OK;
}

// The WN data-gradient chain of flow k, last layer to first, once the flow's pre kernel has written GOk = GO[k & 1] on p.s:
// per layer d pre and d x_i on the p.bh chains (p.s, p.sB), and with parameter gradients the layer's weight-gradient job
// on p.sW behind them.  Chain 1 is joined back into p.s at the end; gx returns d x_0 (GXL[0]).
int wn_flow_backward(wg_handle* h, const Ctx& x, BwdPlan& p, const wg_train_grads* gr, int k, const _Float16* GOk,
                     const _Float16*& gx) {
  const RowGeom& g = x.g;
  const TrainWs& w = x.w;
  const int C = x.C, nl = x.nl, cc = C / 64;
  HIP_TRY(order_after(h, p.s, p.sB));
  gx = nullptr;                               // gx = d x_{i+1} (null: zero, the last layer has no res output)
  for (int i = nl - 1; i >= 0; --i) {
    const int fl = k * nl + i, d = 1 << i;
    const size_t pl = plane_layer(x, k, i);
    _Float16* GPi = w.GP + pl * 2 * w.plane_c;
    WnLayerArgs a;
    // Fused (round 3): the d x launch of layer i + 1 has already produced d pre of this layer behind its own result
    // (wn_layer_kernel MODE 4: the d x tile goes through LDS into the next GEMM instead of out to the planes and back in
    // through a launch of its own); only a flow's last layer, which has no d x above it, runs MODE 3 alone.
    if (!p.fuse || i == nl - 1) {
      // d acts = W_res^T d x_{i+1} + (W_end W_skip_i)^T d out ; gate derivative -> d pre   (wn_layer_kernel MODE 3)
      memset(&a, 0, sizeof a);
      const _Float16* Am = p.wat + (size_t)fl * p.wat_n;
      if (gx) {
        a.x_tap = gx;
        a.x_chunks_per_tap = cc;
        a.sp = GOk;
        a.n_cond_steps = 1;
        a.wA1 = Am;
        a.wA1c = Am + (size_t)cc * p.kstep_n;
      } else {
        a.x_tap = GOk;                     // last layer of a flow: no d x_{i+1}, the d out plane alone
        a.x_chunks_per_tap = 1;
        a.n_cond_steps = 0;
        a.wA1 = Am + (size_t)cc * p.kstep_n;
        a.wA1c = a.wA1;
      }
      a.dil = 0;
      a.g = g;
      a.M = x.c->n_mel_channels;
      a.n_cu = x.n_cu;
      a.in0 = w.T + pl * w.plane_c;
      a.in1 = w.S + pl * w.plane_c;
      a.out0 = GPi;
      for (int half = 0; half < p.bh; ++half) {
        hipStream_t sh = half ? p.sB : p.s;
        TR_PROF(sh, 5, TR_TRY(launch_part(a, g, p.BNw, half, p.bh, [&](const WnLayerArgs& q, int bn) { return launch_wn_plain(q, C, 3, bn, sh); })));
      }
    }
    if (gr) {
      // the weight-gradient stream continues once every chain has written its part of d pre (and of d x_{i+1} before it)
      HIP_TRY(order_after(h, p.s, p.sW));
      if (p.sB != p.s) HIP_TRY(order_after(h, p.sB, p.sW));
      // d W1 / d b1, d W2 / d b2, d (W_end W_skip_i) of the layer (and d out_init with layer 0) and their reduction
      if (int rc = layer_wgrad(h, x, p, gr, k, i, gx, GOk)) return rc;
      HIP_TRY(mark_on(h, p.serial, p.sW, p.w_done[i], i));
    }
    // d x_i = d x_{i+1} + sum_tap W_in[tap]^T d pre(t - (tap-1) d)   (wn_layer_kernel MODE 2: taps at +d, 0, -d)
    memset(&a, 0, sizeof a);
    a.x_tap = GPi;
    a.x_chunks_per_tap = 2 * cc;
    a.n_cond_steps = 0;
    a.wA1 = p.wbt + (size_t)fl * p.wbt_n;
    a.wA1c = a.wA1;
    a.dil = -d;
    a.g = g;
    a.M = x.c->n_mel_channels;
    a.n_cu = x.n_cu;
    a.in0 = gx;
    _Float16* const gxi = w.GXL + (size_t)i * w.plane_c;
    a.out0 = gxi;
    const int kind = (p.fuse && i > 0) ? 4 : 2;
    if (kind == 4) {      // ... and d acts + gate derivative of layer i - 1 on the tile (see above)
      a.wat_prev = p.wat + (size_t)(fl - 1) * p.wat_n;
      a.gout = GOk;
      a.t_prev = w.T + (pl - 1) * w.plane_c;
      a.s_prev = w.S + (pl - 1) * w.plane_c;
      a.dpre_prev = w.GP + (pl - 1) * 2 * w.plane_c;
    }
    for (int half = 0; half < p.bh; ++half) {
      hipStream_t sh = half ? p.sB : p.s;
      if (gr && i > 0) HIP_TRY(wait_on(sh, p.w_done[i - 1]));     // GXL[i]: see BwdPlan
      TR_PROF(sh, 5, TR_TRY(launch_part(a, g, p.BNw, half, p.bh, [&](const WnLayerArgs& q, int bn) { return launch_wn_plain(q, C, kind, bn, sh); })));
    }
    gx = gxi;
  }
  HIP_TRY(order_after(h, p.sB, p.s));
  return WG_OK;
}

// every gradient of the call is final on the caller's stream
int join_wgrad_streams(wg_handle* h, const BwdPlan& p) {
  HIP_TRY(order_after(h, p.sW, p.s));
  HIP_TRY(order_after(h, p.sR, p.s));
  return WG_OK;
}

// Behind the last flow: d spect (GSP planes) -> d mel and, with parameter gradients, d upsample; then the final joins.
int dspect_finish(wg_handle* h, const Ctx& x, const BwdPlan& p, const wg_train_weights* wt, const wg_train_grads* gr,
                  float* g_mel) {
  const TrainWs& w = x.w;
  hipStream_t s = p.s;
  if (x.recompute) {
    HIP_TRY(order_after(h, p.sW, s));      // the last flow's d spect GEMM (dspect_flow) wrote GSP on sW
  } else {
    // d spect = sum over every layer of cond_layer^T d pre: ONE GEMM with K = FL*2C over the kept d pre planes
    const int C = x.C, FL = x.FL;
    PGemmArgs a;
    memset(&a, 0, sizeof a);
    a.n_runs = 1;
    a.run[0] = run_of(w.GP, FL * 2 * (C / 64), 0);
    a.A = (const _Float16*)wt->wct;
    a.ktot = FL * 2 * C;
    a.n_blk = x.M8 / 32;
    a.M = x.M8;
    a.g = x.g;
    a.o0 = w.GSP;
    TR_TRY(launch_plane_gemm(a, s));
  }
  if (g_mel) {
    DmelArgs a;                             // d mel = the upsample's transpose applied to d spect (train.hip: dmel_kernel)
    a.g = x.g;
    a.GSP = w.GSP;
    a.wupt = (const _Float16*)wt->wupt;
    a.M = x.c->n_mel_channels;
    a.M8 = x.M8;
    a.inv_scale = p.inv;
    a.g_mel = g_mel;
    TR_TRY(launch_dmel(a, s));
  }
  if (!gr) return WG_OK;
  if (int rc = upsample_wgrad(x, gr, p.inv, s)) return rc;
  return join_wgrad_streams(h, p);
}

}  // namespace

extern "C" {

int32_t wg_wn_waves(int32_t n_channels) { return wn_waves(n_channels); }

size_t wg_train_workspace_bytes(const wg_handle* h, int32_t B, int32_t n_frames, int32_t audio_len, int32_t flags) {
  Ctx x;
  if (setup(const_cast<wg_handle*>(h), B, n_frames, audio_len, nullptr, 0, flags, x) != WG_OK) return 0;
  return x.w.bytes;
}

int wg_train_forward(wg_handle* h, const wg_train_weights* wt, const void* mel, const void* audio, float* z,
                     float* const* log_s, int32_t B, int32_t n_frames, int32_t audio_len, int32_t fresh,
                     void* workspace, size_t workspace_bytes, int32_t flags, void* stream) {
  if (!wt || !mel || !audio || !z || !log_s || !workspace) return fail(WG_ERR_INVALID, "null argument");
  Ctx x;
  int rc = setup(h, B, n_frames, audio_len, workspace, workspace_bytes, flags, x);
  if (rc) return rc;
  if ((rc = check_weights(wt, x.c->n_flows))) return rc;
  const wg_config& c = *x.c;
  const RowGeom& g = x.g;
  TrainWs& w = x.w;
  hipStream_t s = (hipStream_t)stream;
  const int C = x.C;
  hipStream_t sB;
  if ((rc = second_chain_stream(h, x, s, sB))) return rc;
  const int BNw = fwd_block_n(x);

  if (fresh) TR_TRY(hipMemsetAsync(workspace, 0, w.zero_bytes, s));
  if ((rc = spect_planes(x, wt, mel, s))) return rc;
  int z_ch = 0;
  for (int k = 0; k <= c.n_flows; ++k) {
    FlowArgs f;
    memset(&f, 0, sizeof f);
    f.direction = 1;
    f.g = g;
    f.C = C;
    f.io_f16 = 0;
    f.z_out = z;
    f.z_out_ch0 = z_ch;
    f.first = (k == 0);
    f.last = (k == c.n_flows);
    if (f.first) {
      f.audio_in = audio;
      f.c_in = c.n_group;
    } else {
      f.Z = w.Zpost + (size_t)(k - 1) * w.rows8;
      f.out = w.OUT + (size_t)(k - 1) * w.rows8;
      f.c_in = x.ck[k - 1];
      f.h_in = f.c_in / 2;
      f.log_s_out = log_s[k - 1];
      if (!f.log_s_out) return fail(WG_ERR_INVALID, "null log_s entry");
    }
    if (!f.last) {
      f.Z_w = w.Zpost + (size_t)k * w.rows8;
      f.out_w = w.OUT + (size_t)k * w.rows8;
      f.n_peel = is_early(c, k) ? c.n_early_size : 0;
      f.c_next = x.ck[k];
      f.h_next = f.c_next / 2;
      if (f.c_in - f.n_peel != f.c_next) return fail(WG_ERR_STATE, "flow bookkeeping error");
      f.winv = wt->w1x1[k];
      f.wstart = wt->wstart[k];
      f.bstart = wt->bstart[k];
      f.out_init = wt->out_init[k];
      f.x = w.X + plane_layer(x, k, 0) * w.plane_c;      // flow k's slot (WG_TRAIN_RECOMPUTE: k & 1)
      z_ch += f.n_peel;
    }
    // (measured and dropped: each chain running its own half of the flow step, so that the chains never meet -- they
    //  drift apart and the forward pass took 0.2-1.0 ms longer than with this join per flow)
    TR_TRY(launch_flow(f, s));
    if (f.last) break;
    if ((rc = wn_flow_forward(h, x, wt, k, BNw, w.OUT + (size_t)k * w.rows8, s, sB))) return rc;
  }
  return WG_OK;
}

int wg_train_backward(wg_handle* h, const wg_train_weights* wt, const wg_train_grads* gr, const float* g_z,
                      const float* const* g_log_s, float scale, const void* audio, float* g_mel, float* g_audio,
                      int32_t B, int32_t n_frames, int32_t audio_len, void* workspace, size_t workspace_bytes,
                      int32_t flow_hi, int32_t flow_lo, int32_t flags, void* stream) {
  if (!wt || !audio || !workspace) return fail(WG_ERR_INVALID, "null argument");
  if (!(scale > 0.f)) return fail(WG_ERR_INVALID, "scale must be positive");
  Ctx x;
  int rc = setup(h, B, n_frames, audio_len, workspace, workspace_bytes, flags, x);
  if (rc) return rc;
  if ((rc = check_weights(wt, x.c->n_flows)) || (gr && (rc = check_grads(gr, x.c->n_flows)))) return rc;
  if (g_mel && !wt->wupt) return fail(WG_ERR_INVALID, "g_mel needs wg_train_weights.wupt (packed by wg_train_prepare)");
  // gr == null: no parameter gradients -- the data-gradient chain alone (no weight-gradient launch, slab reduction, start /
  // 1x1 partial, d upsample job; the d spect GEMM only for g_mel)
  const bool pg = gr != nullptr;
  const wg_config& c = *x.c;
  const RowGeom& g = x.g;
  TrainWs& w = x.w;
  hipStream_t s = (hipStream_t)stream;
  BwdPlan p;                                // streams, marks and what orders the reuse of shared buffers: see BwdPlan
  if ((rc = bwd_plan(h, x, wt, gr, scale, s, true, p))) return rc;
  if (flow_lo < 0 || flow_hi >= c.n_flows || flow_lo > flow_hi) return fail(WG_ERR_INVALID, "bad flow range");
  if (x.nl > 10) return fail(WG_ERR_INVALID, "more than 10 layers");
  // channel offsets of the peeled outputs in z (model.py:201-203, :220): early outputs of the flows <= k
  auto early_channels_upto = [&](int k) {
    int n = 0;
    for (int q = 0; q <= k; ++q)
      if (is_early(c, q)) n += c.n_early_size;
    return n;
  };
  int z_final_ch0 = early_channels_upto(flow_hi);
  HIP_TRY(order_after(h, s, p.sW));

  for (int k = flow_hi; k >= flow_lo; --k) {
    const int ck = x.ck[k], hk = ck / 2;
    FlowBwdArgs fb;
    memset(&fb, 0, sizeof fb);
    fb.g = g;
    fb.C = x.C;
    fb.c = ck;
    fb.h = hk;
    fb.scale = scale;
    fb.Zpost = w.Zpost + (size_t)k * w.rows8;
    fb.OUT = w.OUT + (size_t)k * w.rows8;
    fb.g_z = g_z;
    fb.g_log_s = g_log_s ? g_log_s[k] : nullptr;
    fb.from_z = (k == c.n_flows - 1);
    fb.z_ch0 = early_channels_upto(c.n_flows - 1);
    fb.GZ = w.GZ;
    fb.GO = w.GO[k & 1];
    HIP_TRY(wait_on(s, p.w_flow[k & 1]));
    if (x.recompute && k < c.n_flows - 2 && (rc = replay_flow(h, x, wt, k, true, s))) return rc;
    TR_TRY(launch_flow_bwd_pre(fb, s));
    if ((rc = wn_flow_backward(h, x, p, gr, k, fb.GO, fb.GX))) return rc;
    // WG_TRAIN_RECOMPUTE: this flow's share of d spect while its slot still holds its d pre planes -- on sW behind the
    // flow's last weight-gradient job, so that w_flow covers it (without parameter gradients sW is s: behind the chains)
    const bool dspect = x.recompute && (pg || g_mel);
    if (dspect && (rc = dspect_flow(x, wt, k, k == c.n_flows - 1, k == 0, p.sW))) return rc;
    if (pg) HIP_TRY(mark_on(h, p.serial, p.sW, p.w_flow[k & 1], 10 + (k & 1)));
    if (pg && (rc = start_wgrad(x, gr, k, fb.GX, fb.Zpost, p.inv, s))) return rc;
    fb.wstart = wt->wstart[k];
    fb.w1x1 = wt->w1x1[k];
    if (k > 0) {
      fb.Zprev = w.Zpost + (size_t)(k - 1) * w.rows8;
      fb.OUTprev = w.OUT + (size_t)(k - 1) * w.rows8;
      fb.h_prev = x.ck[k - 1] / 2;
      fb.n_peel = is_early(c, k) ? c.n_early_size : 0;
      if (fb.n_peel) z_final_ch0 -= fb.n_peel;
      fb.z_peel_ch0 = z_final_ch0;
    } else {
      fb.audio = (const float*)audio;
      fb.g_audio = g_audio;
    }
    // flow 0 without parameter gradients: the kernel's only outputs would be d W_0 (and d audio)
    if (pg || k > 0 || g_audio) {
      fb.dw_partial = pg ? w.part3 : nullptr;
      TR_TRY(launch_flow_bwd_post(fb, s));
    }
    if (pg) {
      const SlabSeg sg = make_seg(w.part3, flow_bwd_workgroups(g), 64, 64, p.inv, gr->dw1x1[k], 0, 0);
      TR_TRY(launch_slab_reduce_multi(&sg, 1, s));
    }
  }
  // the upsample / mel gradients need the d pre planes of every flow
  if (flow_lo > 0 || !(pg || g_mel)) return join_wgrad_streams(h, p);
  return dspect_finish(h, x, p, wt, gr, g_mel);
}


// ---------------------------------------------------------------------------------------------
// Differentiable synthesis (include/waveglow_amd.h: wg_train_infer_*): WaveGlow.infer (model.py:223-273) on the training
// kernels, with the state that enters every inverse step saved, and its backward w.r.t. mel and the noise.
//   workspace: Zpost[k] = the state y entering inverse step k (step n_flows-1: sigma z_init), OUT[k] = (b | s) of WN_k,
//   X / T / S / A planes of flow k's layers as in the training forward; the backward keeps GP of every layer for d spect.
//   WG_TRAIN_RECOMPUTE: as in the training direction, two flow slots; the forward leaves flows 1 and 0 in them, the
//   backward (ascending) replays flows 2.. into theirs and runs d spect flow by flow.
// ---------------------------------------------------------------------------------------------
namespace {

// common checks and geometry of both calls: audio_len = 256 n_frames (infer's trim, model.py:228).  frames (device, [B], or
// null): the utterances' own frame counts -- every launch of the call takes its padding columns from x.g.frames.
int infer_setup(wg_handle* h, const wg_train_weights* wt, int32_t n_z_early, int32_t B, int32_t n_frames, const int32_t* frames,
                void* workspace, size_t workspace_bytes, int32_t flags, Ctx& x, const float** winv) {
  if (!h) return fail(WG_ERR_INVALID, "null handle");
  const wg_config* c = &h->cfg;
  if (n_frames < 1) return fail(WG_ERR_INVALID, "bad n_frames");
  if (c->n_flows > 64) return fail(WG_ERR_INVALID, "too many flows");
  int rc = setup(h, B, n_frames, n_frames * c->upsample_stride, workspace, workspace_bytes, flags, x);
  if (rc) return rc;
  x.g.frames = (const int*)frames;
  if ((rc = check_weights(wt, c->n_flows))) return rc;
  if (n_z_early != n_early_flows(*c)) return fail(WG_ERR_INVALID, "wrong number of early-noise tensors");
  // W_k^-1: the per-call weights' own (wg_train_prepare inverted them on the device), else the finalised handle's
  for (int k = 0; k < c->n_flows; ++k) {
    if (wt->winv) {
      if (!(winv[k] = wt->winv[k])) return fail(WG_ERR_INVALID, "wg_train_weights.winv has a null per-flow pointer");
    } else if (!(winv[k] = wg_internal_winv(h, k))) {
      return fail(WG_ERR_STATE, "wg_finalize has not been called: the synthesis direction uses the handle's W^-1");
    }
  }
  return WG_OK;
}

// the step's next flow j: its state, WN output and x_0 planes get buffers of their own
void infer_next(const Ctx& x, const wg_train_weights* wt, int j, FlowArgs& f) {
  f.c_next = x.ck[j];
  f.h_next = f.c_next / 2;
  f.wstart = wt->wstart[j];
  f.bstart = wt->bstart[j];
  f.out_init = wt->out_init[j];
  f.Z_w = x.w.Zpost + (size_t)j * x.w.rows8;
  f.out_w = x.w.OUT + (size_t)j * x.w.rows8;
  f.x = x.w.X + plane_layer(x, j, 0) * x.w.plane_c;
  f.skip_x = 0;
  f.a0p = nullptr;
}

}  // namespace

int wg_train_infer_forward(wg_handle* h, const wg_train_weights* wt, const void* mel, const void* z_init,
                           const void* const* z_early, int32_t n_z_early, float sigma, float* audio, int32_t B,
                           int32_t n_frames, const int32_t* frames, int32_t fresh, void* workspace,
                           size_t workspace_bytes, int32_t flags, void* stream) {
  if (!wt || !mel || !z_init || !audio || !workspace || (n_z_early > 0 && !z_early))
    return fail(WG_ERR_INVALID, "null argument");
  Ctx x;
  const float* winv[64];
  int rc = infer_setup(h, wt, n_z_early, B, n_frames, frames, workspace, workspace_bytes, flags, x, winv);
  if (rc) return rc;
  for (int i = 0; i < n_z_early; ++i)
    if (!z_early[i]) return fail(WG_ERR_INVALID, "null early-noise tensor");
  const wg_config& c = *x.c;
  hipStream_t s = (hipStream_t)stream;
  hipStream_t sB;
  if ((rc = second_chain_stream(h, x, s, sB))) return rc;
  const int BNw = fwd_block_n(x);
  // Ragged batch: the planes are cleared on EVERY call, not only on a fresh workspace.  The layer kernels never write a
  // padding column (X, T, S, A in the forward; GP, GXL in the backward), and valid columns read them there -- the dilated
  // taps near an utterance's end, the weight-gradient jobs over every row -- as the zeros of a batch-of-one call: whatever
  // a dense call, or a call with other counts, left in a reused workspace would be read instead.
  if (fresh || frames) TR_TRY(hipMemsetAsync(workspace, 0, x.w.zero_bytes, s));
  if ((rc = spect_planes(x, wt, mel, s))) return rc;
  auto base = [&]() {
    FlowArgs f;
    memset(&f, 0, sizeof f);
    f.direction = 0;
    f.sigma = sigma;
    f.g = x.g;
    f.C = x.C;
    f.io_f16 = 0;
    return f;
  };
  {
    FlowArgs f = base();            // audio = sigma * z_init   (model.py:243-244)
    f.first = 1;
    f.z_extra = z_init;
    infer_next(x, wt, c.n_flows - 1, f);
    TR_TRY(launch_flow(f, s));
  }
  int ze = 0;
  for (int k = c.n_flows - 1; k >= 0; --k) {
    if ((rc = wn_flow_forward(h, x, wt, k, BNw, x.w.OUT + (size_t)k * x.w.rows8, s, sB))) return rc;
    // inverse coupling, W_k^-1, early noise in front   (model.py:253-271); the input state stays in Zpost[k]
    FlowArgs f = base();
    f.Z = x.w.Zpost + (size_t)k * x.w.rows8;
    f.out = x.w.OUT + (size_t)k * x.w.rows8;
    f.c_in = x.ck[k];
    f.h_in = f.c_in / 2;
    f.winv = winv[k];
    if (is_early(c, k)) {
      f.z_extra = z_early[ze++];
      f.n_extra = c.n_early_size;
    }
    const int c_next = f.c_in + f.n_extra;
    f.last = (k == 0);
    if (f.last) {
      if (c_next != c.n_group) return fail(WG_ERR_STATE, "flow bookkeeping error");
      f.c_next = c_next;
      f.audio_out = audio;
    } else {
      if (x.ck[k - 1] != c_next) return fail(WG_ERR_STATE, "flow bookkeeping error");
      infer_next(x, wt, k - 1, f);
    }
    TR_TRY(launch_flow(f, s));
  }
  return WG_OK;
}

int wg_train_infer_backward(wg_handle* h, const wg_train_weights* wt, const wg_train_grads* gr, const float* g_audio,
                            float scale, float sigma, float* g_mel, float* g_z_init, float* const* g_z_early,
                            int32_t n_z_early, int32_t B, int32_t n_frames, const int32_t* frames, void* workspace,
                            size_t workspace_bytes, int32_t flags, void* stream) {
  if (!wt || !g_audio || !workspace) return fail(WG_ERR_INVALID, "null argument");
  if (!(scale > 0.f)) return fail(WG_ERR_INVALID, "scale must be positive");
  Ctx x;
  const float* winv[64];
  int rc = infer_setup(h, wt, n_z_early, B, n_frames, frames, workspace, workspace_bytes, flags, x, winv);
  if (rc) return rc;
  if (g_mel && !wt->wupt) return fail(WG_ERR_INVALID, "g_mel needs wg_train_weights.wupt (packed by wg_train_prepare)");
  // gr == null: the data-gradient chain alone.  Otherwise the packed weight gradients as well, flow by flow behind the data
  // gradients they are made of: per layer the training direction's weight-gradient launch and slab reduction (layer_wgrad),
  // per flow d start (the saved state Y is the WN input, as Zpost is in the training direction), d out_init and d W_k of the
  // inverse 1x1, after the last flow d upsample.
  const bool pg = gr != nullptr;
  if (pg && (rc = check_grads(gr, x.c->n_flows))) return rc;
  const wg_config& c = *x.c;
  const RowGeom& g = x.g;
  TrainWs& w = x.w;
  hipStream_t s = (hipStream_t)stream;
  BwdPlan p;                                // one chain on `s`; streams, marks and buffer reuse: see BwdPlan
  if ((rc = bwd_plan(h, x, wt, gr, scale, s, false, p))) return rc;
  if (pg && x.nl > 10) return fail(WG_ERR_INVALID, "more than 10 layers");
  HIP_TRY(order_after(h, s, p.sW));
  // index in z_early (descending flow order) of early flow k
  auto early_index = [&](int k) {
    int n = 0;
    for (int q = c.n_flows - 1; q > k; --q) n += is_early(c, q);
    return n;
  };
  // Ascending flow order: the gradient enters at the audio, the output of inverse step 0.
  for (int k = 0; k < c.n_flows; ++k) {
    const int ck = x.ck[k];
    HIP_TRY(wait_on(s, p.w_flow[k & 1]));
    if (x.recompute && k >= 2 && (rc = replay_flow(h, x, wt, k, false, s))) return rc;
    InvBwdArgs ib;
    memset(&ib, 0, sizeof ib);
    ib.g = g;
    ib.C = x.C;
    ib.c = ck;
    ib.h = ck / 2;
    ib.scale = scale;
    ib.sigma = sigma;
    ib.Y = w.Zpost + (size_t)k * w.rows8;
    ib.OUT = w.OUT + (size_t)k * w.rows8;
    ib.winv = winv[k];
    ib.g_audio = k == 0 ? g_audio : nullptr;
    ib.GZ = w.GZ;
    ib.GO = w.GO[k & 1];
    if (pg) {
      // d W_k = - sum g_v (x) w, from the step's incoming gradient: before the pre kernel overwrites GZ in place
      InvDwArgs dw;
      memset(&dw, 0, sizeof dw);
      dw.g = g;
      dw.c = ck;
      dw.h = ck / 2;
      dw.scale = scale;
      dw.Y = ib.Y;
      dw.OUT = ib.OUT;
      dw.winv = ib.winv;
      dw.g_audio = ib.g_audio;
      dw.GZ = w.GZ;
      dw.partial = w.part3;
      TR_TRY(launch_inv_dw1x1(dw, s));
      const SlabSeg sg = make_seg(w.part3, flow_bwd_workgroups(g), 64, 64, p.inv, gr->dw1x1[k], 0, 0);
      TR_TRY(launch_slab_reduce_multi(&sg, 1, s));
    }
    TR_TRY(launch_inv_bwd_pre(ib, s));
    if ((rc = wn_flow_backward(h, x, p, gr, k, ib.GO, ib.GX))) return rc;
    ib.wstart = wt->wstart[k];
    ib.last = (k == c.n_flows - 1);
    if (ib.last) {
      ib.g_z_init = g_z_init;
    } else if (is_early(c, k + 1)) {
      ib.n_peel = c.n_early_size;
      ib.g_peel = g_z_early ? g_z_early[early_index(k + 1)] : nullptr;
    }
    // WG_TRAIN_RECOMPUTE: this flow's share of d spect before the slot is replayed for flow k+2 -- with parameter gradients
    // on sW behind the flow's last weight-gradient job, so that w_flow covers it; otherwise on s behind the post kernel
    const bool dspect = x.recompute && (g_mel || pg);
    if (dspect && pg && (rc = dspect_flow(x, wt, k, k == 0, k == c.n_flows - 1, p.sW))) return rc;
    if (pg) HIP_TRY(mark_on(h, p.serial, p.sW, p.w_flow[k & 1], 10 + (k & 1)));
    if (pg && (rc = start_wgrad(x, gr, k, ib.GX, ib.Y, p.inv, s))) return rc;
    TR_TRY(launch_inv_bwd_post(ib, s));
    if (dspect && !pg && (rc = dspect_flow(x, wt, k, k == 0, k == c.n_flows - 1, s))) return rc;
  }
  if (!g_mel && !pg) return WG_OK;
  return dspect_finish(h, x, p, wt, gr, g_mel);
}

}  // extern "C"

// ---------------------------------------------------------------------------------------------
// Training plumbing on the device (train_prep.hip): parameters in their own tensors -> wg_train_weights, packed gradients ->
// one gradient per parameter.
// ---------------------------------------------------------------------------------------------
namespace {

struct ParamDesc { int sec, idx; long long numel; std::string name; };

// canonical parameter list: section-major (wg_train.h: PrepSec), g sections only for weight-normed modules
std::vector<ParamDesc> param_list(const wg_config& c, const int* ck, bool wn) {
  std::vector<ParamDesc> out;
  const int C = c.n_channels, nl = c.n_layers, nf = c.n_flows, M = c.n_mel_channels, M8 = 8 * M, FL = nf * nl;
  auto wname = [&](const std::string& mod, int which) {     // 0: v / dense weight, 1: g
    if (!wn) return mod + ".weight";
    return mod + (which ? ".parametrizations.weight.original0" : ".parametrizations.weight.original1");
  };
  for (int sec = 0; sec <= SEC_UP_B; ++sec) {
    const bool is_g = sec == SEC_IN_G || sec == SEC_RS_G || sec == SEC_CO_G || sec == SEC_ST_G;
    if (is_g && !wn) continue;
    const int n = prep_sec_len(FL, nf, sec);
    for (int q = 0; q < n; ++q) {
      ParamDesc d;
      d.sec = sec;
      d.idx = q;
      const int k = sec <= SEC_RS_B ? q / nl : q, i = sec <= SEC_RS_B ? q % nl : 0, h = ck[k < nf ? k : 0] / 2;
      const std::string wnp = "WN." + std::to_string(k) + ".";
      const std::string in = wnp + "in_layers." + std::to_string(i), rs = wnp + "res_skip_layers." + std::to_string(i);
      const long long rs_rows = i < nl - 1 ? 2 * C : C;
      switch (sec) {
        case SEC_IN_V: d.name = wname(in, 0); d.numel = (long long)2 * C * C * 3; break;
        case SEC_IN_G: d.name = wname(in, 1); d.numel = 2 * C; break;
        case SEC_IN_B: d.name = in + ".bias"; d.numel = 2 * C; break;
        case SEC_RS_V: d.name = wname(rs, 0); d.numel = rs_rows * C; break;
        case SEC_RS_G: d.name = wname(rs, 1); d.numel = rs_rows; break;
        case SEC_RS_B: d.name = rs + ".bias"; d.numel = rs_rows; break;
        case SEC_CO_V: d.name = wname(wnp + "cond_layer", 0); d.numel = (long long)2 * C * nl * M8; break;
        case SEC_CO_G: d.name = wname(wnp + "cond_layer", 1); d.numel = (long long)2 * C * nl; break;
        case SEC_CO_B: d.name = wnp + "cond_layer.bias"; d.numel = (long long)2 * C * nl; break;
        case SEC_ST_V: d.name = wname(wnp + "start", 0); d.numel = (long long)C * h; break;
        case SEC_ST_G: d.name = wname(wnp + "start", 1); d.numel = C; break;
        case SEC_ST_B: d.name = wnp + "start.bias"; d.numel = C; break;
        case SEC_EN_W: d.name = wnp + "end.weight"; d.numel = (long long)2 * h * C; break;
        case SEC_EN_B: d.name = wnp + "end.bias"; d.numel = 2 * h; break;
        case SEC_CV_W: d.name = "convinv." + std::to_string(k) + ".conv.weight"; d.numel = (long long)ck[k] * ck[k]; break;
        case SEC_UP_W: d.name = "upsample.weight"; d.numel = (long long)M * M * c.upsample_kernel; break;
        default: d.name = "upsample.bias"; d.numel = M; break;
      }
      out.push_back(d);
    }
  }
  return out;
}

struct PrepLayout {
  size_t tab, goff, s_in, s_co, s_rs, s_st, wend8, bsum, wes, bytes;
  int n_slots, n_scale[4];
};
PrepLayout prep_layout(const wg_config& c) {
  PrepLayout L;
  const int C = c.n_channels, nl = c.n_layers, nf = c.n_flows, FL = nf * nl;
  L.n_slots = prep_slot_n(FL, nf, SEC_COUNT, 0);
  L.n_scale[0] = FL * 2 * C; L.n_scale[1] = nf * 2 * C * nl; L.n_scale[2] = FL * 2 * C; L.n_scale[3] = nf * C;
  size_t off = 0;
  auto take = [&](size_t bytes) { const size_t o = off; off += align_up(bytes); return o; };
  L.tab = take((size_t)L.n_slots * sizeof(void*));
  L.goff = take((size_t)L.n_slots * sizeof(long long));
  L.s_in = take((size_t)2 * L.n_scale[0] * 4);
  L.s_co = take((size_t)2 * L.n_scale[1] * 4);
  L.s_rs = take((size_t)2 * L.n_scale[2] * 4);
  L.s_st = take((size_t)2 * L.n_scale[3] * 4);
  L.wend8 = take((size_t)nf * 8 * C * 4);
  L.bsum = take((size_t)nf * C * 4);
  L.wes = take((size_t)FL * 8 * C * 4);
  L.bytes = off;
  return L;
}

// fills the argument block and uploads the pointer table (parameters + the per-flow buffers of `wt` / `gr`)
int prep_args(wg_handle* h, const void* const* params, int weight_normed, const wg_train_weights* wt, const wg_train_grads* gr,
              void* aux, size_t aux_bytes, float* flat, hipStream_t s, PrepArgs& a) {
  if (!h || !params || !aux) return fail(WG_ERR_INVALID, "null argument");
  const wg_config& c = h->cfg;
  const int* ck = h->c_k.data();
  if (c.n_flows > kPrepMaxFlows) return fail(WG_ERR_INVALID, "more than 32 flows are not supported by the training direction");
  if (c.upsample_kernel != 1024) return fail(WG_ERR_INVALID, "upsample kernel must be 1024");
  const PrepLayout L = prep_layout(c);
  if (aux_bytes < L.bytes) return fail(WG_ERR_WORKSPACE, "wg_train_prepare: aux buffer too small");
  const int nf = c.n_flows, FL = nf * c.n_layers;
  std::vector<void*> tab((size_t)L.n_slots, nullptr);
  std::vector<long long> goff((size_t)L.n_slots, 0);
  const std::vector<ParamDesc> pl = param_list(c, ck, weight_normed != 0);
  long long off = 0;
  for (size_t i = 0; i < pl.size(); ++i) {
    if (!params[i]) return fail(WG_ERR_INVALID, "null parameter pointer: %s", pl[i].name.c_str());
    const int slot = prep_slot_n(FL, nf, pl[i].sec, pl[i].idx);
    tab[slot] = const_cast<void*>(params[i]);
    goff[slot] = off;
    off += pl[i].numel;
  }
  for (int k = 0; k < nf; ++k) {
    if (wt) {
      tab[prep_slot_n(FL, nf, SEC_O_WSTART, k)] = const_cast<float*>(wt->wstart[k]);
      tab[prep_slot_n(FL, nf, SEC_O_BSTART, k)] = const_cast<float*>(wt->bstart[k]);
      tab[prep_slot_n(FL, nf, SEC_O_OINIT, k)] = const_cast<float*>(wt->out_init[k]);
      tab[prep_slot_n(FL, nf, SEC_O_W1X1, k)] = const_cast<float*>(wt->w1x1[k]);
      if (wt->winv) tab[prep_slot_n(FL, nf, SEC_O_WINV, k)] = const_cast<float*>(wt->winv[k]);
    }
    if (gr) {
      tab[prep_slot_n(FL, nf, SEC_G_DSTART, k)] = gr->dstart[k];
      tab[prep_slot_n(FL, nf, SEC_G_DOINIT, k)] = gr->dout_init[k];
      tab[prep_slot_n(FL, nf, SEC_G_DW1X1, k)] = gr->dw1x1[k];
    }
  }
  char* base = (char*)aux;
  // (through the handle's pinned staging buffers: `tab` / `goff` die with this call, the copies run later on the stream)
  TR_TRY(wg_internal_upload(h, base + L.tab, tab.data(), tab.size() * sizeof(void*), s));
  TR_TRY(wg_internal_upload(h, base + L.goff, goff.data(), goff.size() * sizeof(long long), s));
  memset(&a, 0, sizeof a);
  a.tab = (void* const*)(base + L.tab);
  a.goff = (const long long*)(base + L.goff);
  a.flat = flat;
  a.s_in = (float*)(base + L.s_in); a.s_co = (float*)(base + L.s_co); a.s_rs = (float*)(base + L.s_rs); a.s_st = (float*)(base + L.s_st);
  a.wend8 = (float*)(base + L.wend8); a.bsum = (float*)(base + L.bsum); a.wes = (float*)(base + L.wes);
  a.C = c.n_channels; a.M8 = c.n_mel_channels * 8; a.nl = c.n_layers; a.nf = nf; a.FL = FL;
  for (int k = 0; k < nf; ++k) { a.ck[k] = ck[k]; a.hk[k] = ck[k] / 2; }
  for (int q = 0; q < 4; ++q) a.n_scale[q] = L.n_scale[q];
  if (wt) { a.b1 = const_cast<float*>(wt->b1); a.b2 = const_cast<float*>(wt->b2); a.bup = const_cast<float*>(wt->bup); }
  a.want_winv = wt && wt->winv;
  if (gr) {
    a.dw1 = gr->dw1; a.db1 = gr->db1; a.dw2 = gr->dw2; a.db2 = gr->db2; a.dwes = gr->dwes; a.dwup = gr->dwup; a.dbup = gr->dbup;
    a.layer_stride = gr->layer_stride; a.flow_stride = gr->flow_stride;
  }
  return WG_OK;
}

}  // namespace

extern "C" {

int32_t wg_train_param_count(const wg_handle* h, int32_t weight_normed) {
  if (!h) return 0;
  return (int32_t)param_list(h->cfg, h->c_k.data(), weight_normed != 0).size();
}

const char* wg_train_param_name(const wg_handle* h, int32_t weight_normed, int32_t i) {
  static thread_local std::string name;
  if (!h) return "";
  const std::vector<ParamDesc> pl = param_list(h->cfg, h->c_k.data(), weight_normed != 0);
  if (i < 0 || (size_t)i >= pl.size()) return "";
  name = pl[i].name;
  return name.c_str();
}

int64_t wg_train_param_numel(const wg_handle* h, int32_t weight_normed, int32_t i) {
  if (!h) return 0;
  const std::vector<ParamDesc> pl = param_list(h->cfg, h->c_k.data(), weight_normed != 0);
  return (i < 0 || (size_t)i >= pl.size()) ? 0 : pl[i].numel;
}

size_t wg_train_prepare_bytes(const wg_handle* h) { return h ? prep_layout(h->cfg).bytes : 0; }

int wg_train_prepare(wg_handle* h, const void* const* params, int32_t weight_normed, const wg_train_weights* out, void* aux,
                     size_t aux_bytes, void* stream) {
  if (!out) return fail(WG_ERR_INVALID, "null argument");
  if (!out->a1 || !out->a1c || !out->b1 || !out->a2 || !out->b2 || !out->es || !out->wat || !out->wbt || !out->wct || !out->wup ||
      !out->bup || !out->wstart || !out->bstart || !out->out_init || !out->w1x1)
    return fail(WG_ERR_INVALID, "wg_train_prepare: wg_train_weights has a null member");
  if (out->winv && h)
    for (int k = 0; k < h->cfg.n_flows; ++k)
      if (!out->winv[k]) return fail(WG_ERR_INVALID, "wg_train_prepare: wg_train_weights.winv has a null per-flow pointer");
  hipStream_t s = (hipStream_t)stream;
  PrepArgs pa;
  int rc = prep_args(h, params, weight_normed, out, nullptr, aux, aux_bytes, nullptr, s, pa);
  if (rc) return rc;
  TR_TRY(launch_prepare(pa, s));
  const wg_config& c = h->cfg;
  const int C = c.n_channels, M8 = c.n_mel_channels * 8, FL = c.n_flows * c.n_layers, NW = wn_waves(C);
  if (NW <= 0 || M8 % 64) return fail(WG_ERR_INVALID, "wg_train_prepare: unsupported channel counts");
  const size_t K1 = 3 * (size_t)C + M8;
  PackArgs a;
  memset(&a, 0, sizeof a);
  a.C = C; a.M8 = M8; a.FL = FL; a.NW = NW;
  a.prep = pa;
  a.wes = pa.wes;
  auto run = [&](int kind, const void* dst, const void* dst2, size_t elements) -> hipError_t {
    a.kind = kind;
    a.dst = (_Float16*)const_cast<void*>(dst);
    a.dst2 = (_Float16*)const_cast<void*>(dst2);
    a.n_pieces = elements / 8;
    return launch_pack(a, s);
  };
  TR_TRY(run(PACK_A1, out->a1, out->a1c, (size_t)FL * 2 * C * K1));
  TR_TRY(run(PACK_A2, out->a2, nullptr, (size_t)FL * C * C));
  TR_TRY(run(PACK_ES, out->es, nullptr, (size_t)FL * 16 * C));
  TR_TRY(run(PACK_WAT, out->wat, nullptr, (size_t)FL * C * (C + 64)));
  TR_TRY(run(PACK_WBT, out->wbt, nullptr, (size_t)FL * C * 6 * C));
  TR_TRY(run(PACK_WCT, out->wct, nullptr, (size_t)M8 * FL * 2 * C));
  TR_TRY(run(PACK_WUP, out->wup, nullptr, (size_t)32 * M8 * 512));
  if (out->wupt) TR_TRY(run(PACK_WUPT, out->wupt, nullptr, (size_t)32 * 4 * M8 * wupt_blocks(M8) * 32));
  return WG_OK;
}

int wg_train_param_grads(wg_handle* h, const void* const* params, int32_t weight_normed, const wg_train_grads* grads, void* aux,
                         size_t aux_bytes, float* flat, void* stream) {
  if (!grads || !flat) return fail(WG_ERR_INVALID, "null argument");
  int rc = check_grads(grads, h ? h->cfg.n_flows : 0);
  if (rc) return rc;
  PrepArgs pa;
  rc = prep_args(h, params, weight_normed, nullptr, grads, aux, aux_bytes, flat, (hipStream_t)stream, pa);
  if (rc) return rc;
  TR_TRY(launch_param_grads(pa, (hipStream_t)stream));
  return WG_OK;
}

}  // extern "C"
