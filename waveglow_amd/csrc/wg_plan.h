// Which WN-layer kernel variant a call runs: the one place that decides.  Pure host arithmetic -- no HIP call and no getenv in
// here: the callers (api.cpp run_wn, kernels.hip launch_wn_tt / launch_wn_ttt, train_api.cpp setup / fwd_block_n) read the
// device's CU count and the test switches and pass them in, and wg_plan (api.cpp, include/waveglow_amd.h) reports the same
// functions' answers without a handle or a GPU.  Every threshold below appears here and nowhere else.
#pragma once
#include <stdint.h>

namespace wg {

constexpr int kPhases = 32;           // phase blocks of the activation planes (wg_common.h RowGeom): tiles = 32 * Rp / BN

// Cross-tile prefetch inside a workgroup: see the tile loop of wn_layer_kernel.
// (The next tile's A fragments are NOT prefetched under the epilogue: between such an inline-asm load and its
// wait lies a long stretch of compiler-scheduled code, and hipcc moved the still-in-flight destination registers
// there -- wrong results.  They are loaded at the tile top: ~1 L2 latency exposed per tile.)
constexpr int kTilesPerWG = 2;        // tiles per workgroup (template TPW), fully unrolled; 1 for small workloads;
                                      // the unrolled group of the resident tile walk (template RESIDENT)

// columns (group-timesteps) per workgroup of the widest tile a channel count has (WnCfg<C>::BN)
constexpr int plan_default_bn(int C) { return C >= 512 ? 64 : 128; }

// The test switches, as values.  Defaults = nothing set.
struct PlanSwitches {
  int force_bn = 0;        // WG_FORCE_BN: 64 | 128 pins the tile width (128 only where the channel count has it)
  int resident = -1;       // WG_RESIDENT: -1 unset; 0 = never the resident walk; N > 0 = the walk with 8 ceil(N / 8) workgroups
  bool disable_deep = false;   // WG_DISABLE_DEEP=1: the one-step ring instead of the two-step-deep prefetch kernel
  int train_halves = 0;    // WG_TRAIN_HALVES: 1 never, 2 always (even batches), otherwise by shape
};

// ---- tile width of inference and the no-grad forward (api.cpp run_wn)
// Small workloads: 64-column tiles double the workgroup count when 128-column tiles would leave CUs idle -- when that
// buys whole rounds.  A 64-column tile takes ~0.6 of a 128-column tile's time (measured at 256 channels: 22.7 vs 38.5 us
// for a one-round launch), so compare rounds x tile time: 128 tiles on 256 CUs -> 64-column tiles fill the chip in one
// round (configs[0]); 224 tiles -> two rounds of 64-column tiles lose to one round of 128-column ones (+18 % at 1 x 80x864).
inline int plan_infer_bn(int C, int Rp, int n_cu, int force_bn) {
  int BN = plan_default_bn(C);
  if (BN == 128) {
    const int64_t t128 = (int64_t)kPhases * (Rp / 128), ncu = n_cu > 0 ? n_cu : 1;
    const int64_t r128 = (t128 + ncu - 1) / ncu, r64 = (2 * t128 + ncu - 1) / ncu;
    if (t128 < 4 * ncu && 6 * r64 < 10 * r128) BN = 64;
  }
  if (BN == 128 && force_bn == 64) BN = 64;
  if (force_bn == 128 && plan_default_bn(C) == 128) BN = 128;
  return BN;
}

// ---- tile width of the fused layer kernel in the training forward and the gradient paths (train_api.cpp fwd_block_n):
// 64 columns below one 128-column tile per CU
inline int plan_train_bn(int C, int Rp, int n_cu, int force_bn) {
  int BN = plan_default_bn(C);
  if (BN == 128 && (int64_t)kPhases * (Rp / 128) < (int64_t)n_cu) BN = 64;
  if (force_bn == 64 || (force_bn == 128 && plan_default_bn(C) == 128)) BN = force_bn;
  return BN;
}

// ---- the two half-batch chains of the training direction (train_api.cpp setup).
// A WN-layer launch runs ceil(tiles / CUs) rounds and the next layer waits for its last, partly filled
// round (config 4: 576 tiles of 128 columns on 256 CUs = 2.25 rounds, a quarter of the chip-time idle).  The two
// halves of the batch never exchange data inside a WN, so they run as two chains of half-size launches on two
// streams and fill each other's idle CUs.  That needs the first B/2 utterances to end on a tile boundary: the rows
// per utterance Fp are padded up (71 -> 72 at config 4: 16 x 72 = 9 tiles, the same 2304 rows per phase as before).
// Returns 1 or 2; with 2, fp / rp are the padded rows per utterance and per phase block (otherwise Fp / Rp).
inline int plan_train_halves(int B, int Fp, int Rp, int n_cu, int want, int& fp, int& rp) {
  fp = Fp;
  rp = Rp;
  if (B % 2 != 0 || want == 1) return 1;
  int f = Fp;
  while ((B / 2 * f) % 128) ++f;
  const int r = B * f;
  const long long tiles = (long long)kPhases * (Rp / 128);
  const long long idle = (tiles + n_cu - 1) / n_cu * n_cu - tiles;
  const bool helps = tiles > n_cu && idle * 10 >= tiles && r <= Rp + Rp / 32;
  if (want != 2 && !helps) return 1;
  fp = f;
  rp = r;
  return 2;
}

// ---- launch form of one inference / no-grad-forward layer (kernels.hip launch_wn_tt, launch_wn_ttt)
enum PlanForm { kPlanSingle = 0, kPlanPair = 1, kPlanResident = 2 };
struct WnLaunchPlan {
  int form;            // PlanForm
  int resident_wgs;    // kPlanResident: workgroups per XCD label (the grid is 8 x this); otherwise 0
  bool deep;           // the two-step-deep weight prefetch kernel (DEEP)
};

// the DEEP kernel exists for this tile shape only: 256 channels, 64 columns, one tile per workgroup
constexpr bool plan_deep_shape(int C, int BN, int tiles_per_wg) { return C == 256 && BN == 64 && tiles_per_wg == 1; }

inline WnLaunchPlan plan_wn_launch(int C, int BN, int n_tiles, int n_cu, int n_cond_steps, const PlanSwitches& sw) {
  const int ncu = n_cu > 0 ? n_cu : 1;
  WnLaunchPlan p = {kPlanSingle, 0, false};
  // Resident tile walk where a CU has at least two tiles to walk: at most one workgroup per CU, each walking its share of its
  // XCD label's run tile by tile, so the workgroup start (dispatch, bias / end x skip staging, a cold first B tile) is paid
  // once per CU and launch instead of once per pair, and every tile seam has the B-tile prefetch.  The workgroups do not
  // communicate: nothing depends on their being co-resident or on the block -> XCD mapping (speed only, as above).
  // WG_RESIDENT (read per launch, tests only): 0 = the launches below; N > 0 = the resident launch with 8 ceil(N / 8)
  // workgroups whatever the size.  The two must agree bit for bit.
  {
    const int per_label_tiles = (n_tiles + 7) / 8;
    int wgs = 0;
    if (sw.resident > 0) wgs = (sw.resident + 7) / 8;
    // Not with a sparse tail: the walk is static, so n_tiles mod CUs workgroups run the last tile-round alone after every CU
    // has run all the full ones, where the dispatcher spreads today's pairs over that tail.  Measured at 6 x 80x864 (1312
    // tiles on 256 CUs = 5.125 rounds): +2.4 %, outside both spreads; the next sparsest tail measured, 0.375 of a round,
    // gains.  The quarter lies between the two.  (Too wide at many rounds: at 13 x 80x864, 11.125 rounds, the walk would
    // gain 1.3 % -- DESIGN.md section 8.)
    // By default only where the walk was measured against today's launches: 256 channels on 128-column tiles.  Every other
    // width keeps today's launch -- in particular 64-column tiles at 256 channels, which plan_infer_bn picks for 514 .. 768
    // narrow tiles on 256 CUs (2 .. 3 tiles per CU) and which run the two-step-deep prefetch kernel (DEEP, single tiles):
    // the walk has no DEEP form and would trade that kernel's ~10 % of a launch for its own 1 - 1.5 %.
    else if (sw.resident < 0 && C == 256 && BN == 128 && n_tiles >= 2 * ncu && !(n_tiles % ncu > 0 && 4 * (n_tiles % ncu) < ncu)) {
      const int by_tiles = (per_label_tiles + kTilesPerWG - 1) / kTilesPerWG, by_cus = (ncu + 7) / 8;
      wgs = by_tiles < by_cus ? by_tiles : by_cus;
    }
    if (wgs > 0) {
      p.form = kPlanResident;
      p.resident_wgs = wgs;
      return p;
    }
  }
  // Below two tiles per CU (and under WG_RESIDENT=0): workgroups that end after one or two tiles.  Two tiles per workgroup
  // amortise the launch and prefetch across the tile seam, but need >= 2 tiles per CU -- and must not cost a round: 1120 tiles
  // on 256 CUs are 5 rounds of single tiles but 3 rounds of pairs = 6 tile times (batch 5 x 80x864)
  const int rounds1 = (n_tiles + ncu - 1) / ncu;
  const int rounds2 = ((n_tiles + kTilesPerWG - 1) / kTilesPerWG + ncu - 1) / ncu * kTilesPerWG;
  if (n_tiles >= 2 * kTilesPerWG * ncu && rounds2 <= rounds1) {
    p.form = kPlanPair;
    return p;
  }
  // small workloads (one tile per workgroup, 64 columns) at 256 channels / 80 mel channels: two-step-deep weight prefetch.
  // WG_DISABLE_DEEP=1 (read per launch, tests only) takes the one-step ring instead: the two must agree bit for bit.
  p.deep = plan_deep_shape(C, BN, 1) && n_cond_steps == 5 && !sw.disable_deep;
  return p;
}

}  // namespace wg
