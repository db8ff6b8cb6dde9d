// Constants and launch entry points of likelihood.hip, shared with likelihood_api.cpp (host).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace wg {

constexpr int kNllRow = 8;          // fp64 values per utterance: nll, bits/sample, sum z^2, sum log_s, log_det, samples, z mean, z var
constexpr int kNllPart = 3;         // fp64 partials per (utterance, frame): sum z^2, sum log_s, sum z
constexpr int kNllFrameCols = 32;   // columns (group-timesteps) of one mel frame: upsample_stride / n_group
constexpr int kNllMaxPlanes = 16;   // log_s planes one launch of the frame kernel takes by value

// log_s planes of up to kNllMaxPlanes consecutive flows: p[i] is [B][h[i]][L] fp32
struct NllPlanes {
  const float* p[kNllMaxPlanes];
  int h[kNllMaxPlanes];
  int n;
};

// One launch of the frame kernel: partials [B][NF][kNllPart] of z (when `z` is not null: the first launch of a call, which
// writes the partials) and of the planes in `pl` in order (a later launch adds to the partials).  NF = ceil(L / 32).
// frame_out (or null): [B][NF] fp64, written by the launch that has `last` set.
hipError_t launch_nll_frames(const float* z, const NllPlanes& pl, const int* frames, int B, int L, int n_frames_max,
                             double inv_2s2, double logdet_sum, int last, double* part, double* frame_out, hipStream_t s);
// One workgroup per utterance: the frames of its partials in a fixed order, then the row.
hipError_t launch_nll_rows(const double* part, const int* frames, int B, int L, int n_frames_max, double inv_2s2,
                           double half_log_2pis2, double logdet_sum, double* rows, hipStream_t s);

}  // namespace wg
