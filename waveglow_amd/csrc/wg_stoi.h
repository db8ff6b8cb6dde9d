// Constants and launch entry point of stoi.hip, shared with stoi_api.cpp (host).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace wg {

constexpr int kStoiW = 256;             // frame
constexpr int kStoiH = 128;             // hop
constexpr int kStoiNfft = 512;
constexpr int kStoiBands = 15;
constexpr int kStoiSeg = 30;            // frames of a segment
constexpr int kStoiBinLo = 7;           // the bins the bands of the definition reach: 7 .. 218
constexpr int kStoiBins = 212;
constexpr int kStoiRow = 8;             // fp64 values per pair
constexpr int kStoiMaxPitch = 1 << 21;  // samples per row
constexpr int kStoiFrameTile = 8;       // frames one workgroup of stoi_bands_kernel transforms
constexpr int kStoiSegTile = 4;         // segments one workgroup of stoi_segment_kernel correlates, one per wave

// F0(n) of include/waveglow_amd.h (wg_stoi): the starts are range(0, n - W, H)
__host__ __device__ inline int stoi_frames(int n) { return n > kStoiW ? (n - kStoiW + kStoiH - 1) / kStoiH : 0; }

// Workspace parts of one call (elements, not bytes): everything is sized for rows of `pitch` samples.
struct StoiGeom {
  int B, pitch;
  int F0max;        // max(1, F0(pitch)): frame energies and kept-frame lists per utterance
  int Fmax;         // max(1, F0max - 1): band frames per utterance and signal
  int Jmax;         // max(1, Fmax - 29): segments per utterance
};

inline StoiGeom stoi_geom(int B, int pitch) {
  StoiGeom g;
  g.B = B, g.pitch = pitch;
  const int f0 = stoi_frames(pitch);
  g.F0max = f0 < 1 ? 1 : f0;
  g.Fmax = g.F0max - 1 < 1 ? 1 : g.F0max - 1;
  g.Jmax = g.Fmax - (kStoiSeg - 1) < 1 ? 1 : g.Fmax - (kStoiSeg - 1);
  return g;
}

struct StoiBuffers {
  double* energy;   // [B][F0max]
  int* kept;        // [B][F0max] indices of the kept frames, ascending
  int* counts;      // [B][4]: n, F0, K, J
  double* bands;    // [B][2][15][Fmax]: X then Y
  double* seg;      // [B][Jmax][2]: the STOI and ESTOI sums of one segment
};

hipError_t launch_stoi(const float* x, const int* len_x, const float* y, const int* len_y, const double* window,
                       const int* bands, const double* cossin, double* rows, const StoiGeom& g, const StoiBuffers& w,
                       hipStream_t s);

// Scratch of one backward call (stoi_grad.hip), sized like the forward's parts.
struct StoiGradBuffers {
  int* inv;         // [B][F0max]: silence-free index of an original frame, -1 where it was gated
  double* blocks;   // [B][Jmax][15][30]: one segment's gradient with respect to its block of Y
  double* dband;    // [B][15][Fmax]: gradient with respect to the band sums (the squares of Y)
  double* dframe;   // [B][Fmax][256]: gradient with respect to the silence-free signal through one of its frames
};

// `saved` holds the counts, kept and bands parts a forward left; y [B][pitch], g_rows [B][2] -> d_y [B][pitch] fp64
hipError_t launch_stoi_backward(const float* y, const double* window, const int* bands, const double* cossin,
                                const double* g_rows, const StoiBuffers& saved, double* d_y, const StoiGeom& g,
                                const StoiGradBuffers& w, hipStream_t s);

}  // namespace wg
