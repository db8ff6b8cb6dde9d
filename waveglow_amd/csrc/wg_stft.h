// Kernel argument blocks, geometry and launch entry points of stft.hip, shared with stft_api.cpp (host).
// The argument blocks are passed to the kernels by value: both sides must see ONE definition.
#pragma once
#include <hip/hip_runtime.h>

namespace wg {

// Fixed geometry: filter 1024, hop 256 (TSTFTHParams defaults, taco_stft.py:36-43).
constexpr int kFL = 1024, kHop = 256, kCut = 513;
constexpr int kRows = 1056;            // 2*513 = 1026 interleaved (re_k, im_k) rows, padded to 33 tiles of 32

struct StftArgs {
  const float* audio;      // [B][N]
  const float* fwdA;       // packed A fragments [33 mtile][512 kstep][64 lanes]
  const float* bias;       // [513] magnitude to subtract (device) or null
  float strength;
  float* rec;              // [B][1056][Fs]   Fs = 3 + Fpad (3 zero lead columns), recombined spectrum
  float* mag0;             // optional [B][513]: magnitude of frame 0
  int N, F, Fs;
  float* mag;              // optional [B][513][F]: all magnitudes (mel front-end); rec may then be null
  const int* lens;         // ragged batch: device [B] sample counts (N is then the row pitch, F the frames of N) or null
  int min_len, len_mask;   // ragged batch: a length < min_len, > N or with (length & len_mask) != 0 counts as 0
  float* raw;              // stft_kernel<true> only: [B][1056][Fs] (re, im) before the denoiser epilogue, cells of rec
};
struct MelArgs {
  const float* mag;        // [B][513][F]
  const float* basis;      // [n_mel][513]  Slaney mel filterbank (taco_stft.py:66-73)
  float* mel;              // [B][n_mel][F]  log(clamp(basis . mag, 1e-5))   (taco_stft.py:10-16, :99-104)
  int n_mel, F;
  float* pre;              // optional [B][n_mel][F]: the pre-log sums basis . mag (saved for the backward)
  const int* lens;         // ragged batch: device [B] sample counts (columns behind an utterance's frames are 0) or null
  int N;                   // ragged batch: row pitch of the audio, the upper limit of a length
};
struct IstftArgs {
  const float* rec;        // [B][1056][Fs]
  const float* invA;       // packed A fragments [8 mtile][4 j][528 kstep][64 lanes] (the forward basis for the grad)
  const float* win_sq;     // [1024]
  float* out;              // [B][N]
  int N, F, Fs;
  float* edge;             // grad only: [B][1024] padded positions 0..511 and N+512..N+1023 (N the utterance's own)
  const int* lens;         // ragged batch: device [B] sample counts (out[b][lens[b]:] = 0) or null
};
struct MelBwdArgs {
  const float* g;          // [B][n_mel][F]  d mel
  const float* pre;        // [B][n_mel][F]  pre-log sums A
  const float* mag;        // [B][513][F]
  const float* rec;        // [B][1056][Fs]  raw (re, im) of the forward
  const float* basis;      // [n_mel][513]
  float* gX;               // [B][1056][Fs]  d (re, im); pad rows / columns zero
  int n_mel, F, Fs;
  const int* lens;         // ragged batch: device [B] sample counts (g and pre behind an utterance's frames are unread,
                           // gX stays zero there) or null
  int N;                   // ragged batch: row pitch of the audio, the upper limit of a length
};

// Backward of the denoiser's spectral part (wg_stft_denoise_backward): d audio_out -> d (re, im) of the forward STFT.
struct DenoiseBwdArgs {
  const float* g;          // [B][N]  d loss / d audio_out
  const float* invA;       // inverse basis as packed A fragments [33 mtile][512 kstep][64 lanes] (the layout of fwdA)
  const float* win_sq;     // [1024]
  const float* bias;       // [513] or null
  float strength;
  const float* raw;        // [B][1056][Fs]  raw (re, im) of the forward
  float* gX;               // [B][1056][Fs]  d (re, im); pad rows / columns zero
  int N, F, Fs;
  int phase_grad;          // 1: the derivative of the forward; 0: the reference's graph (phase detached, stft.py:160-161)
  const int* lens;         // ragged batch: device [B] sample counts (g behind an utterance is unread, gX behind its
                           // frames stays zero) or null
};

hipError_t launch_stft(const StftArgs& a, int B, hipStream_t s);
hipError_t launch_stft_saved(const StftArgs& a, int B, hipStream_t s);
hipError_t launch_denoise_bwd(const DenoiseBwdArgs& a, int B, hipStream_t s);
hipError_t launch_mel(const MelArgs& a, int B, hipStream_t s);
hipError_t launch_istft(const IstftArgs& a, int B, hipStream_t s);
hipError_t launch_mel_bwd(const MelBwdArgs& a, int B, hipStream_t s);
hipError_t launch_stft_grad(const IstftArgs& a, int B, hipStream_t s);

}  // namespace wg
