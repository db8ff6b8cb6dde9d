// C ABI of the STFT denoiser (include/waveglow_amd.h: wg_stft_*).
#include "wg_host.h"
#include "wg_stft.h"

using namespace wg;

struct wg_stft {
  int device;
  float *d_fwdA = nullptr, *d_invA = nullptr, *d_win = nullptr;
  float* d_fwdT = nullptr;   // forward basis in the inverse's polyphase pack: A operand of the transposed conv-STFT
  float* d_invF = nullptr;   // inverse basis in the forward's pack: A operand of the transposed inverse STFT
};

extern "C" {

int wg_stft_create(const float* fwd_basis, const float* inv_basis, const float* win_sq, int32_t filter_length,
                   int32_t hop_length, int32_t device_id, wg_stft** out) {
  if (!fwd_basis || !inv_basis || !win_sq || !out) return fail(WG_ERR_INVALID, "null argument");
  if (filter_length != kFL || hop_length != kHop)
    return fail(WG_ERR_INVALID, "only filter_length 1024 / hop_length 256 are supported");
  // basis row c of the library = interleaved (re_k, im_k): c = 2k -> reference row k, c = 2k+1 -> row 513 + k
  auto ref_row = [](int c) { return (c & 1) ? kCut + (c >> 1) : (c >> 1); };
  std::vector<float> fa((size_t)(kRows / 32) * (kFL / 2) * 64, 0.f), ia((size_t)8 * 4 * (kRows / 2) * 64, 0.f);
  std::vector<float> ft(ia.size(), 0.f), iv(fa.size(), 0.f);
  for (int mt = 0; mt < kRows / 32; ++mt)
    for (int ks = 0; ks < kFL / 2; ++ks)
      for (int lane = 0; lane < 64; ++lane) {
        const int c = mt * 32 + (lane & 31), k = 2 * ks + (lane >> 5);
        if (c < 2 * kCut) {
          fa[((size_t)mt * (kFL / 2) + ks) * 64 + lane] = fwd_basis[(size_t)ref_row(c) * kFL + k];
          iv[((size_t)mt * (kFL / 2) + ks) * 64 + lane] = inv_basis[(size_t)ref_row(c) * kFL + k];
        }
      }
  for (int w = 0; w < 8; ++w)
    for (int j = 0; j < 4; ++j)
      for (int ks = 0; ks < kRows / 2; ++ks)
        for (int lane = 0; lane < 64; ++lane) {
          const int r = w * 32 + (lane & 31), c = 2 * ks + (lane >> 5);
          if (c < 2 * kCut) {
            const size_t i = (((size_t)w * 4 + j) * (kRows / 2) + ks) * 64 + lane;
            ia[i] = inv_basis[(size_t)ref_row(c) * kFL + r + kHop * j];
            ft[i] = fwd_basis[(size_t)ref_row(c) * kFL + r + kHop * j];
          }
        }
  wg_stft* h = new wg_stft();
  h->device = device_id;
  DeviceGuard dev_guard;
  HIP_TRY(hipGetDevice(&dev_guard.prev));
  HIP_TRY(hipSetDevice(device_id));
  HIP_TRY(hipMalloc((void**)&h->d_fwdA, fa.size() * 4));
  HIP_TRY(hipMalloc((void**)&h->d_invA, ia.size() * 4));
  HIP_TRY(hipMalloc((void**)&h->d_win, kFL * 4));
  HIP_TRY(hipMalloc((void**)&h->d_fwdT, ft.size() * 4));
  HIP_TRY(hipMalloc((void**)&h->d_invF, iv.size() * 4));
  HIP_TRY(hipMemcpy(h->d_fwdA, fa.data(), fa.size() * 4, hipMemcpyHostToDevice));
  HIP_TRY(hipMemcpy(h->d_invA, ia.data(), ia.size() * 4, hipMemcpyHostToDevice));
  HIP_TRY(hipMemcpy(h->d_win, win_sq, kFL * 4, hipMemcpyHostToDevice));
  HIP_TRY(hipMemcpy(h->d_fwdT, ft.data(), ft.size() * 4, hipMemcpyHostToDevice));
  HIP_TRY(hipMemcpy(h->d_invF, iv.data(), iv.size() * 4, hipMemcpyHostToDevice));
  *out = h;
  return WG_OK;
}

int wg_stft_destroy(wg_stft* h) {
  if (!h) return WG_OK;
  if (h->d_fwdA) (void)hipFree(h->d_fwdA);
  if (h->d_invA) (void)hipFree(h->d_invA);
  if (h->d_win) (void)hipFree(h->d_win);
  if (h->d_fwdT) (void)hipFree(h->d_fwdT);
  if (h->d_invF) (void)hipFree(h->d_invF);
  delete h;
  return WG_OK;
}

static int frames_padded(int F) { return 3 + (F + 3 + 31) / 32 * 32 + 32; }

size_t wg_stft_workspace_bytes(const wg_stft* h, int32_t B, int32_t n_samples) {
  if (!h || B < 1 || n_samples < kFL || n_samples % kHop) return 0;
  const int F = n_samples / kHop + 1;
  return (size_t)B * kRows * frames_padded(F) * 4;
}

// lens == nullptr: every row has n_samples samples.  Otherwise lens is a device array read by the kernels only.
int wg_stft_denoise(wg_stft* h, const float* audio, const int32_t* lens, const float* bias_mag, float strength,
                    float* audio_out, float* mag0_out, int32_t B, int32_t n_samples, void* workspace,
                    size_t workspace_bytes, void* stream) {
  if (!h || !audio || !workspace) return fail(WG_ERR_INVALID, "null argument");
  if (B < 1 || n_samples < kFL || n_samples % kHop)
    return fail(WG_ERR_INVALID, "n_samples must be a multiple of 256 and >= 1024");
  const size_t need = wg_stft_workspace_bytes(h, B, n_samples);
  if (workspace_bytes < need) return fail(WG_ERR_WORKSPACE, "stft workspace too small");
  hipStream_t s = (hipStream_t)stream;
  const int F = n_samples / kHop + 1, Fs = frames_padded(F);
  HIP_TRY(hipMemsetAsync(workspace, 0, need, s));           // zero lead/tail columns and pad rows
  StftArgs a{audio, h->d_fwdA, bias_mag, strength, (float*)workspace, mag0_out, n_samples, F, Fs, nullptr,
             lens, kFL, kHop - 1};
  HIP_TRY(launch_stft(a, B, s));
  if (audio_out) {
    IstftArgs b{(const float*)workspace, h->d_invA, h->d_win, audio_out, n_samples, F, Fs, nullptr, lens};
    HIP_TRY(launch_istft(b, B, s));
  }
  return WG_OK;
}

// Denoiser-gradient state buffer, in floats: [rec, then gX | edge | raw].  rec (the recombined spectrum the forward hands
// its inverse) and gX (the backward's d (re, im)) share the first plane, each zeroed by the call that fills it; edge is
// [B][1024]; raw, the (re, im) of the forward STFT, is the one part a backward reads and needs no zeroing: only cells of
// an utterance's own bins and frames are ever read.
struct DenoiseGradLayout {
  int F, Fs;
  size_t plane, edge, raw, total;          // float offsets; total in floats
};
static DenoiseGradLayout denoise_grad_layout(int B, int n_samples) {
  DenoiseGradLayout L;
  L.F = n_samples / kHop + 1;
  L.Fs = frames_padded(L.F);
  L.plane = 0;
  L.edge = (size_t)B * kRows * L.Fs;
  L.raw = L.edge + (size_t)B * kFL;
  L.total = L.raw + (size_t)B * kRows * L.Fs;
  return L;
}

size_t wg_stft_denoise_grad_workspace_bytes(const wg_stft* h, int32_t B, int32_t n_samples) {
  if (!h || B < 1 || n_samples < kFL || n_samples % kHop) return 0;
  return denoise_grad_layout(B, n_samples).total * 4;
}

static int denoise_grad_check(wg_stft* h, const void* in, const void* out, int32_t B, int32_t n_samples, float* state,
                              size_t state_bytes) {
  if (!h || !in || !out || !state) return fail(WG_ERR_INVALID, "null argument");
  const size_t need = wg_stft_denoise_grad_workspace_bytes(h, B, n_samples);
  if (!need) return fail(WG_ERR_INVALID, "n_samples must be a multiple of 256 and >= 1024");
  if (state_bytes < need) return fail(WG_ERR_WORKSPACE, "denoiser gradient state buffer too small");
  return WG_OK;
}

// lens as in wg_stft_denoise.
int wg_stft_denoise_forward_saved(wg_stft* h, const float* audio, const int32_t* lens, const float* bias_mag,
                                  float strength, float* audio_out, int32_t B, int32_t n_samples, float* state,
                                  size_t state_bytes, void* stream) {
  const int rc = denoise_grad_check(h, audio, audio_out, B, n_samples, state, state_bytes);
  if (rc != WG_OK) return rc;
  hipStream_t s = (hipStream_t)stream;
  const DenoiseGradLayout L = denoise_grad_layout(B, n_samples);
  float* ws = state;
  HIP_TRY(hipMemsetAsync(ws + L.plane, 0, (L.edge - L.plane) * 4, s));   // zero lead/tail columns and pad rows of rec
  StftArgs a{audio, h->d_fwdA, bias_mag, strength, ws + L.plane, nullptr, n_samples, L.F, L.Fs, nullptr,
             lens, kFL, kHop - 1, ws + L.raw};
  HIP_TRY(launch_stft_saved(a, B, s));
  IstftArgs b{ws + L.plane, h->d_invA, h->d_win, audio_out, n_samples, L.F, L.Fs, nullptr, lens};
  HIP_TRY(launch_istft(b, B, s));
  return WG_OK;
}

int wg_stft_denoise_backward(wg_stft* h, const float* g_out, const int32_t* lens, const float* bias_mag, float strength,
                             int32_t phase_grad, float* audio_grad_out, int32_t B, int32_t n_samples, float* state,
                             size_t state_bytes, void* stream) {
  const int rc = denoise_grad_check(h, g_out, audio_grad_out, B, n_samples, state, state_bytes);
  if (rc != WG_OK) return rc;
  hipStream_t s = (hipStream_t)stream;
  const DenoiseGradLayout L = denoise_grad_layout(B, n_samples);
  float* ws = state;
  HIP_TRY(hipMemsetAsync(ws + L.plane, 0, (L.raw - L.plane) * 4, s));    // gX pads and uncovered edge positions are zero
  DenoiseBwdArgs d{g_out, h->d_invF, h->d_win, bias_mag, strength, ws + L.raw, ws + L.plane, n_samples, L.F, L.Fs,
                   phase_grad ? 1 : 0, lens};
  HIP_TRY(launch_denoise_bwd(d, B, s));
  IstftArgs t{ws + L.plane, h->d_fwdT, nullptr, audio_grad_out, n_samples, L.F, L.Fs, ws + L.edge, lens};
  HIP_TRY(launch_stft_grad(t, B, s));
  return WG_OK;
}

size_t wg_stft_mel_workspace_bytes(const wg_stft* h, int32_t B, int32_t n_samples) {
  if (!h || B < 1 || n_samples < kFL / 2 + 1) return 0;          // reflect padding needs n_samples > filter/2
  return (size_t)B * kCut * (n_samples / kHop + 1) * 4;
}

// lens as in wg_stft_denoise.
int wg_stft_mel(wg_stft* h, const float* mel_basis, int32_t n_mel, const float* audio, const int32_t* lens,
                float* mel_out, int32_t B, int32_t n_samples, void* workspace, size_t workspace_bytes, void* stream) {
  if (!h || !mel_basis || !audio || !mel_out || !workspace) return fail(WG_ERR_INVALID, "null argument");
  const size_t need = wg_stft_mel_workspace_bytes(h, B, n_samples);
  if (!need || n_mel < 1 || n_mel > 128) return fail(WG_ERR_INVALID, "bad B / n_samples / n_mel");
  if (workspace_bytes < need) return fail(WG_ERR_WORKSPACE, "mel workspace too small");
  hipStream_t s = (hipStream_t)stream;
  const int F = n_samples / kHop + 1;                             // stft.py:141-152: reflect pad filter/2 both sides
  StftArgs a{audio, h->d_fwdA, nullptr, 0.0f, nullptr, nullptr, n_samples, F, 0, (float*)workspace,
             lens, kFL / 2 + 1, 0};
  HIP_TRY(launch_stft(a, B, s));
  MelArgs m{(const float*)workspace, mel_basis, mel_out, n_mel, F, nullptr, lens, n_samples};
  HIP_TRY(launch_mel(m, B, s));
  return WG_OK;
}

// Mel-gradient workspace, in floats: [rec | gX | edge] (zeroed by the call that fills it) then [mag | pre].
// rec and gX are [B][1056][Fs], edge [B][1024], mag [B][513][F], pre [B][128][F] (sized for the largest n_mel).
struct MelGradLayout {
  int F, Fs;
  size_t rec, gX, edge, mag, pre, total;   // float offsets; total in floats
};
static MelGradLayout mel_grad_layout(int B, int n_samples) {
  MelGradLayout L;
  L.F = n_samples / kHop + 1;
  L.Fs = frames_padded(L.F);
  const size_t plane = (size_t)B * kRows * L.Fs;
  L.rec = 0;
  L.gX = plane;
  L.edge = 2 * plane;
  L.mag = L.edge + (size_t)B * kFL;
  L.pre = L.mag + (size_t)B * kCut * L.F;
  L.total = L.pre + (size_t)B * 128 * L.F;
  return L;
}

size_t wg_stft_mel_grad_workspace_bytes(const wg_stft* h, int32_t B, int32_t n_samples) {
  if (!h || B < 1 || n_samples < kFL / 2 + 1) return 0;          // reflect padding needs n_samples > filter/2
  return mel_grad_layout(B, n_samples).total * 4;
}

static int mel_grad_check(wg_stft* h, const float* mel_basis, int32_t n_mel, const void* in, const void* out, int32_t B,
                          int32_t n_samples, void* workspace, size_t workspace_bytes) {
  if (!h || !mel_basis || !in || !out || !workspace) return fail(WG_ERR_INVALID, "null argument");
  const size_t need = wg_stft_mel_grad_workspace_bytes(h, B, n_samples);
  if (!need || n_mel < 1 || n_mel > 128) return fail(WG_ERR_INVALID, "bad B / n_samples / n_mel");
  if (workspace_bytes < need) return fail(WG_ERR_WORKSPACE, "mel gradient workspace too small");
  return WG_OK;
}

// lens == nullptr: every row has n_samples samples.  Otherwise lens is a device array read by the kernels only.
int wg_stft_mel_forward_saved(wg_stft* h, const float* mel_basis, int32_t n_mel, const float* audio,
                              const int32_t* lens, float* mel_out, int32_t B, int32_t n_samples, void* workspace,
                              size_t workspace_bytes, void* stream) {
  const int rc = mel_grad_check(h, mel_basis, n_mel, audio, mel_out, B, n_samples, workspace, workspace_bytes);
  if (rc != WG_OK) return rc;
  hipStream_t s = (hipStream_t)stream;
  const MelGradLayout L = mel_grad_layout(B, n_samples);
  float* ws = (float*)workspace;
  HIP_TRY(hipMemsetAsync(ws + L.rec, 0, (L.gX - L.rec) * 4, s));  // zero lead/tail columns and pad rows of rec
  StftArgs a{audio, h->d_fwdA, nullptr, 0.0f, ws + L.rec, nullptr, n_samples, L.F, L.Fs, ws + L.mag,
             lens, kFL / 2 + 1, 0};
  HIP_TRY(launch_stft(a, B, s));
  MelArgs m{ws + L.mag, mel_basis, mel_out, n_mel, L.F, ws + L.pre, lens, n_samples};
  HIP_TRY(launch_mel(m, B, s));
  return WG_OK;
}

int wg_stft_mel_backward(wg_stft* h, const float* mel_basis, int32_t n_mel, const float* g_mel, const int32_t* lens,
                         float* audio_grad_out, int32_t B, int32_t n_samples, void* workspace, size_t workspace_bytes,
                         void* stream) {
  const int rc = mel_grad_check(h, mel_basis, n_mel, g_mel, audio_grad_out, B, n_samples, workspace, workspace_bytes);
  if (rc != WG_OK) return rc;
  hipStream_t s = (hipStream_t)stream;
  const MelGradLayout L = mel_grad_layout(B, n_samples);
  float* ws = (float*)workspace;
  HIP_TRY(hipMemsetAsync(ws + L.gX, 0, (L.mag - L.gX) * 4, s));   // gX pads and uncovered edge positions are zero
  MelBwdArgs m{g_mel, ws + L.pre, ws + L.mag, ws + L.rec, mel_basis, ws + L.gX, n_mel, L.F, L.Fs, lens, n_samples};
  HIP_TRY(launch_mel_bwd(m, B, s));
  IstftArgs t{ws + L.gX, h->d_fwdT, nullptr, audio_grad_out, n_samples, L.F, L.Fs, ws + L.edge, lens};
  HIP_TRY(launch_stft_grad(t, B, s));
  return WG_OK;
}

}  // extern "C"
