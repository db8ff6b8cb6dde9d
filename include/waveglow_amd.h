/*
 * waveglow_amd.h -- C ABI of the MI355X-native WaveGlow hot path (libwaveglow_amd.so).
 *
 * The reference (stefantaubert/waveglow) is pure Python and has no FFI of its own; the
 * interface this library replaces is the set of Python methods on its model object
 * (paths relative to /root/reference/):
 *
 *   wg_create / wg_set_tensor / wg_finalize  <-  WaveGlow.__init__ (src/waveglow/model.py:141-176),
 *       load_model -> load_state_dict (src/waveglow/train.py:48-55) and
 *       WaveGlow.remove_weightnorm (model.py:276-297): tensors are handed over by their
 *       state_dict names in weight-norm-removed form.
 *   wg_infer    <-  WaveGlow.infer(spect, sigma)          (model.py:223-274)
 *   wg_forward  <-  WaveGlow.forward((spect, audio))       (model.py:178-221)
 *
 * Conventions: plain pointers and sizes only.  `mel`, noise, outputs and `workspace` are DEVICE
 * pointers owned by the caller; weights given to wg_set_tensor are HOST fp32 pointers and are
 * copied.  Every call returns 0 on success or a negative wg_status; wg_last_error() gives the
 * message of the last failure on the calling thread.  wg_infer / wg_forward only enqueue work on
 * `stream` (a hipStream_t passed as void*); they never synchronise, allocate or free.
 * One handle per device; a handle may be used from one stream at a time.
 */
#ifndef WAVEGLOW_AMD_H
#define WAVEGLOW_AMD_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct wg_handle wg_handle;

typedef enum wg_status {
  WG_OK = 0,
  WG_ERR_INVALID = -1,      /* bad argument / unsupported configuration */
  WG_ERR_STATE = -2,        /* call order (e.g. infer before finalize, missing tensor) */
  WG_ERR_HIP = -3,          /* HIP runtime error (message has the hipError string) */
  WG_ERR_WORKSPACE = -4     /* workspace too small */
} wg_status;

typedef enum wg_dtype { WG_F32 = 0, WG_F16 = 1 } wg_dtype;

/* Model-shaping fields of ModelHParams (src/waveglow/hparams.py:19-31) plus the fixed
 * upsample geometry of model.py:145-150. */
typedef struct wg_config {
  int32_t n_mel_channels;   /* 80 */
  int32_t n_flows;          /* 12 */
  int32_t n_group;          /* 8 (only 8 is supported) */
  int32_t n_early_every;    /* 4 */
  int32_t n_early_size;     /* 2 */
  int32_t n_layers;         /* 8 (dilation 2^i, i < n_layers; <= 8) */
  int32_t n_channels;       /* 64, 128, 256 or 512 */
  int32_t kernel_size;      /* 3 (only 3 is supported) */
  int32_t upsample_kernel;  /* 1024 */
  int32_t upsample_stride;  /* 256 */
} wg_config;

const char* wg_version(void);
const char* wg_last_error(void);

/* WaveGlow.__init__ (model.py:141-176): validates the configuration, selects device `device_id`. */
int wg_create(const wg_config* cfg, int device_id, wg_handle** out);
int wg_destroy(wg_handle* h);

/* One tensor of the weight-norm-removed state_dict (model.py:276-297), fp32, host memory, C order.
 * Names and shapes are the reference's: "upsample.weight" [M,M,K], "upsample.bias" [M],
 * "convinv.k.conv.weight" [c_k,c_k,1], "WN.k.start.{weight [C,h_k,1],bias [C]}",
 * "WN.k.cond_layer.{weight [2C*n_layers, M*8, 1], bias}", "WN.k.in_layers.i.{weight [2C,C,3], bias}",
 * "WN.k.res_skip_layers.i.{weight [2C or C, C, 1], bias}", "WN.k.end.{weight [2h_k,C,1], bias}". */
int wg_set_tensor(wg_handle* h, const char* name, const float* data, const int64_t* shape, int32_t ndim);

/* Number of tensors wg_finalize expects, and the i-th expected name (for host-side checks). */
int wg_num_expected_tensors(const wg_handle* h);
const char* wg_expected_tensor_name(const wg_handle* h, int32_t i);

/* Packs all tensors into the kernels' MFMA fragment layouts (fp16 operands, fp32 biases), inverts the
 * 1x1 matrices in fp64 (model.py:51-60: W.float().inverse()), and uploads them.  May be called again
 * after further wg_set_tensor calls (derived state is rebuilt; no stale W^-1, unlike model.py:52-58). */
int wg_finalize(wg_handle* h);

/* Bytes of device workspace wg_infer / wg_forward need for batch B and n_frames mel frames
 * (forward: audio_len samples per utterance, a multiple of n_group). 0 on invalid arguments and for a batch
 * outside the accepted size range, which the calls refuse with WG_ERR_INVALID before they look at the workspace:
 *   B * (F + 8) <= 1 048 448   (F = n_frames, forward: ceil(audio_len / 256); F + 16 / F + 32 at 9 / 10 layers)
 * -- one 64-channel activation plane stays below 4 GiB. wg_last_error() says which. */
size_t wg_infer_workspace_bytes(const wg_handle* h, int32_t B, int32_t n_frames);
size_t wg_forward_workspace_bytes(const wg_handle* h, int32_t B, int32_t n_frames, int32_t audio_len);

/* WaveGlow.infer (model.py:223-274) with the noise injected (the caller draws it, keeping the
 * reference's RNG order: z_init [B, n_rem, L] first, then one [B, n_early_size, L] per early-output
 * flow in DESCENDING flow index; L = n_frames*upsample_stride/n_group).
 *   mel      [B, n_mel, n_frames]           io_dtype
 *   z_init   [B, n_rem, L]                  io_dtype
 *   z_early  n_z_early device pointers, each [B, n_early_size, L], io_dtype
 *   audio    [B, n_frames*upsample_stride]  io_dtype (output)
 * Arithmetic: fp16 MFMA operands, fp32 accumulation, fp32 flow state.
 * With `frames`, a batch of utterances of DIFFERENT lengths (serving; the reference's commented-out --batch-size,
 * src/waveglow_cli/inference_v2.py:64): a device array of B mel-frame counts, each <= n_frames; mel / noise / audio are
 * padded to n_frames (contents behind an utterance's own length are ignored, its audio tail is zero).  Every utterance
 * gets exactly the result of a batch-of-one call on its own frames: the padding columns are never written, so they are
 * the zero padding the convolutions see at the end of the sequence (model.py:98-102).  frames == NULL: every utterance
 * has n_frames frames. */
int wg_infer(wg_handle* h, const void* mel, const int32_t* frames, const void* z_init, const void* const* z_early,
             int32_t n_z_early, float sigma, void* audio, int32_t B, int32_t n_frames, int32_t io_dtype,
             void* workspace, size_t workspace_bytes, void* stream);

/* WaveGlow.forward (model.py:178-221), inference of the normalising direction (no autograd).
 *   mel      [B, n_mel, n_frames]     io_dtype
 *   audio    [B, audio_len]           io_dtype; audio_len % n_group == 0 and
 *                                     audio_len <= (n_frames-1)*stride + kernel  (model.py:187)
 *   z        [B, n_group, L]          fp32 out, L = audio_len / n_group
 *   log_s    n_flows device pointers, log_s[k] is [B, h_k, L] fp32 out
 *   log_det_W  HOST pointer to n_flows floats: B*L*logdet(W_k) (model.py:63), written before return
 * With `frames`, a batch of utterances of DIFFERENT lengths (scoring held-out audio): a device array of B mel-frame
 * counts as in wg_infer; utterance b is audio[b, :256 * frames[b]] under mel[b, :, :frames[b]].  audio_len must then be
 * 256 * n_frames and n_frames <= INT32_MAX >> 8 (WG_ERR_INVALID otherwise); size range and workspace are unchanged.
 * Every utterance gets, bit for bit, the z and log_s of a batch-of-one call on its own frames; z and every log_s[k] are
 * exactly 0 behind column 32 * frames[b].  Mel and audio behind an utterance are never used (they may hold NaN).  The
 * counts are never read on the host: one outside [1, n_frames] reads and writes nothing outside the buffers, and that
 * utterance's z and log_s are 0.  log_det_W may then be null (per column it is the handle's constant, see wg_nll) and
 * is filled when it is not.  frames == NULL: every utterance has audio_len samples, and log_det_W is required. */
int wg_forward(wg_handle* h, const void* mel, const int32_t* frames, const void* audio, float* z, float* const* log_s,
               float* log_det_W, int32_t B, int32_t n_frames, int32_t audio_len, int32_t io_dtype, void* workspace,
               size_t workspace_bytes, void* stream);

/* Negative log-likelihood per utterance and per mel frame from the outputs of wg_forward:
 * WaveGlowLoss (src/waveglow/train.py:31-45) of every utterance alone.  With L_b = 32 * frames[b] columns (L when
 * frames == NULL, the dense batch; with counts L must be a multiple of 32), n_b = 8 * L_b samples and
 * logdet = sum_k log|det W_k| of the handle (fp64, the value wg_forward multiplies by B * L, model.py:63):
 *   nll_b  = (sum z^2 / (2 sigma^2) - sum_k sum log_s[k] - L_b * logdet) / n_b        sums over the utterance's columns
 *   bits_b = (nll_b + ln(2 pi sigma^2) / 2) / ln 2                                    the constant the training loss drops
 * so sum_b n_b nll_b / sum_b n_b over a dense batch is the batch loss of wg_loss.
 *   z, log_s   device fp32, [B, n_group, L] and n_flows pointers to [B, h_k, L]
 *   frames     device int32 [B] or NULL; a count outside [1, L / 32] counts as 0 columns (samples 0, NaN figures)
 *   rows_out   device fp64 [B, 8]: nll, bits per sample, sum z^2, sum log_s, L_b * logdet, n_b, mean of z, variance of z
 *   frame_out  device fp64 [B, ceil(L / 32)] or NULL: the three terms over columns 32q .. 32q+31 of utterance b, divided
 *              by 256 (256 * the track sums to n_b * nll_b); NaN behind the utterance
 *   workspace  wg_nll_workspace_bytes(h, B, L) bytes (0 for a refused geometry: 1 <= B <= 65535, 1 <= L <= 2^26)
 * Two kernels (one more per 16 flows beyond the first 16) on `stream`; enqueue-only.  All sums are fp64 in a fixed order
 * without atomics: a call gives the same bits every time, an utterance the bits of its own call at any pitch L. */
size_t wg_nll_workspace_bytes(const wg_handle* h, int32_t B, int32_t L);
int wg_nll(const wg_handle* h, const float* z, const float* const* log_s, const int32_t* frames, double sigma, int32_t B,
           int32_t L, double* rows_out, double* frame_out, void* workspace, size_t workspace_bytes, void* stream);

/* WaveGlowLoss.forward (src/waveglow/train.py:31-45) on the outputs of wg_forward:
 *   loss = (sum z^2 / (2 sigma^2) - sum_k sum log_s[k] - sum_k log_det_W[k]) / z_elems      (z_elems = B*n_group*L)
 * z, log_s[k]: device fp32 with z_elems / log_s_elems[k] elements; log_det_W: n_flows HOST floats;
 * loss_out: DEVICE float; workspace: >= 16 bytes of device memory.  Enqueue-only; sums accumulate in fp64. */
int wg_loss(const float* z, int64_t z_elems, const float* const* log_s, const int64_t* log_s_elems, int32_t n_flows,
            const float* log_det_W, float sigma, float* loss_out, void* workspace, size_t workspace_bytes,
            void* stream);
/* The same with log_det_W as n_flows DEVICE floats: nothing of the loss passes through the host, so a training step
 * needs no stream synchronisation between forward and backward (the reference reads the 12 scalars as tensors too,
 * train.py:37-41). */
int wg_loss_dev(const float* z, int64_t z_elems, const float* const* log_s, const int64_t* log_s_elems, int32_t n_flows,
                const float* log_det_W_dev, float sigma, float* loss_out, void* workspace, size_t workspace_bytes,
                void* stream);

/* Algorithmic MACs per group-timestep (8 samples) of one infer pass, as SURVEY.md section 8(d) counts
 * them (for roofline reporting). */
double wg_macs_per_group_step(const wg_handle* h);

/* Which WN-layer kernel variant a call of this size runs on a device with n_cu compute units: the answer of the very
 * functions the launch code calls (csrc/wg_plan.h).  Pure host arithmetic: no handle, no GPU, nothing is enqueued.
 *   direction  WG_PLAN_INFER (wg_infer), WG_PLAN_FORWARD (wg_forward: the same rules), WG_PLAN_TRAIN (the fused layer
 *              kernel of wg_train_forward / wg_train_infer_forward, whose tile width the backward chain takes over), at
 *              audio_len = upsample_stride * n_frames.
 * The test switches WG_FORCE_BN, WG_RESIDENT, WG_DISABLE_DEEP and WG_TRAIN_HALVES are read from the environment at the
 * call, as the library reads them (WG_FORCE_BN of the first two directions: at wg_create).  Variants that differ in
 * block_n, form or deep are different kernels; the library promises the same bits from all of them
 * (tests/test_gpu_dispatch_identity.py). */
typedef enum wg_plan_direction { WG_PLAN_INFER = 0, WG_PLAN_FORWARD = 1, WG_PLAN_TRAIN = 2 } wg_plan_direction;
typedef enum wg_plan_form {
  WG_PLAN_SINGLE = 0,       /* one tile per workgroup */
  WG_PLAN_PAIR = 1,         /* two tiles per workgroup */
  WG_PLAN_RESIDENT = 2      /* resident tile walk: resident_wgs workgroups walk all tiles */
} wg_plan_form;
typedef struct wg_plan_result {
  int32_t block_n;            /* columns per tile: 64 or 128 */
  int32_t form;               /* wg_plan_form */
  int32_t resident_wgs;       /* grid of the resident walk, 0 otherwise */
  int32_t deep;               /* 1: the two-step-deep weight prefetch kernel (256 channels, 64 columns, single tiles) */
  int32_t frag16;             /* 1: GEMM 1 on 16x16x32 MFMAs from its own weight packing (256 channels, 128 columns) */
  int32_t halves;             /* WG_PLAN_TRAIN: 2 = the batch runs as two half-batch chains; otherwise 1 */
  int32_t rows_per_utterance; /* Fp: frames + guard frames (padded up with halves = 2) */
  int32_t rows_per_phase;     /* Rp: B * Fp rounded up to 128 (B * Fp with halves = 2) */
  int32_t n_tiles;            /* tiles of one layer launch: 32 * Rp / block_n (per half with halves = 2) */
} wg_plan_result;
int wg_plan(const wg_config* cfg, int32_t direction, int32_t B, int32_t n_frames, int32_t n_cu, wg_plan_result* out);

/* Per-kernel device timing: when enabled, wg_infer brackets its kernels with hipEvents on `stream`;
 * wg_profile_read synchronises those events and returns accumulated milliseconds per kernel class.
 * classes: 0 = mel_pack, 1 = flow/start, 2 = wn_layer, 3 = memset; with n_classes = 8 also the training direction
 * (wg_train_forward / wg_train_backward): 4 = fused layer forward, 5 = dgrad GEMMs, 6 = wgrad.  `on` = 1 times every class;
 * a value > 1 is a bit mask of the classes to time (bit c = class c). */
int wg_profile_enable(wg_handle* h, int32_t on);
int wg_profile_read(wg_handle* h, double* ms_per_class, int64_t* launches_per_class, int32_t n_classes);

/* ---- Denoiser (src/waveglow/denoiser.py:14-57 on the conv-STFT of src/waveglow/stft.py:98-198), fp32 -----------------
 * wg_stft_create: fwd_basis / inv_basis are the reference's windowed bases [2*513][1024] (STFT.__init__,
 *   stft.py:108-132: real rows then imaginary rows), win_sq the squared zero-centred window [1024]; HOST pointers.
 * wg_stft_denoise: audio [B][n_samples] fp32 device (n_samples % 256 == 0) ->
 *   audio_out [B][n_samples] = istft(max(|X| - strength*bias_mag, 0) * exp(i*arg X))   (Denoiser.forward), and/or
 *   mag0_out [B][513] = |X| of frame 0 (what Denoiser.__init__ keeps as bias_spec).  bias_mag null => no subtraction;
 *   audio_out null => transform only.  Enqueue-only.
 * With `lens`, a batch of utterances of DIFFERENT lengths (Denoiser.forward per utterance, denoiser.py:51-57 on
 *   stft.py:134-198): a device array of B sample counts, each a multiple of 256 in [1024, n_samples]; n_samples is the
 *   row pitch of audio / audio_out and sizes the workspace.  Utterance b gets bit for bit what the call with B = 1,
 *   n_samples = lens[b] and a null lens gives it: reflect padding about its own last sample, lens[b]/256 + 1 frames, the
 *   window-sum-square of those frames, cropping to lens[b]; audio_out[b][lens[b]:] = 0.  lens is read by the kernels
 *   only (enqueue-only, nothing synchronised); a length outside the limits is treated as 0: that row comes out all zero
 *   (its mag0_out row is not written) and nothing is indexed with it.  lens == NULL: every row has n_samples samples. */
typedef struct wg_stft wg_stft;
int wg_stft_create(const float* fwd_basis, const float* inv_basis, const float* win_sq, int32_t filter_length,
                   int32_t hop_length, int32_t device_id, wg_stft** out);
int wg_stft_destroy(wg_stft* h);
size_t wg_stft_workspace_bytes(const wg_stft* h, int32_t B, int32_t n_samples);
int wg_stft_denoise(wg_stft* h, const float* audio, const int32_t* lens, const float* bias_mag, float strength,
                    float* audio_out, float* mag0_out, int32_t B, int32_t n_samples, void* workspace,
                    size_t workspace_bytes, void* stream);

/* Denoiser with an audio gradient, Denoiser.forward_differentiable (denoiser.py:51-57 under autograd: stft.py:135-198).
 * Same arguments and n_samples rule as wg_stft_denoise (audio_out is required, there is no mag0_out), with one typed
 * fp32 device buffer `state` of wg_stft_denoise_grad_workspace_bytes in place of the untyped workspace: it holds the
 * spectrum that lives from the forward to its backward, and in front of it the planes either call fills for itself.
 * wg_stft_denoise_forward_saved: audio_out bit-identical to wg_stft_denoise; keeps the raw (re, im) of the forward
 *   transform in `state` for the backward.
 * wg_stft_denoise_backward: g_out [B][n_samples] fp32 device = d loss / d audio_out -> audio_grad_out [B][n_samples] =
 *   d loss / d audio, through the crop and the window-sum-square normalisation (stft.py:175-196), the transposed inverse
 *   transform (stft.py:169-173), the spectral subtraction (denoiser.py:54-55), the conv-STFT and the reflect padding
 *   (stft.py:141-153).  Per (bin, frame), with c = strength * bias_mag[bin]: no gradient where |X| = 0 (never NaN) and
 *   where |X| - c < 0 (the clamp passes its bound).  phase_grad != 0: the derivative of what the forward computes,
 *   max(|X| - c, 0) X / |X|.  phase_grad = 0: what the reference's own autograd gives, whose STFT.transform detaches the
 *   phase (stft.py:160-161): g X = (Re(conj(X) g Y) / |X|^2) X.  bias_mag and strength are constants: pass the forward's.
 *   bias_mag null => no subtraction.  Reads the `state` of a forward_saved call with the same B and n_samples; leaves
 *   that call's saved state intact, so it may run more than once.
 * With `lens` (as in wg_stft_denoise: device [B], multiples of 256 in [1024, n_samples], anything else counts as 0;
 *   read by the kernels only; n_samples the row pitch): g_out at and behind lens[b] is not read;
 *   audio_grad_out[b][:lens[b]] is bit for bit the backward of that utterance alone with a null lens,
 *   audio_grad_out[b][lens[b]:] = 0.  Pass the backward the lens of its forward.  lens == NULL: every row has n_samples.
 * One `state` of wg_stft_denoise_grad_workspace_bytes serves both; what it holds before forward_saved does not matter.
 *   The saved spectrum [B][1056][Fs] is its tail of (bytes - B * 4096) / 2 bytes; the rest ([B][1056][Fs] for the
 *   recombined spectrum, then d (re, im); [B][1024] edges) each call zeroes for itself, so the caller may use it between
 *   the two calls.  Enqueue-only. */
size_t wg_stft_denoise_grad_workspace_bytes(const wg_stft* h, int32_t B, int32_t n_samples);
int wg_stft_denoise_forward_saved(wg_stft* h, const float* audio, const int32_t* lens, const float* bias_mag,
                                  float strength, float* audio_out, int32_t B, int32_t n_samples, float* state,
                                  size_t state_bytes, void* stream);
int wg_stft_denoise_backward(wg_stft* h, const float* g_out, const int32_t* lens, const float* bias_mag, float strength,
                             int32_t phase_grad, float* audio_grad_out, int32_t B, int32_t n_samples, float* state,
                             size_t state_bytes, void* stream);

/* Mel front-end, TacotronSTFT.mel_spectrogram (src/waveglow/taco_stft.py:84-104): STFT magnitudes (reflect padding,
 * stft.py:141-152) x mel filterbank -> log(clamp(., 1e-5)).  audio [B][n_samples] fp32 device (any n_samples > 512),
 * mel_basis [n_mel][513] fp32 DEVICE, mel_out [B][n_mel][n_samples/256 + 1] fp32 device.  Enqueue-only.
 * With `lens`, a batch of utterances of DIFFERENT lengths (taco_stft.py:84-103 per utterance): a device array of B sample
 * counts, each in (512, n_samples]; n_samples is the row pitch of audio and sizes the workspace.  Columns of mel_out
 * below lens[b]/256 + 1 are bit for bit those of the call with a null lens on that utterance alone, the others are 0.
 * A length outside the limits is treated as 0 (row all zero).  lens == NULL: every row has n_samples samples. */
size_t wg_stft_mel_workspace_bytes(const wg_stft* h, int32_t B, int32_t n_samples);
int wg_stft_mel(wg_stft* h, const float* mel_basis, int32_t n_mel, const float* audio, const int32_t* lens,
                float* mel_out, int32_t B, int32_t n_samples, void* workspace, size_t workspace_bytes, void* stream);

/* Mel front-end with an audio gradient, TacotronSTFT.mel_spectrogram_differentiable (taco_stft.py:84-104 without the
 * detach at :99; conv-STFT of stft.py:135-163).  Same arguments and n_samples rule as wg_stft_mel (n_mel <= 128).
 * wg_stft_mel_forward_saved: mel_out bit-identical to wg_stft_mel; keeps (re, im), |X| and the pre-log sums in the
 *   workspace for the backward.
 * wg_stft_mel_backward: g_mel [B][n_mel][n_samples/256 + 1] fp32 device -> audio_grad_out [B][n_samples] = d loss /
 *   d audio, through log(clamp(., 1e-5)) (gradient where the sum >= 1e-5), the mel projection, |X| (0 where |X| = 0),
 *   the conv-STFT and the reflect padding.  Reads the workspace of a forward_saved call with the same mel_basis, n_mel,
 *   B and n_samples; leaves that call's saved state intact, so it may run more than once.
 * With `lens` (as in wg_stft_mel: device [B], each in (512, n_samples], anything else counts as 0; read by the kernels
 *   only; n_samples the row pitch): mel_out of the forward is 0 at and behind column lens[b]/256 + 1; g_mel at and behind
 *   an utterance's frame count is not read; audio_grad_out[b][:lens[b]] is bit for bit the backward of that utterance
 *   alone with a null lens (reflect padding folded about its own sample lens[b] - 1), audio_grad_out[b][lens[b]:] = 0.
 *   Pass the backward the lens of its forward.  lens == NULL: every row has n_samples samples.
 * One workspace of wg_stft_mel_grad_workspace_bytes serves both.  Enqueue-only. */
size_t wg_stft_mel_grad_workspace_bytes(const wg_stft* h, int32_t B, int32_t n_samples);
int wg_stft_mel_forward_saved(wg_stft* h, const float* mel_basis, int32_t n_mel, const float* audio, const int32_t* lens,
                              float* mel_out, int32_t B, int32_t n_samples, void* workspace, size_t workspace_bytes,
                              void* stream);
int wg_stft_mel_backward(wg_stft* h, const float* mel_basis, int32_t n_mel, const float* g_mel, const int32_t* lens,
                         float* audio_grad_out, int32_t B, int32_t n_samples, void* workspace, size_t workspace_bytes,
                         void* stream);

/* ---- PCM finishing of a synthesised batch (src/waveglow/audio_utils.py:36-95, :132-138), no handle -----------------
 * raw, denoised [B][n_samples] fp32 device (they may be the same array), lens device [B] sample counts (clamped to
 * [0, n_samples]), n_samples a multiple of 8, arrays 16-byte aligned.  Per utterance b over [0, lens[b]):
 *   stats_out[b] = {raw min, raw max, raw max|x|, denoised min, denoised max, denoised max|x|, f, 0} (8 floats, device);
 *     f = 1 when a sample of either signal is NaN or infinite (the host functions' own asserts fail on such input), else 0.
 *     is_overamp (audio_utils.py:132-138) is raw min < -1 or raw max > 1.
 *   pcm_out[b] = int16 of convert_wav(normalize_wav(denoised[b])) (audio_utils.py:67-95, :36-64) in float32 arithmetic:
 *     y = x / peak (IEEE division) unless peak is 1 or 0, then round-half-even of y * 32767; pcm_out[b][lens[b]:] = 0.
 * Bit for bit the host functions' result.  Workspace: device memory for the per-chunk extrema.  Enqueue-only. */
size_t wg_wav_finish_workspace_bytes(int32_t B);
int wg_wav_finish(const float* raw, const float* denoised, const int32_t* lens, int16_t* pcm_out, float* stats_out,
                  int32_t B, int32_t n_samples, void* workspace, size_t workspace_bytes, void* stream);

/* ---- Training segments out of a device-resident wav pool (src/waveglow/dataloader.py:45-54, audio_utils.py:141-150
 * get_wav_tensor_segment, :36-64 convert_wav), no handle ----------------------------------------------------------------
 * pool: the samples of n_utt utterances back to back on the device, int16 (WG_PCM_I16) or fp32 (WG_PCM_F32), pool_elems
 * of them; offsets device [n_utt + 1] int64, ascending, offsets[n_utt] == pool_elems; picks device [B][2] int32:
 * utterance index, start sample.  For row b with u = picks[b][0], s = picks[b][1], len = offsets[u+1] - offsets[u]:
 *   audio_out[b][i] = conv(pool[offsets[u] + s + i]) where s + i < len, 0 elsewhere (the zero padding a short utterance
 *   gets); conv is (float)x * (1.0f / 32768.0f) for int16 -- a power of two, so bit for bit what convert_wav computes in
 *   fp64 and rounds -- and the identity for fp32.
 * A pick outside the pool (u outside [0, n_utt), s < 0, s > max(len - segment_length, 0)) gives an all-zero row and, if
 * status_out (device [1], may be null) is given, sets status_out[0] = 1; otherwise status_out is left alone.  Nothing
 * outside [0, pool_elems) is read whatever the picks hold.  One launch, no workspace.  Enqueue-only. */
typedef enum wg_pcm_dtype { WG_PCM_I16 = 0, WG_PCM_F32 = 1, WG_PCM_F64 = 2 /* wg_resample_backward's d_out only */ } wg_pcm_dtype;
int wg_data_gather(const void* pool, int32_t pool_dtype, int64_t pool_elems, const int64_t* offsets, int32_t n_utt,
                   const int32_t* picks, float* audio_out, int32_t* status_out, int32_t B, int32_t segment_length,
                   void* stream);

/* ---- Streaming synthesis: the windows of a step in, the chunks of a step out (not in the reference), no handle ------
 * A step over B streams synthesises one window per stream as a ragged batch (wg_infer, wg_stft_denoise with lengths)
 * and hands out the interior of each window.  Both tables are device arrays of B rows, read by the kernels only.
 * wg_stream_gather, one launch: for row b with w = windows[b], n = w.count clamped to [0, w_max] and to the source's
 *   pitch (a negative start or count counts as n = 0), cpf = cols_per_frame (256 / n_group: 32):
 *     mel_out[b][m][f]        = w.mel[m * w.mel_pitch + w.start + f]                      m < n_mel, f < n; 0 elsewhere
 *                               (mel_out is [B][n_mel_out][w_max], n_mel_out >= n_mel: the rows behind n_mel are 0)
 *     z_init_out[b][c][l]     = w.z_init[c * w.noise_pitch + cpf * w.start + l]           c < n_rem, l < cpf * n; 0 elsewhere
 *     z_early_out[i][b][c][l] = w.z_early[i][c * w.noise_pitch + cpf * w.start + l]       c < n_early_size, likewise
 *   (z_init_out [B][n_rem][cpf * w_max], z_early_out: host array of n_early device arrays [B][n_early_size][cpf * w_max],
 *   0 <= n_early <= WG_STREAM_MAX_EARLY, null allowed when n_early is 0).  Elements are io_dtype (WG_F32 / WG_F16) and
 *   copied unchanged.  Every element of the outputs is written, so the result does not depend on what they held.  The
 *   outputs are 16-byte aligned and cols_per_frame is a multiple of 8; noise rows move in 16-byte pieces where the source
 *   (pointer and pitch) is 16-byte aligned too, element by element where it is not.  Nothing outside
 *   [0, pitch) of a source row is read, whatever the table holds; the row counts of the sources are the caller's word.
 * wg_stream_emit, one launch: for row b with c = crops[b], n = c.count clamped to [0, n_max], over i in [0, n):
 *     x = c.raw[c.offset + i], y = c.denoised[c.offset + i] (fp32; the two may be the same array), g = y * c.gain,
 *     pcm_out[b][i] = int16 of round-half-even(clip(g, -1, 1) * 32767) -- convert_wav(np.clip(y * gain, -1, 1), int16) of
 *       audio_utils.py:36-64 in float32 arithmetic, bit for bit; NOT peak-normalised --, pcm_out[b][n:] = 0
 *       (pcm_out is [B][n_max], n_max a multiple of 8, 16-byte aligned);
 *     stats_out[b] = {min x, max x, min y, max y, the number of i with g > 1 or g < -1, f, 0, 0} (8 floats, device);
 *       f = 1 when an x or a y is NaN or infinite, else 0; all 0 for n = 0.  A count above 2^24 is not exact as a float.
 *   Minimum, maximum and an integer count do not depend on the order of the reduction; no atomics.  c.offset must not
 *   be negative (such a row counts as n = 0); offset + count inside the source is the caller's word.
 * Both are enqueue-only. */
#define WG_STREAM_MAX_EARLY 8
typedef struct wg_stream_window {
  const void* mel;                            /* this stream's mel [n_mel][mel_pitch] */
  const void* z_init;                         /* its noise [n_rem][noise_pitch] */
  const void* z_early[WG_STREAM_MAX_EARLY];   /* [n_early_size][noise_pitch] each, descending flow index; the rest unused */
  int64_t mel_pitch;                          /* elements between two mel rows (the buffer's capacity in frames) */
  int64_t noise_pitch;                        /* elements between two noise rows */
  int32_t start;                              /* first mel frame of the window */
  int32_t count;                              /* mel frames of the window */
} wg_stream_window;
typedef struct wg_stream_crop {
  const float* raw;                           /* raw audio of the window */
  const float* denoised;                      /* denoised audio of the window (raw again without a denoiser) */
  int32_t offset;                             /* first sample of the chunk inside the window */
  int32_t count;                              /* samples of the chunk */
  float gain;
  int32_t reserved;                           /* 0 */
} wg_stream_crop;
int wg_stream_gather(const wg_stream_window* windows, void* mel_out, void* z_init_out, void* const* z_early_out,
                     int32_t n_early, int32_t B, int32_t n_mel, int32_t n_mel_out, int32_t n_rem, int32_t n_early_size,
                     int32_t w_max, int32_t cols_per_frame, int32_t io_dtype, void* stream);
int wg_stream_emit(const wg_stream_crop* crops, int16_t* pcm_out, float* stats_out, int32_t B, int32_t n_max,
                   void* stream);

/* ---- Validation metrics of mel-spectrogram pairs (src/waveglow/validation.py:211-235), no handle --------------------
 * Ragged batches: arrays [B][C][tmax] fp32 device, frame counts int32 device [B], read by the kernels only.  A frame
 * count outside [1, min(tmax, 4096)] counts as 0: that utterance's MFCC columns are all 0 and its metrics NaN.  fp64
 * arithmetic without contraction, every sum in a fixed order, no atomics: a call gives the same bits every time, and an
 * utterance of a batch the bits of its own call with B = 1 and tmax = its frame count.  Enqueue-only.
 * wg_metrics_mfcc: mfcc_out[b][k-1][t] = fp32 of sum_{n ascending} mel[b][n][t] sqrt(2/N) cos(pi k (2n+1) / (2N)),
 *   k = 1..n_mfcc, N = n_mel (orthonormal DCT-II over the mel axis without coefficient 0; no logarithm is taken);
 *   0 behind an utterance's frames.  1 <= n_mfcc < n_mel <= 128, 1 <= tmax <= 4096.
 * wg_metrics_dtw: exact dynamic time warping of feat_a[b] [K][tmax_a] against feat_b[b] [K][tmax_b], 1 <= K <= 128,
 *   1 <= tmax <= 4096.  d(i,j) = sqrt(sum_{k ascending} (a[k][i] - b[k][j])^2); C(0,0) = d(0,0), L(0,0) = 1; otherwise
 *   C(i,j) = d(i,j) + C(pred), L(i,j) = L(pred) + 1 with pred the first minimal of (i-1,j), (i,j-1), (i-1,j-1).
 *   cost_out[b] = C(Ta-1, Tb-1) (fp64), frames_out[b] = L(Ta-1, Tb-1) (int32; 0 with a NaN cost for a refused count).
 * wg_metrics_mel: the two above chained on the MFCCs of both mels, plus the padded comparison (F = max(Ta, Tb), the
 *   shorter one's MFCCs / mel 0 behind its end).  rows_out[b] = 8 fp64:
 *     {mcd = mean_t |fa_t - fb_t|_2, penalty = 2 - (Ta+Tb)/F, F, mcd_dtw = C/L, penalty_dtw = 2 - (Ta+Tb)/L, L,
 *      cosine = 1 - mean_c (1 - u.v / (|u| |v|)) over the mel channels (score 1 where |u| |v| = 0), 0}.
 * Workspace: wg_metrics_workspace_bytes (0 for arguments outside the limits) serves all three with the same sizes. */
size_t wg_metrics_workspace_bytes(int32_t B, int32_t n_mel, int32_t n_mfcc, int32_t tmax_a, int32_t tmax_b);
int wg_metrics_mfcc(const float* mel, const int32_t* frames, float* mfcc_out, int32_t B, int32_t n_mel, int32_t n_mfcc,
                    int32_t tmax, void* workspace, size_t workspace_bytes, void* stream);
int wg_metrics_dtw(const float* feat_a, const int32_t* frames_a, const float* feat_b, const int32_t* frames_b,
                   double* cost_out, int32_t* frames_out, int32_t B, int32_t K, int32_t tmax_a, int32_t tmax_b,
                   void* stream);
int wg_metrics_mel(const float* mel_a, const int32_t* frames_a, const float* mel_b, const int32_t* frames_b,
                   double* rows_out, int32_t B, int32_t n_mel, int32_t n_mfcc, int32_t tmax_a, int32_t tmax_b,
                   void* workspace, size_t workspace_bytes, void* stream);

/* ---- Pitch metrics of audio pairs: a YIN F0 tracker and the F0 / voicing errors of two tracks, no handle ------------
 * The reference has no counterpart.  The tracker restates steps 1-5 of de Cheveigne & Kawahara, "YIN, a fundamental
 * frequency estimator for speech and music", JASA 111(4), 2002: difference function (eq. 6), cumulative mean normalised
 * difference (eq. 8), absolute threshold (step 4), parabolic interpolation (step 5).  Step 6, an energy gate, centred
 * frames and any smoothing of the track are not built.
 * Parameters: sampling_rate sr, frame_length W in [16, 2048], hop_length H >= 1, 2 <= tau_min < tau_max <= 1024,
 * 0 < threshold < 1; a caller with a frequency range passes tau_max = ceil(sr / fmin), tau_min = max(2, floor(sr / fmax)).
 * Anything else is WG_ERR_INVALID.
 * Frames: audio [B][N] fp32 device, lens int32 device [B], read by the kernels only; a length outside [0, N] counts as
 *   0 frames.  Utterance b has F_b = (len_b - W - tau_max) / H + 1 frames if len_b >= W + tau_max, else 0 (wg_pitch_frames
 *   gives this count for a length).  Frame t starts at s = t H and reads x[s .. s + W + tau_max - 1]: no padding, no
 *   centring, nothing behind len_b is ever read.
 * Per frame, in fp64 on the fp32 samples, no contraction:
 *   d(tau) = sum_{j = 0 .. W-1 ascending} (x[s+j] - x[s+j+tau])^2, tau = 0 .. tau_max, as written (no autocorrelation
 *     identity);
 *   d'(0) = 1, d'(tau) = d(tau) tau / sum_{k=1..tau} d(k), and 1 where that sum is 0;
 *   pick: the smallest tau in [tau_min, tau_max] with d'(tau) < threshold, then tau += 1 while tau + 1 <= tau_max and
 *     d'(tau+1) < d'(tau).  No such lag: f0 = 0 (unvoiced), aperiodicity = min d' over [tau_min, tau_max].  Otherwise
 *     aperiodicity = d'(tau) and, where tau - 1 >= 1 and tau + 1 <= tau_max, with a, b, c = d'(tau-1), d'(tau), d'(tau+1)
 *     and den = a - 2b + c: shift = (a - c) / (2 den) if den > 0 and |shift| <= 1, else 0; f0 = sr / (tau + shift).
 *   d(tau) is the plain ascending sum; the running sum of d is a scan of fixed shape (it depends on tau_max alone), so a
 *   frame's values depend on its samples and the parameters only: a call gives the same bits every time, an utterance of
 *   a batch the bits of its own call with B = 1 and N = len_b, and audio scaled by a power of two the same tracks.
 * wg_pitch_yin: f0_out, aperiodicity_out [B][fmax] fp64, 0 behind an utterance's frames; frames_out int32 [B].
 *   1 <= B <= 65535, N >= 1, fmax >= max(1, F(N)).
 * wg_pitch_compare: tracks f0_a [B][fmax_a], f0_b [B][fmax_b] with frame counts (a count outside [0, fmax] counts as 0)
 *   -> rows_out[b] = 8 fp64 over the F = min(Fa, Fb) first frames, a frame being voiced where f0 > 0:
 *     {F0_RMSE_CENTS = sqrt(mean over the both-voiced frames of (1200 log2(f0_b / f0_a))^2), F0_RMSE_HZ = the same of
 *      f0_b - f0_a, GPE = share of the both-voiced frames with |f0_b / f0_a - 1| > 0.2, VUV_ERROR = share of the F frames
 *      voiced on exactly one side, FRAMES = F, VOICED_A, VOICED_B, VOICED_BOTH = counts among the F frames}.
 *   The first three are NaN when no frame is voiced on both sides, the first four when F = 0.  A thread sums its frames
 *   ascending, the partial sums are joined by a fixed tree.
 * wg_pitch_metrics: wg_pitch_yin of audio_a [B][n_a] and of audio_b [B][n_b], then wg_pitch_compare of the two tracks,
 *   bit for bit those three calls.  Workspace: wg_pitch_workspace_bytes (0 for arguments outside the limits).
 * Enqueue-only. */
typedef struct wg_pitch_params {
  double sampling_rate, threshold;
  int32_t frame_length, hop_length, tau_min, tau_max;
} wg_pitch_params;
int32_t wg_pitch_frames(const wg_pitch_params* params, int32_t n_samples);   /* F(n_samples), or an error code (< 0) */
size_t wg_pitch_workspace_bytes(const wg_pitch_params* params, int32_t B, int32_t n_a, int32_t n_b);
int wg_pitch_yin(const float* audio, const int32_t* lens, const wg_pitch_params* params, double* f0_out,
                 double* aperiodicity_out, int32_t* frames_out, int32_t B, int32_t N, int32_t fmax, void* stream);
int wg_pitch_compare(const double* f0_a, const int32_t* frames_a, const double* f0_b, const int32_t* frames_b,
                     double* rows_out, int32_t B, int32_t fmax_a, int32_t fmax_b, void* stream);
int wg_pitch_metrics(const float* audio_a, const int32_t* lens_a, int32_t n_a, const float* audio_b, const int32_t* lens_b,
                     int32_t n_b, const wg_pitch_params* params, double* rows_out, int32_t B, void* workspace,
                     size_t workspace_bytes, void* stream);

/* ---- Intelligibility metrics of audio pairs: STOI and ESTOI of 10 kHz audio, no handle --------------------------------
 * The reference has no counterpart.  Short-time objective intelligibility (Taal, Hendriks, Heusdens and Jensen, IEEE TASL
 * 19(7), 2011) and its extended form (Jensen and Taal, IEEE/ACM TASLP 24(11), 2016) as pystoi.stoi(x, y, 10000, extended)
 * computes them, restated; parity with pystoi itself is unpinned.  x is the clean signal, y the
 * processed one; the metric is not symmetric.
 * Constants: fs = 10000, frame W = 256, hop H = 128, NFFT = 512, 15 one-third-octave bands from 150 Hz, segments of N = 30
 *   frames, BETA = -15 dB, dynamic range 40 dB, EPS = 2^-52, window w[i] = 0.5 - 0.5 cos(2 pi (i + 1) / 257), i = 0 .. 255.
 * 1. n = min(len_x, len_y), both cropped to n; all arithmetic from here is fp64 on the fp32 samples.
 * 2. Frame starts range(0, n - W, H): F0 = ceil((n - 256) / 128) frames for n > 256, else 0 (exclusive end: 256 + 128 k
 *    samples have k frames).
 * 3. e[t] = 20 log10(||w x_t||_2 + EPS) on the clean signal; frame t is kept where max(e) - 40 - e[t] < 0.  The K kept
 *    frames of x and the same frames of y, windowed, are overlap-added at hop 128 into x_s, y_s of (K - 1) 128 + 256
 *    samples.
 * 4. x_s, y_s are framed again the same way (F = K - 1 frames for K >= 2, else 0), windowed with w again, zero-padded to
 *    512; band b sums the power at bins lo[b] .. hi[b] - 1, X[b, t] = sqrt(band sum), Y alike.  With f = k fs / 512,
 *    lo[b] = argmin_k (f - 150 2^((2b-1)/6))^2, hi[b] = argmin_k (f - 150 2^((2b+1)/6))^2: bins 7 .. 218 at 10 kHz.
 * 5. J = F - 29 segments m = 30 .. F over X[:, m-30:m], Y[:, m-30:m].
 *    STOI: per band row alpha = ||x|| / (||y|| + EPS), y' = min(alpha y, x (1 + 10^(15/20))); both rows mean-removed and
 *      divided by (their norm + EPS); d = sum x y' / (15 J) over all bands and segments.
 *    ESTOI: both blocks row-normalised (mean removed, divided by norm + EPS), then column-normalised the same way;
 *      d = sum over the segments of (sum x y / 30) / J.
 * 6. F < 30 (no segment) gives NaN for both values, the counts still reported.  Silence gives exactly 0.0 twice.
 * x, y: [B][pitch] fp32 device, 10 kHz.  len_x, len_y: int32 device [B], read by the kernels only; a length outside
 *   [0, pitch] counts as 0.  Nothing at or behind a row's common length n is read (it may hold NaN).
 * params: device pointers to the caller's tables: window fp64 [256]; bands int32 [15][2] = (lo, hi) (the kernels compute
 *   bins 7 .. 218 only and clamp the table to them); cossin fp64 [512][2] = (cos, sin)(2 pi k / 512), aligned to 16 bytes.
 *   The kernels call no device cos or sin.
 * rows_out: fp64 [B][8] = {STOI, ESTOI, F0, K, J, 0, 0, 0}.
 * Arithmetic: every sum is fp64 in a fixed order that depends on the utterance alone, without atomics; products may be
 *   fused into the sums.  A call gives the same bits every time and every utterance of a batch the bits of its own call
 *   with B = 1, whatever the pitch.
 * Limits: 1 <= B <= 65535, 1 <= pitch <= 2^21; anything else is WG_ERR_INVALID before any launch.  Workspace:
 *   wg_stoi_workspace_bytes(B, pitch) (0 for a refused geometry).  Five launches on `stream`.  Enqueue-only. */
typedef struct wg_stoi_params {
  const double* window;
  const int32_t* bands;
  const double* cossin;
} wg_stoi_params;
size_t wg_stoi_workspace_bytes(int32_t B, int32_t n_max);
int wg_stoi(const float* x, const int32_t* len_x, const float* y, const int32_t* len_y, int32_t B, int32_t pitch,
            const wg_stoi_params* params, double* rows_out, void* workspace, size_t workspace_bytes, void* stream);

/* ---- STOI and ESTOI as a training signal: the gradient with respect to the processed signal y --------------------------
 * The energy gate (step 3) depends on the clean signal alone, so with the gate and x held constant both values are
 * differentiable in y; the gradient runs through the definition above, step by step.
 * wg_stoi_forward: wg_stoi -- the same five launches, rows_out bit for bit -- that also leaves in `saved`
 *   (wg_stoi_saved_bytes(B, pitch) bytes, aligned to 8; 0 for a refused geometry) what the backward needs:
 *   [counts int32 [B][4] = (n, F0, K, J) | kept-frame lists int32 [B][F0max] | band spectra fp64 [B][2][15][Fmax], X then Y],
 *   each part aligned to 256 bytes, F0max = max(1, F0(pitch)), Fmax = max(1, F0max - 1).  workspace: as wg_stoi.
 * wg_stoi_backward: y, B, pitch, params and saved as the forward had them; g_rows fp64 [B][2] device, the upstream
 *   gradients of STOI and ESTOI; d_y fp64 [B][pitch] = the gradient of g_rows[b][0] STOI_b + g_rows[b][1] ESTOI_b with
 *   respect to y[b].  Exact zeros at and behind the common length n, in gated frames and behind the last frame; a row
 *   without a segment (J = 0) is all zeros whatever g_rows[b] holds (it is not read).  Nothing at or behind n is read.
 *   Workspace: wg_stoi_backward_workspace_bytes(B, pitch); the backward writes to it and to d_y only, so a second call on
 *   the same saved buffer gives the same bits.  Five launches on `stream`:
 *   the inverse of the kept-frame list; one wave per segment recomputing its 15 x 30 block from the saved X, Y and writing
 *   the block's gradient, weights g0 / (15 J) and g1 / (30 J) folded in; per (band, t) the sum of the at most 30 blocks
 *   that cover it, ascending in m, divided by 2 Y[band, t]; per frame the (re, im) of bins 7 .. 218 recomputed from y as
 *   the forward computes them, d re = 2 re dP, d im = 2 im dP, and d frame[j] = w[j] sum over the bins ascending of
 *   (cos d re + sin d im) from the caller's table; the overlap-add as a gather, one thread per sample of y.
 * Conventions where the definition is not smooth: the gradient through a square root whose argument is exactly 0 is 0
 *   (band sums, row and column norms, ||y|| in alpha), so silence on either side gives exactly zero gradients; at a tie
 *   of min(alpha y, x (1 + 10^(15/20))) the gradient goes to the alpha y branch; alpha is differentiated (it depends on
 *   y); the gate and x are constants.
 * Arithmetic: fp64, every sum in a fixed order that depends on the utterance alone, no atomics; products may be fused
 *   into the sums.  A call gives the same bits every time and every utterance of a batch the bits of its own call with
 *   B = 1, whatever the pitch.  Limits and argument checks as wg_stoi.  Enqueue-only. */
size_t wg_stoi_saved_bytes(int32_t B, int32_t pitch);
size_t wg_stoi_backward_workspace_bytes(int32_t B, int32_t pitch);
int wg_stoi_forward(const float* x, const int32_t* len_x, const float* y, const int32_t* len_y, int32_t B, int32_t pitch,
                    const wg_stoi_params* params, double* rows_out, void* saved, size_t saved_bytes, void* workspace,
                    size_t workspace_bytes, void* stream);
int wg_stoi_backward(const float* y, int32_t B, int32_t pitch, const wg_stoi_params* params, const double* g_rows,
                     const void* saved, size_t saved_bytes, double* d_y, void* workspace, size_t workspace_bytes,
                     void* stream);

/* ---- Soft-DTW: the warped distance of wg_metrics_dtw as a training signal, no handle -----------------------------------
 * Cuturi and Blondel, "Soft-DTW: a differentiable loss function for time-series", ICML 2017; the reference has no
 * counterpart.  Inputs as wg_metrics_dtw: feat_a [B][K][tmax_a], feat_b [B][K][tmax_b] fp32 device, frame counts int32
 * device [B], read by the kernels only; 1 <= K <= 128, 1 <= tmax <= 4096, gamma > 0 and finite; anything else is
 * WG_ERR_INVALID before any launch.  A count outside [1, min(tmax, 4096)] counts as 0: that utterance's value is NaN, its
 * part of E and of both gradients all zeros (g_value[b] is not read), and no other utterance is affected.  Nothing behind
 * a count is read (it may hold NaN).  0-based indices, Ta = frames_a[b], Tb = frames_b[b].
 * Cost: WG_SDTW_L2: d(i,j) = sqrt(sum_{k ascending} (a[k][i] - b[k][j])^2), wg_metrics_dtw's distance bit for bit, so the
 *   value tends to wg_metrics_dtw's cost as gamma -> 0; WG_SDTW_SQ: the same sum without the root (the paper's cost).
 * wg_softdtw_forward: R(0,0) = d(0,0); otherwise R(i,j) = d(i,j) + softmin(R(i-1,j), R(i,j-1), R(i-1,j-1)), a cell outside
 *   the matrix counting as +infinity, softmin(x) = m - gamma log(sum_q exp(-(x_q - m) / gamma)) with m = min x and the sum
 *   in the order written (the quotient is taken as a product with 1 / gamma).  value_out[b] = R(Ta-1, Tb-1), fp64.
 *   r_out: null (values only), or the accumulated-cost matrix for the backward, wg_softdtw_bytes(B, tmax_a, tmax_b) bytes
 *   (0 outside the limits), diagonal-major and skewed:
 *     R(i,j) of pair b at r_out[(b (tmax_a + tmax_b - 1) + (i + j)) tmax_a + i]        for i < Ta, j < Tb;
 *   the other elements are neither written nor, by the backward, read.
 * wg_softdtw_backward: arguments as the forward had them and its r.  E(Ta-1, Tb-1) = 1; otherwise
 *     E(i,j) = sum over s in ((i+1,j), (i,j+1), (i+1,j+1)), in that order, of E(s) exp((R(s) - R(i,j) - d(s)) / gamma),
 *   evaluated as ((R(s) - d(s)) - R(i,j)) times 1 / gamma, a successor outside the matrix left out by predicate (no
 *   inf - inf is formed).  E is the expected alignment:
 *   E(0,0) = 1, 0 <= E <= 1, every row and column sums to at least 1.
 *   e_out: null, or fp64 [B][tmax_a][tmax_b] row-major, written whole: E inside the frames, exact zeros elsewhere.
 *   g_a [B][K][tmax_a], g_b [B][K][tmax_b] fp32, each may be null, written whole (exact zeros behind the frames):
 *     g_a[k][i] = fp32(g_value[b] sum_{j ascending} E(i,j) dd(i,j)/da[k][i]),
 *     g_b[k][j] = fp32(g_value[b] sum_{i ascending} E(i,j) dd(i,j)/db[k][j]),
 *   dd/da = (a - b) / d for L2 and 0 where d = 0 (the library's convention for a root at 0), 2 (a - b) for SQ; the sum
 *   over j runs as 64 interleaved ascending sums (j = l, l + 64, ...) joined by a fixed tree, the sum over i as 8 such sums
 *   (i = w, w + 8, ...) joined as ((0+1)+(2+3))+((4+5)+(6+7)): both orders depend on the utterance's counts alone.
 *   g_value: fp64 [B] device, the upstream gradients of the values; may be null when both g_a and g_b are.
 *   With gradients wanted and e_out null the call takes a temporary of E's size from the stream-ordered allocator
 *   (hipMallocAsync / hipFreeAsync on `stream`); with all three outputs null it does nothing.  The backward writes to its
 *   outputs only, so a second call on the same r gives the same bits.
 * Launches: forward one (one workgroup per pair, one anti-diagonal per step); backward a memset of E, one wavefront launch
 *   and one launch per gradient.  The distances are recomputed by the backward, not stored beside R.
 * Arithmetic: fp64, every sum in a fixed order that depends on the utterance alone, no atomics.  A call gives the same
 *   bits every time and every utterance of a batch the bits of its own call with B = 1 and tmax = its counts.
 *   Enqueue-only. */
#define WG_SDTW_L2 0
#define WG_SDTW_SQ 1
size_t wg_softdtw_bytes(int32_t B, int32_t tmax_a, int32_t tmax_b);
int wg_softdtw_forward(const float* feat_a, const int32_t* frames_a, const float* feat_b, const int32_t* frames_b,
                       double gamma, int32_t cost, double* value_out, double* r_out, int32_t B, int32_t K,
                       int32_t tmax_a, int32_t tmax_b, void* stream);
int wg_softdtw_backward(const float* feat_a, const int32_t* frames_a, const float* feat_b, const int32_t* frames_b,
                        double gamma, int32_t cost, const double* r, const double* g_value, double* e_out, float* g_a,
                        float* g_b, int32_t B, int32_t K, int32_t tmax_a, int32_t tmax_b, void* stream);

/* ---- Soft-DTW inside a Sakoe-Chiba band -------------------------------------------------------------------------------
 * The calls above with the warping restricted to a band around the diagonal, an integer `band` = w in [1, 511] (anything
 * else is WG_ERR_INVALID; w = 0 would disconnect pairs of unequal lengths).  With n = Ta - 1, m = Tb - 1 and
 * W = w max(n, m), cell (i,j) is inside the band iff |i m - j n| <= W, in integer arithmetic (it fits int32 within the
 * limits): |i - j| <= w for Ta = Tb, otherwise the band around the line from (0,0) to (n,m).  A cell outside the band
 * counts as +infinity, exactly as a cell outside the matrix; everything else in the recursions for R and E, the gradient
 * formulas, the frame-count rule and the arithmetic is the text above, with the terms of cells outside the band left out
 * of the gradient sums (the order of the remaining terms is unchanged, so it depends on the counts and w alone).
 * (0,0) and (n,m) are inside the band, every in-band cell has an in-band predecessor and all but (n,m) an in-band
 * successor.  On the anti-diagonal d = i + j the in-band rows are the interval lo(d) .. hi(d),
 *     lo(d) = max(0, d - m, ceil((d n - W) / (n + m))),   hi(d) = min(n, d, floor((d n + W) / (n + m)))      (n + m > 0),
 *   of at most 2 w + 1 rows; lo and hi advance by 0 or 1 per diagonal.  With w >= min(n, m) the band is the whole matrix
 *   and every output has the bits of the dense call.
 * wg_softdtw_banded_bytes: B (tmax_a + tmax_b - 1) S 8 with S = min(2 band + 1, tmax_a); 0 outside the limits.
 * r_out / r: diagonal-major, S slots per diagonal:
 *     R(i,j) of pair b at r[(b (tmax_a + tmax_b - 1) + (i + j)) S + (i - lo_b(i + j))]   for (i,j) inside the band,
 *   lo_b from the pair's own counts; the other elements are neither written nor read.
 * wg_softdtw_banded_backward: e_out null, or fp64 [B][tmax_a][tmax_b] written whole: E inside the band, exact zeros
 *   elsewhere.  With gradients wanted the call takes a temporary of wg_softdtw_banded_bytes for E in the layout of r from
 *   the stream-ordered allocator; e_out is filled only when given.
 * Launches: forward one (one workgroup of P threads per pair, P the smallest power of two >= 2 w + 2, at least 64);
 *   backward a memset of e_out if given, one wavefront launch and one launch per gradient. */
size_t wg_softdtw_banded_bytes(int32_t B, int32_t tmax_a, int32_t tmax_b, int32_t band);
int wg_softdtw_banded_forward(const float* feat_a, const int32_t* frames_a, const float* feat_b, const int32_t* frames_b,
                              double gamma, int32_t cost, double* value_out, double* r_out, int32_t B, int32_t K,
                              int32_t tmax_a, int32_t tmax_b, int32_t band, void* stream);
int wg_softdtw_banded_backward(const float* feat_a, const int32_t* frames_a, const float* feat_b, const int32_t* frames_b,
                               double gamma, int32_t cost, const double* r, const double* g_value, double* e_out,
                               float* g_a, float* g_b, int32_t B, int32_t K, int32_t tmax_a, int32_t tmax_b, int32_t band,
                               void* stream);
/* The soft-DTW divergence (Blondel, Mensch and Vert, "Differentiable divergences between time series", AISTATS 2021) is
 * D_b = v_ab - 0.5 (v_aa + v_bb) in fp64, in exactly that form, each v the value of that pair under the same gamma, cost
 * and band; NaN where any of the three is.  It is composed by the caller (waveglow_amd/softdtw.py: soft_dtw_divergence)
 * from one forward and one backward call over 3 B pairs. */

/* ---- Resampling by a rational ratio: wav data of any sampling rate in, any rate out, no handle ------------------------
 * The reference has no counterpart.  The definition is scipy.signal.resample_poly(x, up, down) with its defaults
 * (window ('kaiser', 5.0), padtype 'constant') in closed form.  With up / down reduced, M = max(up, down), half = 10 M and
 * h = up * firwin(2 half + 1, 1 / M, window=('kaiser', 5.0)) in fp64:
 *   out_len(len) = ceil(len up / down)
 *   y[n] = sum over m ascending, 0 <= m < len with 0 <= half + n down - m up <= 2 half, of x[m] h[half + n down - m up].
 * Limits: 1 <= up, down <= 1024, gcd(up, down) = 1, 0 <= half <= 10240, B >= 1, 1 <= n_in <= 2^26, out_len(n_in) < 2^31;
 * anything else is WG_ERR_INVALID before any launch.  All index arithmetic (n down, m up) is 64-bit.
 * in: [B][n_in] device, fp32 (WG_PCM_F32) or int16 (WG_PCM_I16; converted as (float)x * (1.0f / 32768.0f), as in
 *   wg_data_gather).  lens: int32 device [B], read by the kernel only; a length outside [0, n_in] counts as 0.  Nothing at
 *   or behind in[b][lens[b]] is read (it may hold NaN).
 * taps: the caller's h as a polyphase table on the device, fp64 [up][K] with K = ceil((2 half + 1) / up) and every row
 *   reversed: taps[p][j] = h[p + (K - 1 - j) up], 0 where that index exceeds 2 half.  One output's taps are one row, read
 *   in ascending j, which is ascending m.  The library does not compute h: a caller with another filter passes its own.
 * out: [B][n_out] fp32, out_len(n_in) <= n_out <= 2^31 - 1 - 1024; row b holds out_len(lens[b]) samples and zeros behind them up to n_out.
 * Arithmetic: each product is an fp32 sample widened to fp64 times an fp64 tap, the sum is fp64 in ascending m over the
 *   terms of the definition only and is rounded to fp32 once; no contraction, no atomics.  A call gives the same bits
 *   every time, and every row of a batch the bits of its own call with B = 1 and n_in = lens[b]; the tile
 *   (wg_resample_plan) and the kernel variant do not enter the arithmetic.
 * flags: WG_RESAMPLE_CLIP clamps the fp32 result to [-1, 1] as y < -1 ? -1 : (y > 1 ? 1 : y) (a NaN stays a NaN): a
 *   band-limited copy of full-scale audio overshoots 1.
 * up == down == 1 copies (or converts int16) and zero-fills behind the length: the bits of the input.
 * wg_resample_plan: the argument checks of wg_resample alone, and (each pointer may be null) out_len(n_in), K, the number
 *   of consecutive outputs one workgroup computes and whether the workgroups of this ratio stage their samples in LDS (1)
 *   or read them through the cache (0: down / up above about 7, and the copy).  No workspace is needed.  One launch.
 *   Enqueue-only. */
#define WG_RESAMPLE_CLIP 1
int wg_resample_plan(int32_t up, int32_t down, int32_t half, int32_t n_in, int32_t* out_len, int32_t* taps_per_phase,
                     int32_t* tile, int32_t* staged);
int wg_resample(const void* in, int32_t in_dtype, const int32_t* lens, float* out, const double* taps, int32_t up,
                int32_t down, int32_t half, int32_t flags, int32_t B, int32_t n_in, int32_t n_out, void* stream);

/* ---- The transpose of wg_resample: the gradient of a loss computed at another rate -------------------------------------
 *   d_in[m] = sum over n ascending, 0 <= n < out_len(lens[b]) with 0 <= half + n down - m up <= 2 half, of
 *             d_out[n] h[half + n down - m up],
 * the gradient with respect to in[b][m] of sum_n d_out[n] out[b][n] for the unclipped wg_resample (there is no clipped
 * variant).  up, down, half, B, n_in, n_out, lens and their limits as in wg_resample.
 * d_out: [B][n_out] device, fp32 (WG_PCM_F32) or fp64 (WG_PCM_F64).  Nothing at or behind d_out[b][out_len(lens[b])] is
 *   read (it may hold NaN).
 * d_in: [B][n_in] fp32, written for m < lens[b] and exact zeros behind.
 * taps_t: the caller's h as a second polyphase table on the device, fp64 [down][Kt] with Kt = ceil((2 half + 1) / down):
 *   taps_t[r][i] = h[r + i down], 0 where that index exceeds 2 half.  With c = half - m up, r = c mod down (non-negative)
 *   and n0 = (r - c) / down, input m is sum_i d_out[n0 + i] taps_t[r][i]: one input's taps are one row, read in ascending
 *   i, which is ascending n.
 * Arithmetic: each product is a gradient widened to fp64 times an fp64 tap, the sum is fp64 in ascending n over the terms
 *   of the definition only and is rounded to fp32 once; no contraction, no atomics.  A call gives the same bits every
 *   time, and every row of a batch the bits of its own call with B = 1; the tile (1024 consecutive inputs per workgroup)
 *   and the kernel variant (the span of d_out staged in LDS, or read through the cache for up / down above about 4) do not
 *   enter the arithmetic.
 * up == down == 1 copies (an fp64 gradient is rounded to fp32) and zero-fills behind the length.  One launch, no
 *   workspace.  Enqueue-only. */
int wg_resample_backward(const void* d_out, int32_t d_out_dtype, const int32_t* lens, float* d_in, const double* taps_t,
                         int32_t up, int32_t down, int32_t half, int32_t B, int32_t n_in, int32_t n_out, void* stream);

/* ---- Multi-resolution STFT loss (spectral convergence + log-magnitude L1), fp32, with its backward ------------------
 * For resolution r = (n_fft, hop, win): X = STFT(x) with reflect padding by n_fft/2 and the window of `win` samples
 * centred in n_fft, M = sqrt(max(re^2 + im^2, eps)); sc_r = |M(y) - M(x)|_F / |M(y)|_F over the whole batch,
 * mag_r = mean |log M(y) - log M(x)|; sc = mean_r sc_r, mag = mean_r mag_r.
 * wg_stftloss_create: 1..8 resolutions; n_fft a multiple of 32 in [32, 2048], 1 <= hop <= n_fft, 1 <= win <= n_fft;
 *   fwd_basis[r] is the windowed Fourier basis [2*(n_fft/2+1)][n_fft] (real rows, then imaginary rows), HOST pointers,
 *   packed once.  device_id < 0 makes a planning handle (no device work, fwd_basis may be null): workspace sizes only.
 * wg_stftloss_workspace_bytes: 0 unless B >= 1 and n_samples > max n_fft / 2.  saved = 0 sizes wg_stftloss_forward with
 *   saved = 0, saved = 1 sizes wg_stftloss_forward with saved = 1 + wg_stftloss_backward (one workspace serves both).
 * wg_stftloss_forward: audio, target [B][n_samples] fp32 device -> out3 = {sc, mag, factor_sc sc + factor_mag mag} fp32
 *   device.  saved = 1 also keeps the prediction's (re, im), M(target) and the two norms in the workspace; saved = 0
 *   gives the same out3 bits and keeps nothing.  Any other value is WG_ERR_INVALID.
 * wg_stftloss_backward: g_out3 [3] fp32 DEVICE = d loss / d out3 -> audio_grad_out [B][n_samples] = d loss / d audio
 *   (no gradient under the clamp, sign(0) = 0).  Reads the workspace of a forward call with saved = 1 and the same lens,
 *   factors, B and n_samples and leaves its saved state intact, so it may run more than once.
 * With `lens`, utterances of DIFFERENT lengths inside the dense [B][n_samples] arrays: a device array of B sample counts,
 *   read by the kernels only.  Utterance b is transformed as its own crop x[b][:lens[b]] (reflect padding about its own
 *   last sample, F_b = lens[b] / hop + 1 frames); the norms of sc_r run over the frames f < F_b of every utterance and
 *   mag_r divides by K sum_b F_b, formed on the device: the loss of the cropped utterances with their frames
 *   concatenated.  audio_grad_out[b][lens[b]:] = 0.  A length outside (max n_fft / 2, n_samples] counts as 0: that
 *   utterance contributes nothing, gets a zero gradient row, and nothing is indexed with it; if every length counts as
 *   0, out3 and the gradient are zeros.  The workspace is that of (B, n_samples).  With every length equal to n_samples
 *   the results are bit for bit those of a null lens.  lens == NULL: every row has n_samples samples.
 * Sums are reduced in a fixed order (no floating-point atomics): results are bit-reproducible.  Enqueue-only; argument
 * checks (null arguments and sizes, then the workspace size, then the refusal of a planning handle with WG_ERR_STATE) run
 * before any device work. */
typedef struct wg_stftloss wg_stftloss;
int wg_stftloss_create(int32_t n_res, const int32_t* n_fft, const int32_t* hop, const int32_t* win,
                       const float* const* fwd_basis, float eps, int32_t device_id, wg_stftloss** out);
int wg_stftloss_destroy(wg_stftloss* h);
size_t wg_stftloss_workspace_bytes(const wg_stftloss* h, int32_t B, int32_t n_samples, int32_t saved);
int wg_stftloss_forward(wg_stftloss* h, const float* audio, const float* target, const int32_t* lens, float factor_sc,
                        float factor_mag, float* out3, int32_t B, int32_t n_samples, int32_t saved, void* workspace,
                        size_t workspace_bytes, void* stream);
int wg_stftloss_backward(wg_stftloss* h, const float* g_out3, const int32_t* lens, float factor_sc, float factor_mag,
                         float* audio_grad_out, int32_t B, int32_t n_samples, void* workspace, size_t workspace_bytes,
                         void* stream);

/* ---- Multi-scale mel-spectrogram loss (log-mel L1 + linear-mel L1), fp32, with its backward ---------------------------
 * HiFi-GAN's mel L1 in the multi-scale form of DAC and BigVGAN; the reference has no counterpart.  For scale
 * r = (n_fft, hop, win, n_mels) with the dense bank W_r [n_mels][n_fft/2 + 1]: X = STFT(x) as in the STFT loss above (the
 * same transform), M = sqrt(re^2 + im^2) with one rounding per operation, mel = W_r M, lmel = ln(max(mel, clamp));
 * log_r = mean |lmel(x) - lmel(y)|, lin_r = mean |mel(x) - mel(y)| over the n_mels sum_b F_b cells of the batch;
 * log = mean_r log_r, lin = mean_r lin_r, loss = factor_log log + factor_lin lin.
 * Gradient: sign(0) = 0; the log term passes nothing where mel(x) < clamp; a bin with re^2 + im^2 = 0 gets 0, never NaN;
 * only the prediction gets one.
 * wg_melloss_create: 1..8 scales; n_fft a multiple of 32 in [32, 2048], 1 <= hop, win <= n_fft,
 *   1 <= n_mels <= n_fft/2 + 1, clamp > 0 and finite; anything else is WG_ERR_INVALID.  fwd_basis[r] is the windowed
 *   Fourier basis [2*(n_fft/2+1)][n_fft] (real rows, then imaginary rows) and mel_basis[r] the bank [n_mels][n_fft/2+1],
 *   HOST pointers, packed once.  The projection multiplies a row of the bank from its first to its last non-zero bin
 *   (a row of zeros is legal) and, in the backward, a bin over the rows whose span covers it, both in ascending index
 *   order.  device_id < 0 makes a planning handle (no device work, both bases may be null): buffer sizes only.
 * wg_melloss_spectra_elems / wg_melloss_mels_elems: the number of floats of the two saved buffers, 0 unless
 *   1 <= B <= 65535 and n_samples > max n_fft / 2.  With F = n_samples / hop + 1 frames and Fp = F rounded up to 64:
 *     spectra: scale after scale, each block rounded up to 64 floats, the prediction's transform [B][n_fft][Fp] with
 *       rows interleaved: row 0 = re of bin 0, row 1 = re of bin n_fft/2, rows 2p and 2p + 1 = (re, im) of bin p,
 *       1 <= p < n_fft/2;
 *     mels: scale after scale, the prediction's linear mels [B][n_mels][Fp] rounded up to 64 floats, then the target's
 *       in the same form; behind the last scale 64 floats that hold fp64 [8], element r the cell count
 *       n_mels sum_b F_b of scale r (the only reduced sum the backward needs).
 *   Columns f >= F_b of either buffer are neither written nor read.  Both buffers must be 8-byte aligned.
 * wg_melloss_forward: audio, target [B][n_samples] fp32 device -> out3 = {log, lin, loss} fp32 device.  lens: null, or a
 *   device array of B sample counts, read by the kernels only: utterance b is then its own crop x[b][:lens[b]] (reflect
 *   padding about its own last sample, F_b = lens[b] / hop + 1 frames), nothing behind a length is read (it may hold NaN)
 *   and the cell count is formed on the device.  A length outside (max n_fft / 2, n_samples] counts as 0: that utterance
 *   contributes nothing and nothing is indexed with it; if every length counts as 0, out3 is zeros.  With every length
 *   equal to n_samples the results are bit for bit those of a null lens.  spectra and mels may be null only together:
 *   values only, the same out3 bits, nothing saved.
 * wg_melloss_backward: g_out3 [3] fp32 DEVICE = d loss / d out3, the lens, factors, B and n_samples of the forward and
 *   its spectra and mels -> audio_grad_out [B][n_samples] = d loss / d audio, written whole, exact zeros behind a length.
 *   It reads the saved buffers and writes neither, so a second call gives the same bits.
 * Temporaries (the target's transform, per-workgroup sums, the gradient planes) come from the stream-ordered allocator
 *   (hipMallocAsync / hipFreeAsync on `stream`).  Every loss sum is reduced in fp64 per thread, per workgroup and in one
 *   final kernel in a fixed order, overlapping frames are summed per sample in ascending frame order, no floating-point
 *   atomics: results are bit-reproducible.  Enqueue-only; argument checks (null arguments and sizes, then the refusal
 *   of a planning handle with WG_ERR_STATE) run before any device work. */
typedef struct wg_melloss wg_melloss;
int wg_melloss_create(int32_t n_scales, const int32_t* n_fft, const int32_t* hop, const int32_t* win,
                      const int32_t* n_mels, const float* const* fwd_basis, const float* const* mel_basis,
                      float clamp, int32_t device_id, wg_melloss** out);
int wg_melloss_destroy(wg_melloss* h);
size_t wg_melloss_spectra_elems(const wg_melloss* h, int32_t B, int32_t n_samples);
size_t wg_melloss_mels_elems(const wg_melloss* h, int32_t B, int32_t n_samples);
int wg_melloss_forward(wg_melloss* h, const float* audio, const float* target, const int32_t* lens,
                       float factor_log, float factor_lin, float* out3, float* spectra, float* mels,
                       int32_t B, int32_t n_samples, void* stream);
int wg_melloss_backward(wg_melloss* h, const float* g_out3, const int32_t* lens, float factor_log,
                        float factor_lin, const float* spectra, const float* mels, float* audio_grad_out,
                        int32_t B, int32_t n_samples, void* stream);

/* ---- Training direction: WaveGlow.forward under autograd and loss.backward() ---------------------------------------
 * (src/waveglow/model.py:178-221, train.py:190-199).  Weights change every optimiser step, so they are NOT taken from
 * the handle: the caller passes device buffers.  Every fp16 matrix below is given as [rows][K] in "(pos,pos)" order
 * -- rows and K columns permuted inside 32-blocks so that position 16h+4g+i holds channel 8g+4h+i -- and then laid out
 * in MFMA-fragment order [K/64][rows/32][4][64 lanes][8]: lane (r = lane&31, h = lane>>5), element j of sub-step s,
 * block b, K-step t = Mat[32b + pos(r)][64t + 32h + 8s + j]  (wg_train_prepare fills the struct from the module's own
 * parameter tensors: weight norm, the folds below and every layout in one pass per tensor on the device).
 * Gradients come back in natural channel order (wg_train_grads).
 * C = n_channels, M8 = 8*n_mel_channels, fl = flow*n_layers + layer, K1 = 3C + M8, h_k / c_k per flow.
 * Needs only wg_create (no wg_set_tensor / wg_finalize). */
typedef struct wg_train_weights {
  /* Forward (one fused launch per WN layer, the inference kernel's structure).  MFMA A-fragment order of that kernel:
   * NW = wg_wn_waves(C) waves own MB = C/(32 NW) channel blocks each; M tile mt < MB = tanh rows of block w*MB+mt,
   * mt >= MB = sigmoid rows (+C) of block w*MB+mt-MB; lane (r = lane&31, hh = lane>>5) element j of k16 step
   * 2*(u&1)+k2 of half K-step u holds  W[row 32*blk + r][64*(u>>1) + 32*(u&1) + 16*k2 + 8*hh + j]  -- rows in NATURAL
   * channel order, K in position order (tap-major: tap0 | tap1 | tap2, then the cond_layer slice).  The tanh rows and
   * bias entries are pre-scaled by 2*log2(e), the sigmoid rows by -log2(e) (the gate works on exp2). */
  const void* a1;      /* fp16 [FL][2*3C/64][NW][2MB][2][64][8]   in_layers (model.py:98-102) */
  const void* a1c;     /* fp16 [FL][2*M8/64][NW][2MB][2][64][8]   cond_layer slice of the layer (model.py:121-128) */
  const float* b1;     /* [FL][2C]  (in_layers.bias + cond_layer.bias slice), natural order, pre-scaled */
  const void* a2;      /* fp16 [FL][NW][MB][C/16][64][8]   res rows of res_skip_layers (model.py:131-134): lane (r, hh)
                          element j of k16 step k = W_res[32*blk + r][16k + 8hh + j]; last layer of a flow unused */
  const float* b2;     /* [FL][C] natural order */
  const void* es;      /* fp16 [FL][C/32][64][8]  end x skip fold W_end.W_skip_i [8][C]: lane (row = lane&15, l4 = lane>>4)
                          element j of step s = hi (row < 8) / lo (row >= 8) fp16 half of  Wes[row&7][32s + 8 l4 + j] */
  /* Backward dgrad GEMMs on the same kernel (plain row blocks: [FL][2*K/64][NW][MB][2][64][8], lane (r, hh) element j of
   * k16 step 2*(u&1)+k2 of half K-step u = Mat[32*blk + r][64*(u>>1) + 32*(u&1) + 16*k2 + 8*hh + j], rows natural, K in
   * the position order of the planes it multiplies): */
  const void* wat;     /* fp16, Mat [C][C+64] = [ W_res^T | (W_end.W_skip_i)^T hi halves, padded to 64 ]  (K: d x positions,
                          then the d out plane's 64 channels) */
  const void* wbt;     /* fp16, Mat [C][6C]   = W_in[:, :, tap]^T for tap 0, 1, 2  (K per tap: the 2C d-pre positions) */
  /* ... and on the plane GEMM: [rows][K] in "(pos,pos)" order, fragment order [K/64][rows/32][4][64][8]: lane (r, h)
   * element j of sub-step s of block b, K-step t = Mat[32b + pos(r)][64t + 32h + 8s + j] */
  const void* wct;     /* fp16 [M8][FL*2C]    cond_layer^T of every layer */
  const void* wup;     /* fp16 [32][M8][512]  upsample per phase p: row (o,g) , K = [tap j][128]: W_up[i][o][8p+g+256j] */
  const float* bup;    /* [M8]                upsample.bias[o] repeated over g */
  const float* const* wstart;    /* n_flows pointers: [C][h_k] fp32 */
  const float* const* bstart;    /* [C] */
  const float* const* out_init;  /* [8]   W_end.(sum_i b_skip_i) + b_end, zero padded */
  const float* const* w1x1;      /* [c_k][c_k] fp32 row-major (model.py:64) */
  /* Optional (null: not packed, not read): the upsample transposed for the mel input gradient (wg_train_backward with
   * g_mel), fp16 [32 p][4 j][M8/64 t][NB][4 s][64 lanes][8] with NB = ceil(n_mel/32): lane (r, h), element e of sub-step
   * s = W_up[i = 32 blk + r][o][8p + g + 256j] for the spectrogram channel (o, g) = 8o + g at d spect plane position
   * 64t + 32h + 8s + e (zero for i >= n_mel).  wg_train_prepare fills it when it is non-null. */
  const void* wupt;
  /* Optional (null: not filled, not read): n_flows pointers to [c_k][c_k] fp32 row-major W_k^-1 of the 1x1 matrices.
   * wg_train_prepare fills them when the member is non-null: an fp64 Gauss-Jordan elimination with partial pivoting on the
   * device, rounded to fp32 (a singular or non-finite matrix gives non-finite entries, never a host sync).  The synthesis
   * calls (wg_train_infer_*) then take the inverses from here instead of from the finalised handle, so a model whose
   * weights move every optimiser step needs no wg_finalize between steps. */
  const float* const* winv;
} wg_train_weights;

/* Gradients: fp32 device buffers in NATURAL channel order, w.r.t. the stacked natural-order matrices (dw1, dw2, dwes,
 * dwup) and the natural-order bias vectors; wg_train_param_grads turns them into one gradient per parameter. */
typedef struct wg_train_grads {
  float* dw1;          /* [FL][2C][K1]   in_layers[i].weight as K = tap*C + c_in (tap-major), then the layer's cond_layer rows [M8] */
  float* db1;          /* [FL][2C] */
  float* dw2;          /* [FL][C][C]     res rows of res_skip_layers[i] (last layer of each flow: untouched) */
  float* db2;          /* [FL][C] */
  float* dwes;         /* [FL][8][C]     the effective end x skip matrix W_end . W_skip_i, zero padded to 8 rows */
  float* dwup;         /* [32][M8][512]  upsample per phase p: row (o,g), K = [tap j][128]: W_up[i][o][8p+g+256j] */
  float* dbup;         /* [M8] */
  float* const* dstart;      /* n_flows pointers: [5][C]: rows j < 4 = d Wstart[:, j] (zero for j >= h_k), row 4 = d bstart */
  float* const* dout_init;   /* [8] */
  float* const* dw1x1;       /* [8][8], top-left [c_k][c_k] used: the W.z term only; the logdet term (model.py:63) is
                                the caller's */
  /* Record layout of dw1 / db1 / dw2 / db2 / dwes (elements of float).  Both 0: every tensor is dense, entry fl at
   * fl * (its own size).  Otherwise entry fl = flow*n_layers + layer of each of the five lies at
   * base + flow*flow_stride + layer*layer_stride: a data-parallel caller interleaves the five tensors of a layer in one
   * record and the records of a flow (plus its dstart / dout_init / dw1x1) in one contiguous region, so that a flow's
   * gradients travel as ONE all-reduce message (waveglow_amd/train.py: GradBuffers). */
  int64_t layer_stride;
  int64_t flow_stride;
} wg_train_grads;

/* Flag of the training entry points below (flags = 0: every activation is kept).
 * WG_TRAIN_RECOMPUTE: activation recomputation.  The workspace keeps the layer planes (X / T / S / A / d pre) of two flow
 *   slots (flow k in slot k & 1) instead of every flow, plus every flow's fp32 state as before; the backward replays each
 *   flow's forward into its slot just before that flow's data-gradient chain (the last two flows the forward ran are still
 *   there and are not replayed) and computes d spect flow by flow into an fp32 accumulator.  About 0.2x the workspace at
 *   256 channels for about one more forward pass of the WN layers.  Outputs of the forwards and every gradient except those
 *   that go through d spect (upsample weight / bias, d mel: summation order, <= 3e-5 relative) are bit-identical to flags = 0.
 *   A workspace keeps one layout from its forward to its backward: where the recompute size is below the full-save size,
 *   the workspace of a recompute call must be smaller than the full-save size and at least the recompute size, and a call
 *   whose flags do not match the size it is given returns WG_ERR_INVALID.  At a depth where the flag saves nothing (one or
 *   two flows: the two slots hold every flow; one layer per flow) it runs all the same, on a workspace of
 *   wg_train_workspace_bytes(..., WG_TRAIN_RECOMPUTE) bytes, which is then no smaller than the full-save one. */
#define WG_TRAIN_RECOMPUTE 1

/* Bytes of device workspace the four calls below need for batch B, n_frames mel frames and audio_len samples per
 * utterance (a multiple of n_group, at most what n_frames upsample to; the synthesis calls: 256 * n_frames), with the
 * flags of those calls.  0 on invalid arguments or unknown flags; wg_last_error() says which. */
size_t wg_train_workspace_bytes(const wg_handle* h, int32_t B, int32_t n_frames, int32_t audio_len, int32_t flags);

/* ---- Training plumbing on the device: the module's OWN parameter tensors in, one gradient per parameter out.  Weight
 * norm, stacking, the W_end x W_skip fold and their backward run here, not in the caller's autograd: reference modules WN.start / in_layers / cond_layer / res_skip_layers
 * (torch weight_norm: w = g v / ||v||, model.py:85-113), WN.end (model.py:90-92), Invertible1x1Conv.conv
 * (model.py:29-43), WaveGlow.upsample (model.py:145-150).
 * The parameters come in the library's canonical order: wg_train_param_count / _name (the state_dict key of the
 * reference's module tree: "...parametrizations.weight.original0|1" for weight-normed modules, "...weight" otherwise,
 * weight_normed selects which) / _numel.  All tensors fp32, contiguous, in their native layouts. */
int32_t wg_train_param_count(const wg_handle* h, int32_t weight_normed);
const char* wg_train_param_name(const wg_handle* h, int32_t weight_normed, int32_t i);   /* valid until the next call on this thread */
int64_t wg_train_param_numel(const wg_handle* h, int32_t weight_normed, int32_t i);
/* Scratch the two calls below share (row norms, W_end x W_skip, pointer tables): must stay untouched between a
 * wg_train_prepare and the wg_train_param_grads of the same step. */
size_t wg_train_prepare_bytes(const wg_handle* h);
/* Fills EVERY member of *out (fragment tensors and the small fp32 vectors; all buffers caller-allocated with the
 * sizes documented on wg_train_weights) from params[i] = device pointer of canonical parameter i.  Enqueue-only. */
int wg_train_prepare(wg_handle* h, const void* const* params, int32_t weight_normed, const wg_train_weights* out, void* aux,
                     size_t aux_bytes, void* stream);
/* From the packed gradients that wg_train_backward left in *grads to one gradient per parameter: flat[offset_i ..
 * offset_i + numel_i) with offset_i = sum of the numel of the canonical parameters before i.  The 1x1 weights get the
 * W.z term only (the logdet term, model.py:63, is the caller's).  Enqueue-only. */
int wg_train_param_grads(wg_handle* h, const void* const* params, int32_t weight_normed, const wg_train_grads* grads, void* aux,
                         size_t aux_bytes, float* flat, void* stream);

/* Waves per workgroup of the WN-layer kernel for n_channels (the NW of the fragment orders above); 0 = unsupported. */
int32_t wg_wn_waves(int32_t n_channels);

/* Forward with saved activations.  mel [B][n_mel][n_frames] fp32, audio [B][audio_len] fp32 (audio_len % 8 == 0),
 * z [B][8][L] fp32 out, log_s[k] [B][h_k][L] fp32 out.  `fresh` != 0: the workspace has not been used with this
 * geometry before (it is cleared: guard rows must read as zero).  The workspace (wg_train_workspace_bytes with the same
 * flags) must stay untouched until wg_train_backward has run.  flags: 0 or WG_TRAIN_RECOMPUTE (only the last two flows'
 * layer planes stay in the workspace).  Enqueue-only.  At large batch the call also enqueues on streams the handle owns:
 * they are forked from `stream` inside the call and joined back into it before it returns, so the caller sees ordinary
 * stream order.  Environment: WG_TRAIN_SERIAL=1 keeps every launch on `stream` (timing single kernels);
 * WG_TRAIN_HALVES=1|2 never / always runs the forward as two half-batch chains. */
int wg_train_forward(wg_handle* h, const wg_train_weights* w, const void* mel, const void* audio, float* z,
                     float* const* log_s, int32_t B, int32_t n_frames, int32_t audio_len, int32_t fresh,
                     void* workspace, size_t workspace_bytes, int32_t flags, void* stream);

/* Backward of the last wg_train_forward on this workspace, with the flags of that forward: loss.backward() of the
 * reference's plain autograd (src/waveglow/model.py:178-221), after which the parameters and the inputs hold gradients.
 * g_z [B][8][L] (or null), g_log_s[k] [B][h_k][L] (null entries = zero) are the gradients of the returned tensors;
 * `scale` (> 0) multiplies them on entry (fp16 gradient planes) and is divided out of every result.
 *   grads   the packed parameter gradients, or null: no parameter gradient is computed at all (a frozen model used as a
 *           likelihood loss): no weight-gradient launch, slab reduction, start / 1x1 partial or upsample-gradient job
 *           runs, and the d spect GEMM only for g_mel.
 *   g_mel   null, or fp32 [B][n_mel][n_frames]: d loss / d mel through the upsample and squeeze (model.py:186-193); frames
 *           whose spectrogram columns were trimmed to audio_len (model.py:188-189) get 0.  Needs w->wupt.
 *   g_audio null, or fp32 [B][audio_len]: d loss / d audio through the unfold and flow 0's 1x1 conv (model.py:195, :64).
 *   flow_hi, flow_lo   the pass cut at flow boundaries: the call processes flows flow_hi, flow_hi-1, ..., flow_lo
 *           (0 <= flow_lo <= flow_hi < n_flows); calls must come in descending, contiguous order starting at n_flows-1.
 *           flow_hi = n_flows - 1, flow_lo = 0, flags = 0 is the whole plain pass.  After a call returns, the gradient
 *           slices of its flows (dw1[fl], db1[fl], dw2[fl], db2[fl], dwes[fl] for fl in [flow_lo*n_layers,
 *           (flow_hi+1)*n_layers), dstart / dout_init / dw1x1 of those flows) are final on `stream` -- a data-parallel
 *           caller can start their all-reduce while the earlier flows are still being computed (waveglow_amd/train.py).
 *           The call with flow_lo == 0 also produces the upsample gradients, and g_mel / g_audio, both written entirely
 *           (no accumulation), are final on `stream` after it.
 *   flags   WG_TRAIN_RECOMPUTE: every call of a flow range replays the flows of its range; the call with flow_lo == 0
 *           finishes d spect (upsample gradients, g_mel).
 * Enqueue-only.  Like the forward, the call forks streams the handle owns from `stream` (the weight-gradient launches
 * and their reductions run on two low-priority ones) and joins them back before it returns; WG_TRAIN_SERIAL=1 keeps
 * everything on `stream`. */
int wg_train_backward(wg_handle* h, const wg_train_weights* w, const wg_train_grads* grads, const float* g_z,
                      const float* const* g_log_s, float scale, const void* audio, float* g_mel, float* g_audio,
                      int32_t B, int32_t n_frames, int32_t audio_len, void* workspace, size_t workspace_bytes,
                      int32_t flow_hi, int32_t flow_lo, int32_t flags, void* stream);

/* Differentiable synthesis: WaveGlow.infer with injected noise (src/waveglow/model.py:223-273) with saved state, and its
 * backward w.r.t. mel, the noise and the weights.  Both run on the training workspace of the same geometry,
 * wg_train_workspace_bytes(h, B, n_frames, 256 * n_frames, flags) (infer's trim to 256 T samples is forward's crop to
 * audio_len), and on the wg_train_weights of wg_train_prepare (with wupt for g_mel).  The inverse 1x1 matrices are
 * w->winv when it is given; otherwise those wg_infer uses: the handle must then be finalised with the same weights
 * (WG_ERR_STATE otherwise).
 *
 * Forward: mel [B][n_mel][n_frames] fp32, z_init [B][c_last][L] fp32, z_early[i] [B][n_early_size][L] fp32 in descending
 * flow order (as wg_infer), audio [B][256 n_frames] fp32 out; L = 32 n_frames.  `fresh`, flags (WG_TRAIN_RECOMPUTE: flows
 * 1 and 0 stay in the two slots) and the streams as for wg_train_forward.  The workspace must stay untouched until
 * wg_train_infer_backward has run.  Enqueue-only.
 *
 * With `frames` (both calls), a batch of utterances of DIFFERENT lengths: a device array of B mel-frame counts as in
 * wg_infer; same workspace.  Utterance b is mel[b, :, :frames[b]] with z_init[b, :, :32 frames[b]] and
 * z_early[i][b, :, :32 frames[b]], synthesised alone (src/waveglow/model.py:223-273 on that utterance; the reference has
 * no ragged mode, its convolutions' zero padding at the end of a sequence, model.py:98-102, is what the padding columns
 * stand for):
 *   forward   audio[b, :256 frames[b]] has the bits of the batch-of-one call on the utterance, audio behind it is 0.
 *   backward  g_mel, g_z_init and g_z_early[i] are 0 behind the count and have the bits of the batch-of-one call (same
 *             scale) in front of it; every entry of `grads` is the sum over the utterances of the batch-of-one calls'
 *             (up to accumulation order).  The backward takes the counts of its forward.
 * Nothing behind an utterance's count is read: mel, noise and g_audio may hold NaN there.  The counts are never read on
 * the host and nothing synchronises: a count <= 0 makes its utterance all padding (zero audio, zero gradients, nothing
 * added to `grads`), a count above n_frames counts as n_frames; neither reads or writes outside the buffers.
 * With counts the forward clears the workspace's planes on every call, whatever `fresh` says (the layer kernels leave
 * padding columns unwritten, and a reused workspace may hold another batch there).
 * frames == NULL: every utterance has n_frames frames. */
int wg_train_infer_forward(wg_handle* h, const wg_train_weights* w, const void* mel, const void* z_init,
                           const void* const* z_early, int32_t n_z_early, float sigma, float* audio, int32_t B,
                           int32_t n_frames, const int32_t* frames, int32_t fresh, void* workspace,
                           size_t workspace_bytes, int32_t flags, void* stream);

/* Backward of the last wg_train_infer_forward on this workspace, with the flags and `frames` of that forward
 * (WG_TRAIN_RECOMPUTE: flows 2.. are replayed).  g_audio [B][256 n_frames] fp32 is the gradient of the returned audio;
 * `scale` (> 0) multiplies it on entry (fp16 gradient planes) and is divided out of every result.  Flows in ascending order.
 * Outputs, each optional (null: not computed) and written entirely (no accumulation): g_mel [B][n_mel][n_frames],
 * g_z_init [B][c_last][L], g_z_early[i] [B][n_early_size][L] (g_z_early itself or any entry may be null).
 *   grads   null: the data gradients alone, on `stream` alone.  Otherwise also the gradients of the weights through
 *           synthesis (the vocoder trained on a loss on its own output): the packed gradients of wg_train_grads are filled
 *           as wg_train_backward fills them -- dw1 | db1 | dw2 | db2 | dwes per layer, dstart, dout_init per flow, the
 *           upsample tail -- and dw1x1[k] = - sum over rows of (W_k^-T d w) (x) w for the inverse 1x1 step w = W_k^-1 u
 *           (an [8][8] record, rows / columns >= c_k zero; this direction has no logdet term); wg_train_param_grads turns
 *           them into one gradient per parameter.  Every entry is written except dw2 / db2 of the last layer of each
 *           flow.  The forward must have run on the same wg_train_weights; with a moving model that means one prepared
 *           with winv.  The weight-gradient launches and their reductions run on two low-priority streams the handle
 *           owns, forked from `stream` inside the call and joined back into it before it returns, as in
 *           wg_train_backward (WG_TRAIN_SERIAL=1: everything on `stream`; same results bit for bit).
 * The d spect GEMM runs when g_mel or grads is given.  Enqueue-only. */
int wg_train_infer_backward(wg_handle* h, const wg_train_weights* w, const wg_train_grads* grads,
                            const float* g_audio, float scale, float sigma, float* g_mel, float* g_z_init,
                            float* const* g_z_early, int32_t n_z_early, int32_t B, int32_t n_frames,
                            const int32_t* frames, void* workspace, size_t workspace_bytes, int32_t flags, void* stream);

/* Diagnostic builds only (-DWG_STAMPS): device buffer of n_tiles*8 uint64 that the WN-layer kernel fills with
 * s_memtime stamps at its phase boundaries (last launch wins).  A no-op pointer in the shipped library. */
int wg_debug_set_stamp_buffer(wg_handle* h, void* device_buffer);

#ifdef __cplusplus
}
#endif
#endif /* WAVEGLOW_AMD_H */
