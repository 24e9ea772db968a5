/* vvtts.h -- C ABI of the MI355X-native VietVoice-TTS synthesis hot path (libvvtts_hip.so).
 *
 * The reference has no FFI: its hot path is three onnxruntime sessions driven from Python
 *   preprocess : vietvoicetts/core/tts_engine.py:133-146  (sessions['preprocess'].run)
 *   transformer: vietvoicetts/core/tts_engine.py:148-174  (sessions['transformer'].run, 31 calls)
 *   decode     : vietvoicetts/core/tts_engine.py:176-187  (sessions['decode'].run)
 * created in vietvoicetts/core/model.py:65-129.  This header is what a binding for that path
 * would bind instead (INTEGRATION.md shows the ctypes stub): plain pointers and sizes, no torch
 * types, every call returns 0 or a negative errno-style code, the message is read with
 * vv_last_error(); nothing aborts or throws across the ABI.  All pointers named *device* are
 * HBM addresses on the context's GPU; `stream` is a hipStream_t passed as void*.
 * One context per GPU; calls on one context must be serialised by the caller
 * (reference threading: vietvoicetts/api/tts_engine.py:64-87).
 */
#ifndef VVTTS_H
#define VVTTS_H
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* exported entry points: the library is built with -fvisibility=hidden, only these symbols leave it */
#if defined(__GNUC__)
#define VV_API __attribute__((visibility("default")))
#else
#define VV_API
#endif

#define VV_DTYPE_F32 0
#define VV_DTYPE_BF16 1
#define VV_MAX_UP 8
#define VV_MAX_RES 4

/* activation codes (gemm epilogue) */
#define VV_ACT_NONE_ 0
#define VV_ACT_GELU_TANH_ 1
#define VV_ACT_GELU_ERF_ 2
#define VV_ACT_SILU_ 3
#define VV_ACT_MISH_ 4
/* gemm epilogue modes */
#define VV_EPI_STORE 0     /* C = act(A W^T + bias)                         */
#define VV_EPI_QKV_ROPE 1  /* C = rope(A W^T + bias) on the q and k columns */
#define VV_EPI_GATE_RES 2  /* C += gate * (A W^T + bias)   (fp32 residual)  */
#define VV_EPI_GATE_STORE 3 /* C = gate * (A W^T + bias); the add is fused into the next vv_layernorm (delta) */

typedef struct vv_ctx vv_ctx;

/* Architecture constants (the reference hides them in the ONNX graphs). */
typedef struct vv_model_cfg {
    int32_t n_mel, n_fft, win_length, hop_length;
    int32_t dim, depth, heads, head_dim, ff_mult;
    int32_t text_dim, text_layers, text_conv_k, text_ff_mult, vocab_rows;
    int32_t pos_conv_k, pos_conv_groups, time_freq_dim;
    float cfg_strength;
    int32_t voc_pre_ch, voc_pre_k, voc_post_k;
    int32_t voc_n_up, voc_up_rates[VV_MAX_UP], voc_up_kernels[VV_MAX_UP];
    int32_t voc_n_res, voc_res_kernels[VV_MAX_RES];
    int32_t voc_n_dil, voc_res_dilations[VV_MAX_RES];
    float voc_lrelu;
    int32_t max_pos; /* rows of the rope / text position tables */
} vv_model_cfg;

/* N6: the Vocos decoder (ConvNeXt backbone + ISTFT head) in place of the HiFi-GAN generator.  vv_model_cfg is ABI and
 * stays as it is; a context is switched to Vocos with vv_set_vocos between vv_create and vv_finalize_weights. */
typedef struct vv_vocos_cfg {
    int32_t dim, intermediate, layers;   /* backbone width (% 128, <= 1024), ConvNeXt intermediate width (% 128), block count */
    int32_t embed_k, dw_k;               /* odd kernel sizes of the embed conv and of the depthwise convs */
    float ln_eps;                        /* every LayerNorm of the backbone */
    int32_t n_fft, win_length, hop_length;   /* the ISTFT: n_fft == win_length == the model's n_fft (% 128), hop == the model's hop */
} vv_vocos_cfg;

/* ---- context ------------------------------------------------------------------------------ */
/* replaces onnxruntime.InferenceSession creation, core/model.py:96-102 */
VV_API int vv_create(vv_ctx** out, int device, const vv_model_cfg* cfg, int acoustic_dtype);
VV_API void vv_destroy(vv_ctx* ctx);
VV_API const char* vv_last_error(const vv_ctx* ctx);   /* ctx may be NULL: last create error */
VV_API const char* vv_version(void);

/* Bind one named tensor of the (already uploaded) flat weight buffer.  Layouts: DESIGN.md 3. */
VV_API int vv_bind_weight(vv_ctx* ctx, const char* name, const void* device_ptr, uint64_t bytes);
/* Verify every tensor the three stages need is bound (names listed in the error if not). */
VV_API int vv_finalize_weights(vv_ctx* ctx);

/* Select the Vocos decoder for this context (fp32 whatever the acoustic dtype).  Only between vv_create and the first
 * vv_finalize_weights, which then checks the Vocos tensor names (voc.embed / voc.norm / voc.blocks.{i}.* / voc.final_norm / voc.head,
 * const.istft_basis; layouts DESIGN.md 3) instead of the HiFi-GAN ones.  -22 otherwise, and for a cfg the kernels cannot run.
 * vv_decode / vv_decode_into / vv_decode_ws_bytes then run Vocos: pcm_len[b] = hop * max(T_b - 1, 0) (centred ISTFT) where the
 * HiFi-GAN gives hop * T_b; samples from pcm_len[b] up to t_gen_max * hop are written as zeros. */
VV_API int vv_set_vocos(vv_ctx* ctx, const vv_vocos_cfg* cfg);

/* ODE time grid: sinus[n_steps][time_freq_dim] (host), dt[n_steps] (host).  Runs the time MLP and
 * every block's AdaLN projection once on the GPU and keeps the modulation tables in HBM. */
VV_API int vv_set_time_grid(vv_ctx* ctx, const float* sinus_host, const float* dt_host, int n_steps, void* stream);

/* N7 ODE plan: vv_set_time_grid generalised to an explicit Runge-Kutta method with s <= 4 stages.  a [s * s] row-major
 * and strictly lower triangular, b [s]; sinus [n_steps * s][time_freq_dim] holds one row per EVALUATION (step n, stage i at row
 * n * s + i: the embedding of t_n + c_i h_n, c_i = sum_j a[i][j]), dt [n_steps] the step sizes h_n (all host).  n_steps * s <= 512.
 * -22 for a tableau that is not strictly lower triangular, not finite, or whose weights do not sum to 1 (|sum b - 1| < 1e-6), for
 * s outside [1, 4] and for too many evaluations; the plan in force then stays as it was.  vv_set_time_grid is the s = 1 case.
 * vv_transformer_steps* keep counting ODE steps; each runs s evaluations, and with s > 1 vv_transformer_ws_bytes grows by the stage
 * state and up to s - 1 slope buffers ([rows][n_mel] fp32 each). */
VV_API int vv_set_ode_plan(vv_ctx* ctx, const float* sinus_host, const float* dt_host, int n_steps, int s, const double* a,
                           const double* b, void* stream);

/* N20 multistep plan: an Adams-Bashforth method on vv_set_time_grid's tables.  sinus [n_steps][time_freq_dim] and dt
 * [n_steps] as vv_set_time_grid takes them (ONE evaluation per step, at t_n); beta [n_steps][q] (host, row-major), j = 0 the newest
 * slope: step n computes x += h_n * sum_j beta[n][j] f_{n-j}, f_n the combined velocity of the step (after guidance and the projected
 * term), f_{n-1}, f_{n-2} kept from the steps before in q - 1 slope buffers per lane ([rows][n_mel] fp32, a ring; reported by the
 * vv_transformer_*_ws_bytes queries).  A weight that reaches behind the call's first step must be 0 (model_spec.multistep_weights: the
 * order at step n is min(q, n + 1)).  -22 for q outside [1, 3], a weight that is not finite, a row that does not sum to 1
 * (|sum - 1| < 1e-6) or reaches behind step 0; the plan in force then stays as it was.  vv_set_time_grid and vv_set_ode_plan clear it.
 * The kept slopes live for one call: under this plan every vv_transformer_steps* call starts at step0 = 0 (-22 otherwise). */
VV_API int vv_set_ode_multistep(vv_ctx* ctx, const float* sinus_host, const float* dt_host, int n_steps, int q, const double* beta,
                                void* stream);
/* N20 step report: report (device, [n_steps][B][2] float64, caller-owned) receives per step n and item b {D2, F2} = {sum (f_n - f_{n-1})^2,
 * sum f_n^2} over the item's rows and the n_mel columns, from every later vv_transformer_steps* call under a multistep plan whose batch
 * is B items (-22 from that call when its B or the plan's n_steps differ); step 0 stores {0, F2}.  Two small launches per step and lane
 * and one more slope buffer per lane.  report NULL: off (the default); setting a plan turns it off as well. */
VV_API int vv_set_ode_report(vv_ctx* ctx, double* report, int n_steps, int B);

/* ---- the three stages (device-resident, batched) ------------------------------------------ */
/* replaces sessions['preprocess'].run, core/tts_engine.py:133-146.
 * audio [B][ld_audio] int16, audio_len[B], text_ids [B][ld_text] int32, text_len[B], seq_len[B]
 * (= max_duration per item, frames), N = padded frame count (>= every seq_len).
 * Outputs: cat_mel_text, cat_mel_text_drop [B][N][n_mel+text_dim] f32, ref_signal_len[B] int32.
 * (noise is supplied by the caller, or drawn on the device by vv_noise_fill; the rope tables are slices of the bound constant tables.) */
VV_API int vv_preprocess(vv_ctx* ctx, int B, int N, const int16_t* audio, int ld_audio, int max_audio_len,
                  const int32_t* audio_len, const int32_t* text_ids, int ld_text, const int32_t* text_len,
                  const int32_t* seq_len, float* cat_mel_text, float* cat_mel_text_drop,
                  int32_t* ref_signal_len, void* stream);

/* The same call with the clip lengths also handed over on the HOST (same values as the device array).  A centred STFT reflects
 * n_fft / 2 samples at both ends of a clip, which is defined only for clips of more than n_fft / 2 samples (the reference admits
 * any clip, core/audio_processor.py:15-26, core/tts_engine.py:46-56; torch.stft refuses a shorter one): this form returns -22
 * for such an item before anything is launched.  Without host lengths (vv_preprocess) the mel kernel clamps the doubly reflected
 * index -- finite, deterministic, defined by no reference. */
VV_API int vv_preprocess_h(vv_ctx* ctx, int B, int N, const int16_t* audio, int ld_audio, int max_audio_len,
                    const int32_t* audio_len, const int32_t* audio_len_host, const int32_t* text_ids, int ld_text,
                    const int32_t* text_len, const int32_t* seq_len, float* cat_mel_text, float* cat_mel_text_drop,
                    int32_t* ref_signal_len, void* stream);

/* ---- N5 speech editing: regenerate chosen spans of an existing clip (F5-TTS's edit_mask), the rest conditioned frame by frame.
 * The host plans the edit on the hop grid (vietvoice-tts_amd/speech_edit.py); these three calls run it with the stages above:
 *   vv_edit_splice -> vv_preprocess_edit -> vv_transformer_steps_h -> vv_edit_restore -> vv_decode (ref_signal_len = 0).
 *
 * Splice: out [B][ld_out] int16 (8-byte aligned, ld_out % 4 == 0) from source clips in HBM.  desc = n_rows x 4 int64 (device)
 * {item, src_off, dst_off, n}: out[item][dst_off + k] = src[src_off + k] for k < n.  Every output sample is written exactly once:
 * copied where a row covers it, 0 elsewhere (the spans to regenerate and everything past the clip).  The rows live in device
 * memory, so the library cannot check them: the CALLER validates them before the call (0 <= item < B, src_off + n <= n_src,
 * dst_off + n <= ld_out, the rows of one item disjoint on the output; runtime.HipSynth.edit_splice does). */
VV_API int vv_edit_splice(vv_ctx* ctx, const int16_t* src, int64_t n_src, const int64_t* desc, int n_rows, int B, int16_t* out,
                          int ld_out, void* stream);
/* The preprocess stage of an edit: the arguments of vv_preprocess_h plus keep [B][ld_keep] uint8 (device, ld_keep >= N).
 * cat_mel_text[b][t] = [mel(audio_b)[t] where keep[b][t] and t < audio_len[b] / hop + 1, else 0 | text(b)] -- the frame mask in place
 * of the reference prefix; cat_mel_text_drop exactly as vv_preprocess builds it; ref_signal_len[b] = 0. */
VV_API int vv_preprocess_edit(vv_ctx* ctx, int B, int N, const int16_t* audio, int ld_audio, int max_audio_len,
                              const int32_t* audio_len, const int32_t* audio_len_host, const int32_t* text_ids, int ld_text,
                              const int32_t* text_len, const int32_t* seq_len, float* cat_mel_text, float* cat_mel_text_drop,
                              int32_t* ref_signal_len, const uint8_t* keep, int ld_keep, void* stream);
/* After the last Euler step: x[b][t][0:n_mel] = cat_mel_text[b][t][0:n_mel] wherever keep[b][t] and t < seq_len[b], bit for bit
 * (x [B][N][n_mel], cat_mel_text [B][N][n_mel + text_dim], both 16-byte aligned; keep as above). */
VV_API int vv_edit_restore(vv_ctx* ctx, int B, int N, float* x, const float* cat_mel_text, const uint8_t* keep, int ld_keep,
                           const int32_t* seq_len, void* stream);

/* ---- N9 start noise on the device.  The reference's preprocess graph returns `noise` itself (core/tts_engine.py:133-146,
 * 229-230); this call fills x [B][N][n_mel] f32 (16-byte aligned, n_mel % 4 == 0) with it.  Philox4x32-10: key = the 64-bit seed (low word
 * k0, high word k1), counter = (q, 0, stream_lo, stream_hi); element e = t * n_mel + m of item b lies in group q = e >> 2 and takes output
 * word e & 3.  keys = device [B][2] uint64 {seed, stream}: a value is a pure function of (seed, stream, t, m), whatever the batch, N or
 * the padding, and a captured hipGraph replays with new keys without a new capture.  Word w -> u = ((w >> 9) + 0.5f) * 2^-23 (exact in
 * fp32, in (0, 1)); kind 0 = normals by Box-Muller on the word pairs (0, 1) and (2, 3): r = sqrtf(-2 logf(u0)), z0 = r cospif(2 u1),
 * z1 = r sinpif(2 u1); kind 1 = the four uniforms themselves (exact tests).  Rows t >= clamp(seq_len[b], 0, N) are written as +0.0f.
 * -22, and nothing is launched, for n_mel % 4 != 0, a misaligned x, B < 1, N < 1, a kind outside {0, 1}, a null pointer, or N * n_mel / 4
 * > 2^32 (the counter word q); the context stays usable. */
VV_API int vv_noise_fill(vv_ctx* ctx, int B, int N, int n_mel, float* x, const int32_t* seq_len,
                         const uint64_t* keys /* device [B][2] = {seed, stream} */, int kind /* 0 normal, 1 uniform */, void* stream);

/* replaces the loop over sessions['transformer'].run, core/tts_engine.py:148-174: n_steps Euler
 * steps of the flow ODE starting at step index step0, state x [B][N][n_mel] f32 updated in HBM.
 * rope tables are [>=N][head_dim] f32 (q tables carry the softmax scale).
 * Under a plan of more than one stage (vv_set_ode_plan) a step is one Runge-Kutta step of s evaluations; step0 and n_steps of
 * every form below keep counting ODE steps, and a step is never split between calls. */
VV_API int vv_transformer_steps(vv_ctx* ctx, int B, int N, const int32_t* seq_len, float* x, const float* cat_mel_text,
                         const float* cat_mel_text_drop, const float* rope_cos_q, const float* rope_sin_q,
                         const float* rope_cos_k, const float* rope_sin_k, int step0, int n_steps, void* stream);

/* The same call with the per-item lengths also handed over on the HOST (same values as the device array): the host needs them
 * for the launch shapes, so vv_transformer_steps reads them back (one 4*B-byte copy + stream synchronisation per call); this form
 * has no synchronisation at all and can be captured into a hipGraph once the context arena is large enough. */
VV_API int vv_transformer_steps_h(vv_ctx* ctx, int B, int N, const int32_t* seq_len, const int32_t* seq_len_host, float* x,
                           const float* cat_mel_text, const float* cat_mel_text_drop, const float* rope_cos_q, const float* rope_sin_q,
                           const float* rope_cos_k, const float* rope_sin_k, int step0, int n_steps, void* stream);

/* replaces sessions['decode'].run, core/tts_engine.py:176-187: frames [ref_len, seq_len) of x ->
 * vocoder -> int16 PCM.  pcm [B][ld_pcm], ld_pcm >= t_gen_max*hop; pcm_len[B] = samples per item.
 * wave_f32 (optional, [B][t_gen_max*hop]) receives the pre-quantisation waveform. */
VV_API int vv_decode(vv_ctx* ctx, int B, int N, const float* x, const int32_t* ref_signal_len, const int32_t* seq_len,
              int t_gen_max, int16_t* pcm, int ld_pcm, int32_t* pcm_len, float* wave_f32, void* stream);

/* vv_transformer_steps_h with every intermediate carved from a CALLER-OWNED device block `ws` (256-byte aligned, >=
 * vv_transformer_ws_bytes for the same B, N and host lengths) instead of the context arena: no allocation, no synchronisation and
 * nothing that can move -- the form to capture into a hipGraph (all Euler steps of an utterance + vv_decode_into as ONE graph
 * launch: the single-utterance latency path).  No reference counterpart (the reference pays a host round trip per step,
 * core/tts_engine.py:157-172). */
VV_API int vv_transformer_ws_bytes(vv_ctx* ctx, int B, int N, const int32_t* seq_len_host, uint64_t* bytes);
VV_API int vv_transformer_steps_into(vv_ctx* ctx, int B, int N, const int32_t* seq_len, const int32_t* seq_len_host, float* x,
                              const float* cat_mel_text, const float* cat_mel_text_drop, const float* rope_cos_q,
                              const float* rope_sin_q, const float* rope_cos_k, const float* rope_sin_k, int step0,
                              int n_steps, void* ws, uint64_t ws_bytes, void* stream);

/* One struct-argument entry for the transformer stage: every argument of vv_transformer_steps_into plus a guidance strength PER
 * ITEM.  seq_len_host NULL = the lengths are read back (vv_transformer_steps); ws NULL = the context arena (a ws needs the host
 * lengths); cfg_item NULL = vv_model_cfg.cfg_strength for every item, else a device array [B] of fp32 strengths (item b's slope is
 * p_c + (p_c - p_u) * cfg_item[b]).  A zero-initialised struct plus the fields of the positional entries behaves as they do. */
typedef struct vv_steps_args {
    int32_t B, N;
    const int32_t* seq_len;           /* device [B] */
    const int32_t* seq_len_host;      /* host [B], optional */
    float* x;                         /* [B][N][n_mel] f32, updated in place */
    const float* cat_mel_text;
    const float* cat_mel_text_drop;
    const float* rope_cos_q; const float* rope_sin_q; const float* rope_cos_k; const float* rope_sin_k;
    int32_t step0, n_steps;           /* ODE steps of the plan in force (vv_set_ode_plan / vv_set_time_grid) */
    void* ws; uint64_t ws_bytes;      /* optional caller-owned workspace (>= vv_transformer_ws_bytes, 256-byte aligned) */
    const float* cfg_item;            /* optional device [B] */
} vv_steps_args;
VV_API int vv_transformer_steps_ex(vv_ctx* ctx, const vv_steps_args* args, void* stream);

/* N8 guidance interval: vv_transformer_steps_ex with a guidance MASK.  guide_host is a HOST array
 * [evaluations of the plan in force][ld_guide] of uint8, ld_guide >= B: row e = step * s + stage (the plan's ABSOLUTE evaluation index, so
 * calls split by step0 / n_steps read the same table), column b != 0 = item b is guided at evaluation e.  A guided item's slope is
 * p_c + (p_c - p_u) * g_b as in every other entry; an item that is not guided has the slope p_c and NO unconditional rows at that
 * evaluation: per lane the conditional rows stay at [0, Rc) and the unconditional rows of the guided items alone are packed behind them,
 * so an evaluation costs Rc + Ru_e rows instead of 2 Rc (nothing is launched on zero rows).  Every other row's arithmetic is that of the
 * unmasked call, bit for bit.  guide_host NULL = every item guided everywhere: the call IS vv_transformer_steps_ex.  The mask is read
 * during the call only (it reaches the device as kernel arguments): with host lengths the call never synchronises and can be captured
 * into a hipGraph.  A caller-owned ws holds vv_transformer_guided_ws_bytes bytes: vv_transformer_ws_bytes plus the row tables of the
 * subsets, the same figure whatever the mask.  -22 for ld_guide < B, for more than 1024 items, and for a mask while option
 * "split_k_tail" is on (its tail plan depends on the row count); a refused call launches nothing and leaves the context usable. */
VV_API int vv_transformer_steps_guided(vv_ctx* ctx, const vv_steps_args* args, const uint8_t* guide_host, int ld_guide, void* stream);
VV_API int vv_transformer_guided_ws_bytes(vv_ctx* ctx, int B, int N, const int32_t* seq_len_host, uint64_t* bytes);

/* N11 adaptive projected guidance (APG): vv_transformer_steps_guided where the two predictions of a guided item are
 * combined as k = p_c + A_b D + C_b d, D = p_c - p_u, d = x_e + (1 - t_e) p_c the conditional data estimate at the state x_e the DiT was
 * evaluated at.  Over the item's valid frames and the n_mel columns: S1 = sum D d, S2 = sum d d, S3 = sum D D, n = frames * n_mel;
 * s = r_b / ((1 - t_e) sqrt(S3 / n)) where r_b > 0 and that RMS exceeds it, else 1; A_b = g_b s; C_b = g_b s (eta_b - 1) S1 / S2 (0 when
 * S2 == 0): the part of the difference parallel to d is scaled by eta_b, its data-space RMS capped at r_b.  eta / norm_rms: device [B]
 * fp32, NULL = 1 / no cap for every item; an item with eta 1 and !(r > 0) gets the bits of the plain rule, an item that is not guided at an
 * evaluation has k = p_c and nothing is reduced for it.  t_host: HOST [evaluations of the plan in force] fp32, the evaluation times t_e the
 * plan's sinusoids were made from (row e = step * s + stage; read during the call only).  The sums are float64, deterministic and independent
 * of the item's place in the batch (no atomics); every evaluation adds two small launches to the stage kernel's.  apg NULL: the call IS
 * vv_transformer_steps_guided.  A caller-owned ws holds vv_transformer_apg_ws_bytes bytes (the same figure whatever the mask).  -22 for
 * what vv_transformer_steps_guided refuses and for a missing t_host; no readback, no synchronisation. */
#define VV_APG_TILE 32   /* frames per partial sum, counted from the item's frame 0 */
typedef struct vv_apg_args {
    const float* eta;        /* device [B], optional */
    const float* norm_rms;   /* device [B], optional */
    const float* t_host;     /* host [evaluations] */
} vv_apg_args;
VV_API int vv_transformer_steps_apg(vv_ctx* ctx, const vv_steps_args* args, const uint8_t* guide_host, int ld_guide, const vv_apg_args* apg,
                                    void* stream);
VV_API int vv_transformer_apg_ws_bytes(vv_ctx* ctx, int B, int N, const int32_t* seq_len_host, uint64_t* bytes);

/* N21 guidance reuse: vv_transformer_steps_guided with a THIRD mask value.  guide_host[e * ld_guide + b] is 0 = item b
 * is not guided at evaluation e (N8), 1 = guided and p_u COMPUTED, 2 = guided and the guidance difference D = p_c - p_u REUSED: the item
 * has no unconditional rows at that evaluation (exactly like an unguided one: per lane Rc + Ru_e rows, Ru_e the rows of the items with a
 * 1) and its slope is p_c + D g_b with the D stored at the item's latest evaluation of the same call that had a 1 and the fresh p_c.  D
 * lives in one [Rc][n_mel] fp32 buffer per lane of the call's workspace and does not outlive the call; it is stored only at evaluations
 * some later one reads it from (or at every computed one under a report).  A computed row's arithmetic is N8's bit for bit.
 * reuse (optional): report != NULL asks for the drift report, a caller-owned DEVICE array [n_evals][B][2] float64 with n_evals the
 * evaluations of the plan in force and B the call's: row (e, b) of an evaluation of the call is {sum (D_new - D_stored)^2, sum D_new^2}
 * over the item's valid frames and the n_mel columns where b is computed at e (the first sum 0 at its first computed evaluation of the
 * call), {0, 0} where it reuses or is not guided; rows of evaluations outside the call are not written.  float64, deterministic,
 * independent of the item's place in the batch (vv_cfg_drift_reduce); two small launches per evaluation and lane in front of the stage
 * kernel's, none without a report.
 * A mask without a 2 and no report: the call IS vv_transformer_steps_guided (same launches, same workspace).  Otherwise a caller-owned ws
 * holds vv_transformer_reuse_ws_bytes bytes: the guided figure plus one D buffer per lane, plus the report's partial sums when
 * with_report != 0 -- the same figure whatever the mask.  -22, nothing launched and the context left usable, for: a mask value above 2; a 2
 * at an evaluation of the call for an item with no 1 at an earlier evaluation of the same call; a mask with a 2 and step0 != 0; a report
 * whose report_B / report_evals are not the call's B and the plan's evaluations; and whatever vv_transformer_steps_guided refuses.  There
 * is no reuse together with projected guidance (vv_transformer_steps_apg takes no such argument).  The mask reaches the device as kernel
 * arguments: with host lengths the call does not synchronise and can be captured into a hipGraph. */
typedef struct vv_reuse_args {
    double* report;                   /* device [report_evals][report_B][2] float64, optional */
    int32_t report_B, report_evals;
} vv_reuse_args;
VV_API int vv_transformer_steps_reuse(vv_ctx* ctx, const vv_steps_args* args, const uint8_t* guide_host, int ld_guide, const vv_reuse_args* reuse,
                                      void* stream);
VV_API int vv_transformer_reuse_ws_bytes(vv_ctx* ctx, int B, int N, const int32_t* seq_len_host, int with_report, uint64_t* bytes);

/* N23 block caching: vv_transformer_steps_ex where a span [first, last) of the DiT blocks is skipped at chosen
 * evaluations.  X_l is the fp32 residual stream at the entry of block l (X_depth: what the final norm reads), formed per element as the
 * LayerNorm kernel forms it: (xres + (float)d_attn) + (float)d_mlp with the two pending deltas of block l - 1, fp32 adds in this order, or
 * plain xres at l = 0.  modes_host is a HOST array of n_modes = [evaluations of the plan in force] uint8, row e = step * s + stage:
 *   0 FULL           the evaluation of vv_transformer_steps_ex, launch for launch;
 *   1 FULL + STORE   the same, bit for bit, plus two read-only launches per lane (or branch view): buf = X_first in front of block `first`,
 *                    buf = X_last - buf (one fp32 subtraction) in front of block `last`, or of the final norm when last = depth;
 *   2 LIGHT          blocks 0 ... first - 1 run, then xres = X_first + buf (one fp32 add, nothing pending behind it), then blocks last ...
 *                    depth - 1 and the tail; blocks first ... last - 1 launch nothing.
 * buf is one fp32 [R][D] plane per lane (R its packed rows of both CFG branches) of the call's workspace and does not outlive the call.
 * report (optional): a caller-owned DEVICE array [report_evals][report_B][2][2] float64, report_evals the evaluations of the plan and
 * report_B the call's B: at an evaluation of the call with mode 1, item b, branch c (0 conditional, 1 unconditional) it holds
 * {sum (buf_new - buf_prev)^2, sum buf_new^2} over the item's valid frames and the D columns (the first sum 0 at the first store of the
 * call), {0, 0} at every other evaluation of the call; rows of evaluations outside the call are not written.  float64, deterministic,
 * independent of the item's place in the batch (vv_block_drift_reduce).  With a report the workspace holds a second plane (the stores
 * alternate between the two) and the partial sums.
 * Every mode 0 and no report: the call IS vv_transformer_steps_ex (same launches, same workspace).  Otherwise a caller-owned ws holds
 * vv_transformer_cached_ws_bytes bytes: the vv_transformer_ws_bytes figure plus one plane per lane, plus the second plane and the partial
 * sums when with_report != 0 -- the same figure whatever the schedule.  -22, nothing launched and the context left usable, for: a mode
 * above 2; a 2 at an evaluation of the call with no 1 at an earlier evaluation of the same call; a 2 in a call with step0 != 0; first /
 * last outside 0 <= first < last <= depth; n_modes other than the plan's evaluations; a report whose report_B / report_evals are not the
 * call's B and the plan's evaluations; option "split_k_tail" (its tail rows keep fp32 parts instead of a delta); and whatever
 * vv_transformer_steps_ex refuses.  There is no mask, no APG and no reuse argument on this entry: a guided subset moves the unconditional
 * rows between evaluations, which the stored rows do not follow.  The schedule reaches the device as launches alone: with host lengths
 * the call does not synchronise and can be captured into a hipGraph. */
#define VV_BLOCK_FULL 0
#define VV_BLOCK_STORE 1
#define VV_BLOCK_LIGHT 2
typedef struct vv_block_cache_args {
    int32_t first, last;              /* the span [first, last) of blocks */
    const uint8_t* modes_host;        /* host [n_modes] */
    int32_t n_modes;
    double* report;                   /* device [report_evals][report_B][2][2] float64, optional */
    int32_t report_B, report_evals;
} vv_block_cache_args;
VV_API int vv_transformer_steps_cached(vv_ctx* ctx, const vv_steps_args* args, const vv_block_cache_args* cache, void* stream);
VV_API int vv_transformer_cached_ws_bytes(vv_ctx* ctx, int B, int N, const int32_t* seq_len_host, int with_report, uint64_t* bytes);

/* N24 CFG-Zero* and guidance rescale: vv_transformer_steps_guided where the two predictions of a guided item are
 * combined as k = f_b (p_c + (p_c - s_b p_u) g_b).  Over the item's valid frames and the n_mel columns of the fp32 predictions:
 * S_cu = sum p_c p_u, S_uu = sum p_u^2, S_cc = sum p_c^2, S_c = sum p_c, S_u = sum p_u, n = frames * n_mel.  s_b = S_cu / S_uu where
 * star[b] != 0 and S_uu != 0, else 1 (Fan et al. 2025: the unconditional velocity projected onto the conditional one), rounded to fp32
 * once.  With a = 1 + g_b, c = -g_b s_b, V_xy = S_xy / n - (S_x / n)(S_y / n) and var_k = a^2 V_cc + 2 a c V_cu + c^2 V_uu:
 * rho = sqrt(V_cc / var_k) (1 unless both are > 0), f_b = phi_b rho + (1 - phi_b) with phi_b = rescale[b], exactly 1 where that is 0,
 * rounded to fp32 once (Lin et al. 2024, applied to the guided VELOCITY, not to an x_0 prediction).  star / rescale: device [B] fp32,
 * NULL = off for every item; an item with s = 1 and f = 1 gets the bits of the plain rule, an item that is not guided at an evaluation
 * has k = p_c and nothing is reduced for it.  report (optional): a caller-owned DEVICE array [evaluations of the plan in force][B][2] fp32
 * that receives the (s, f) used at every evaluation of the call, {1, 1} where the item is not guided; rows of evaluations outside the call
 * are not written.  The sums are float64 (a product and an add each, never fused), deterministic and independent of the item's place in
 * the batch (no atomics; vv_cfg_norm_coef); every evaluation adds two small launches to the stage kernel's.  norm NULL: the call IS
 * vv_transformer_steps_guided.  guide_host NULL: every item guided everywhere.  A caller-owned ws holds vv_transformer_norm_ws_bytes bytes
 * (the same figure whatever the mask).  -22 for what vv_transformer_steps_guided refuses and for a mask that holds a 2 (guidance reuse:
 * the item has no p_u to measure); a refused call launches nothing and leaves the context usable; no readback, no synchronisation. */
typedef struct vv_cfg_norm_args {
    const float* star;       /* device [B], optional: != 0 = the optimised scale for item b */
    const float* rescale;    /* device [B], optional: phi of item b */
    float* report;           /* device [evaluations][B][2], optional */
} vv_cfg_norm_args;
VV_API int vv_transformer_steps_norm(vv_ctx* ctx, const vv_steps_args* args, const uint8_t* guide_host, int ld_guide, const vv_cfg_norm_args* norm,
                                     void* stream);
VV_API int vv_transformer_norm_ws_bytes(vv_ctx* ctx, int B, int N, const int32_t* seq_len_host, uint64_t* bytes);

/* The same decode stage with every intermediate carved from a CALLER-OWNED device block `ws` (256-byte aligned,
 * >= vv_decode_ws_bytes bytes) instead of the context arena.  The context arena may be reallocated by any later call
 * that needs more bytes (vv_ws_generation counts those moves); a launch sequence captured into a hipGraph
 * (BASELINE.json configs[4], "hipGraph-captured vocoder step") must therefore run through vv_decode_into so that
 * nothing it points at can move while the graph lives.  No reference counterpart (the reference never captures). */
VV_API int vv_decode_ws_bytes(vv_ctx* ctx, int B, int t_gen_max, uint64_t* bytes);
VV_API int vv_decode_into(vv_ctx* ctx, int B, int N, const float* x, const int32_t* ref_signal_len, const int32_t* seq_len,
                   int t_gen_max, int16_t* pcm, int ld_pcm, int32_t* pcm_len, float* wave_f32, void* ws, uint64_t ws_bytes,
                   void* stream);
VV_API uint64_t vv_ws_generation(const vv_ctx* ctx);   /* number of times the context arena has been (re)allocated */

/* Declares that the rope tables handed to vv_transformer_steps are the STANDARD RoPE tables of base `theta` (angle = pos *
 * theta^(-2i/head_dim); the q tables times head_dim^-0.5) -- which is what vv_preprocess's contract produces.  The bf16 model then
 * computes the angles in the QKV GEMM's epilogue instead of reading the tables (vv_gemm_args.rope_theta) and hands the softmax scale to
 * the attention kernel (vv_attn_args.q_scale).  theta = 0 (the default of a new context): the tables are read.  The fp32 model always
 * reads them. */
VV_API int vv_set_rope_theta(vv_ctx* ctx, float theta);

/* Context switches (explicit API, never the environment).  "fuse_mrf": run the MRF resblock pairs of the C <= 64 vocoder
 * stages through vv_mrf_resblock's fused kernel -- 0 never (two vv_conv1d launches per pair), 1 always, 2 (default) for
 * decodes of <= 8 items, where the stage is launch-bound.  Results are bit-identical either way.
 * "split_k_tail" (bf16 acoustic model): lets vv_transformer_steps take vv_gemm_tail_plan's split-K tail -- 0 (default) never,
 * 1 for the out-projection and FF2 GEMMs, 2 for FF2 only.  The K parts of a tail row are kept in fp32, summed by the consuming
 * norm and the SUM rounded to bf16 once, where a row outside the tail is rounded in the GEMM epilogue: a tail row differs from
 * the plain launch by fp32 summation order -- which later bf16 roundings amplify to bf16-level noise, so with the tail on a row's
 * result depends (inside the bf16 tolerance class) on its position in the launch.  Off, it does not; the fp32 path never splits.
 * "rope_q_attn" (bf16): 1 (default) = the query side of the rope is applied by the attention kernel while it loads Q, the QKV GEMM
 * ropes the k columns only; 0 = all of it in the GEMM epilogue (the fp32 model always does).
 * "rope_rows": 1 gathers the compact rope tables per packed row once per call (vv_rope_rows); 0 (default) looks positions up.
 * "lanes": vv_transformer_steps* runs a batch of >= 2 items as TWO half batches on two HIP streams -- lane 0 on the caller's stream,
 * lane 1 on a context-owned stream forked from it at the start of the call and joined to it before the call returns (so the call
 * keeps its stream semantics, and can be captured into a hipGraph) -- so that one lane's kernel tails and launch gaps are filled by
 * the other's kernels.  A single item runs its two CFG branches (conditional / unconditional rows) as the lanes, forked and joined once
 * per Euler step.  0 (default) = for the bf16 model from 1,024 packed rows (2 x sum of the lengths) on, 1 = never, 2 = always.
 * Results are bit-identical: every row's arithmetic is independent of what shares its launch.
 * "ring_tiles": 1 (default) = bf16 GEMMs of the path with N <= 1024 whose 64-token x 128-feature tiles are fewer than the CUs (the
 * out-projection and FF2 of a single utterance's CFG branch) take 64 x 64 tiles on a three-stage LDS ring (vv_gemm tile 6464); 0 = never;
 * n > 1 = the same with n as the tile-count bound.  Same bits either way.
 * "pp_min_tiles": -1 (default) = vv_gemm's own choice between its persistent 256 x 256 kernel and the 128 x 128 one; n >= 0 = the
 * persistent kernel for every bf16 GEMM of the path with M >= 4096, N % 256 == 0 and >= n 256-tiles.  Same bits either way. */
VV_API int vv_set_option(vv_ctx* ctx, const char* name, int value);

/* ---- profiling (HIP events on the launch stream, per kernel class) ------------------------- */
#define VV_PROF_GEMM 0
#define VV_PROF_ATTN 1
#define VV_PROF_NORM 2
#define VV_PROF_POSCONV 3
#define VV_PROF_ELEMWISE 4
#define VV_PROF_VOC_CONV 5      /* Vocos context: the backbone (embed, ConvNeXt blocks, final norm) */
#define VV_PROF_VOC_POST 6      /* Vocos context: the ISTFT head (head GEMM, spectrum, inverse-DFT GEMM, overlap-add) */
#define VV_PROF_MEL 7
#define VV_PROF_TEXT 8
/* the vocoder convs once more, by stage (each launch is counted in VV_PROF_VOC_CONV and in exactly one of these): conv_pre, the four
 * transposed-conv upsamplers (K11), the four MRF stacks (K12) */
#define VV_PROF_VOC_PRE 9
#define VV_PROF_VOC_UP0 10      /* + stage, stages 0..3 */
#define VV_PROF_VOC_MRF0 14     /* + stage, stages 0..3 */
#define VV_PROF_NCLASS 18
VV_API int vv_prof_enable(vv_ctx* ctx, int on);
/* Synchronises, then fills per class: launches, total ms, algorithmic flops, algorithmic bytes. */
VV_API int vv_prof_collect(vv_ctx* ctx, int64_t* launches, double* ms, double* flops, double* bytes);

/* ---- single-kernel entry points (unit parity tests call these through the ABI) ------------- */
typedef struct vv_gemm_args {
    int32_t dtype, out_dtype, mode, act;
    const void* A; int32_t lda;
    const void* W; int32_t ldw;
    void* C; int32_t ldc;
    int32_t M, N, K;
    const float *bias, *gate, *cos_q, *sin_q, *cos_k, *sin_k;
    int32_t n_store, seq_n, rope_dim;
    /* n_store (VV_EPI_STORE only; 0 = N): the caller relies on columns [0, n_store) being written and on NOTHING at or past n_store
       rounded up to a multiple of 4 (8 for bf16 output) ever being written; the columns in between may or may not be (the kernels
       store 4 or 8 columns at a time).  vv_gemm refuses a non-zero n_store in the other epilogue modes (-22). */
    const float *rope_cs_q, *rope_cs_k;   /* optional compact [pos][64] (cos,sin) pair tables, see vv_rope_compact */
    int32_t tile;   /* 0 = auto (bf16: the persistent 256x256 kernel when M >= 4096, N % 256 == 0 and the shape has at least one round of
                       256-tiles for the chip's CUs or N >= 3072, below that 128x128 tiles or, for launches that do not fill the chip, 64-token x 128-feature
                       tiles; fp32: 256x256 when M >= 4096 and N % 256 == 0), 128 or 256 to force (bf16: also 64, and 6464 = 64 x 64 tiles on a three-stage
                       LDS ring).  Every bf16 choice gives the same bits */
    const int32_t* rope_pos;   /* optional [M]: rope position of each row (packed ragged rows); default row % seq_n */
    int32_t rope_by_row;       /* 1: rope_cs_q / rope_cs_k are [M][64] tables gathered per row by vv_rope_rows (the persistent kernel then
                                  needs no position lookup); the cos/sin tables + rope_pos still serve the other kernels */
    int32_t tail_parts, tail_row0;   /* split-K tail (VV_EPI_GATE_STORE, bf16): both exactly as vv_gemm_tail_plan returns them, 0 = off */
    void* C_tail;              /* tail_parts > 1: fp32 [tail_parts][M - tail_row0][ldc] gated products of the K parts of rows >= tail_row0
                                  (part 0 carries the bias); those rows of C are NOT written: the consumer sums the parts and rounds
                                  the sum to the output dtype once (vv_ln_args.delta_tail) */
    float rope_theta;          /* VV_EPI_QKV_ROPE, bf16: > 0 = the tables are the standard RoPE tables of this base (angle = pos * theta^(-2i/64)):
                                  the epilogue COMPUTES cos / sin of the q and k columns (v_exp / v_fract / v_sin / v_cos on the position: no
                                  table load behind the stores, the costliest part of the rope epilogue) and applies NO softmax scale to q
                                  (vv_attn_args.q_scale carries it); angle accurate to ~3e-4 rad at position 4096 -- a tenth of a bf16
                                  rounding of the roped value.  0 = read the tables (always in fp32) */
    int32_t rope_skip_q;       /* VV_EPI_QKV_ROPE: 1 = leave the q columns [0, rope_dim) un-roped (plain bias + store); the attention
                                  kernel ropes them while it loads Q (vv_attn_args.rope_cs_q).  The k columns are roped as always */
    int32_t chip_share;        /* 0 / 1 = the launch has the chip to itself; 2 = it shares the chip with another stream of launches (the
                                  two lanes of vv_transformer_steps): tile = 0 then prices its tilings for half of the CUs.  Speed only */
} vv_gemm_args;
VV_API int vv_gemm(vv_ctx* ctx, const vv_gemm_args* args, void* stream);
/* The persistent bf16 GEMM walks ceil(tiles / CUs) rounds of 256x256 tiles; when the tile count leaves a partial last round, the
 * gate-store form can split the K range of the last row panels `parts` ways so that the remainder costs 1/parts of a round.
 * Returns the plan for this shape (contiguous operands: lda = ldw = K, ldc = N) on the context's device: rows >= row0 are split
 * `parts` ways; parts = 0: nothing to gain, or an operand of 2 GiB or more (those take the plain-pointer kernel, which has no
 * tail).  ctx may be NULL (the process's current device, 256 CUs when there is none). */
VV_API int vv_gemm_tail_plan(vv_ctx* ctx, int32_t M, int32_t N, int32_t K, int32_t* row0, int32_t* parts);

typedef struct vv_attn_args {
    int32_t dtype;
    const void* qkv; int32_t ld_qkv;
    void* out; int32_t ld_out; /* qkv, out and ld_qkv rows 16-byte aligned; ld_out a multiple of 4 elements (the width of a store) */
    int32_t n_seq, seq_n, heads, dim;
    const int32_t* kv_len;     /* optional [n_seq]: keys [0, kv_len[s]) of sequence s are attended, clamped to seq_n.  Padded layout: a
                                  length <= 0 is taken as 1 (the sequence still has its seq_n output rows).  Packed layout: a sequence
                                  with kv_len[s] <= 0 owns no row -- nothing of it is read or written */
    const int32_t* row_start;  /* optional [n_seq]: packed ragged rows -- sequence s owns rows [row_start[s], +kv_len[s]);
                                  default s * seq_n (padded layout, rows beyond kv_len are computed and ignored).
                                  EVERY row inside the qkv buffer must hold FINITE values, masked ones included (rows >= kv_len[s] of a
                                  padded sequence, a packed neighbour's rows, rows no sequence owns): a masked key gets the weight 0, and a
                                  non-finite V there reaches the output as 0 x nan */
    int32_t total_rows;        /* rows in the qkv / out buffers (bounds the K/V buffer resource; reads past it return zero).
                                  Required (> 0) with row_start; 0 = n_seq * seq_n in the padded layout */
    float q_scale;             /* bf16 kernel: factor applied to q while it is loaded (the softmax scale when the projection did not carry
                                  it: vv_gemm_args.rope_theta); 0 = 1.0 */
    const float* rope_cs_q;    /* optional (bf16 kernel): compact [seq_n][64] (cos, sin) pair table of the QUERY side (vv_rope_compact of
                                  the q tables, which carry the softmax scale): the q columns arrive un-roped (vv_gemm_args.rope_skip_q)
                                  and are roped here, position = row inside the sequence, in fp32 before the one rounding to bf16 the
                                  kernel applies to Q anyway.  NULL = q is already roped */
} vv_attn_args;
VV_API int vv_attention(vv_ctx* ctx, const vv_attn_args* args, void* stream);

typedef struct vv_ln_args {
    int32_t out_dtype;
    const float* x; int32_t ldx;
    void* y; int32_t ldy;
    int32_t R, D;
    const float *w, *b;
    int32_t add_one;
    float eps;
    const void* delta;      /* optional [R][ld_delta]: x += delta first (x is then updated in place) */
    int32_t delta_dtype, ld_delta;
    const void* delta2;     /* optional second delta (same dtype / ld): y = LN((x + delta) + delta2) */
    int32_t keep_x;         /* 1: normalise x + delta but leave x as it is (the caller adds this delta again later, with delta2) */
    int32_t tail_row0;      /* split-K tails of the deltas (vv_gemm_args.C_tail): for rows >= tail_row0 the delta is NOT read;    */
    int32_t delta_tail_parts, delta2_tail_parts;   /*   it is the sum, in part order, of fp32 delta_tail [parts][R - tail_row0][ld_delta] */
    const void *delta_tail, *delta2_tail;          /*   rounded once to delta_dtype (0 / 1 parts = none)                       */
} vv_ln_args;
/* Refused with -22 (nothing is launched, nothing written): R < 1; D outside [4, 1024] or not a multiple of 4; ldx, ldy not multiples of 4
 * or below D; ld_delta likewise when delta is given; delta2 without delta; a tail (parts > 1) without its delta or its buffer, with
 * tail_row0 outside [0, R), more than 8 parts or a buffer that is not 16-byte aligned.  w / b NULL = 1 - add_one / 0. */
VV_API int vv_layernorm(vv_ctx* ctx, const vv_ln_args* args, void* stream);

typedef struct vv_posconv_args {
    int32_t dtype, out_dtype;
    const void* in; int32_t ld_in;
    const void* W;            /* bf16: [G][KW][64 co][64 ci]   f32: [G][KW][64 ci][64 co] */
    const float* bias;
    void* out; int32_t ld_out;
    const void* resid; int32_t ld_resid;   /* optional, operand dtype; ld_resid >= groups * 64 */
    int32_t n_seq, seq_n, groups, KW, B;
    const int32_t* seq_len;    /* optional [B], indexed seq % B (conditional and unconditional lanes share it): B >= 1 when given */
    const int32_t* row_start;  /* optional [n_seq]: packed ragged rows, as in vv_attn_args */
} vv_posconv_args;
/* Refused with -22 (nothing is launched): seq_len with B <= 0; resid with ld_resid < groups * 64; and, on the bf16 kernel, whose epilogue
 * moves 4 channels at a time: ld_out or ld_resid not a multiple of 4 elements, out not 8-byte (bf16 out) / 16-byte (f32 out) aligned,
 * resid not 8-byte aligned, bias not 16-byte aligned.  The f32 kernel's epilogue is scalar and has no such precondition. */
VV_API int vv_posconv(vv_ctx* ctx, const vv_posconv_args* args, void* stream);

typedef struct vv_conv_args {
    const float* in;          /* [B][Cin][T_in]  */
    const float* W;           /* [Cin_pad8][KW][rows_pad64], rows = co (conv) or co*up + phase (transposed); nothing past Cin_pad8 is read */
    const float* bias;        /* [Cout] */
    float* out;               /* [B][Cout][T_out] */
    const float* resid;       /* optional, like out */
    int32_t B, Cin, Cout, T_in, T_out, KW, dil, transposed, up, rows_total, rows_pad, accumulate;
    float pre_slope, out_scale;
    const int32_t* len_in;    /* optional per-item valid input length */
    const void* W_x3;         /* optional: W split by vv_conv_split_weights; when given, the products run as exact 3-way bf16
                                 splits on the bf16 matrix pipe (six piece products, fp32 accumulate: fp32 fidelity, ~2.7x less
                                 matrix time) instead of v_mfma_f32_32x32x2_f32.  Same result class, not bit-identical. */
    int32_t wg_rows;          /* x3 only: 0 = default (64-row workgroups of 4 waves; the x2 up-samplers with 64 / 128 input channels take the
                                 streaming kernel), 128 = 128-row workgroups of 8 waves when rows_total > 64, -1 = the generic kernel
                                 also where the streaming one would be taken (its bit-identical twin: tests, A/B) */
} vv_conv_args;
VV_API int vv_conv1d(vv_ctx* ctx, const vv_conv_args* args, void* stream);
/* W fp32 [Cin_pad][KW][rows_pad] -> out [ceil(Cin_pad / 16)][KW][3 pieces][2 octets][rows_pad][8] bf16 (w = h + m + l exactly, each piece the
 * truncated leading 8 significand bits of the remainder).  vv_conv_split_bytes gives the size of `out` (16-byte aligned). */
VV_API uint64_t vv_conv_split_bytes(int32_t Cin_pad, int32_t KW, int32_t rows_pad);
VV_API int vv_conv_split_weights(vv_ctx* ctx, const float* W, int32_t Cin_pad, int32_t KW, int32_t rows_pad, void* out, void* stream);

/* K12, one (kernel, dilation) pair of an MRF resblock fused through LDS (SURVEY 8(a) K12 / 8(b) vv_mrf_resblock):
 *   out = [accumulate ? out : 0] + out_scale * ( conv2(lrelu(conv1(lrelu(y)))) + y ),  conv1 dilated, conv2 undilated, C -> C.
 * Fused form for C = 32 / 64 (the intermediate tile stays in the CU); bit-identical to vv_conv1d(conv1) + vv_conv1d(conv2, resid = y).
 * replaces two nodes of decode.onnx's HiFi-GAN resblock (reference core/tts_engine.py:176-187 runs the graph; no source). */
typedef struct vv_mrf_args {
    const float* y;           /* [B][C][T] resblock input (also the residual) */
    const float *W1, *b1;     /* conv1: [C_pad8][KW][64], [C] */
    const float *W2, *b2;     /* conv2 */
    float* out;               /* [B][C][T], must not alias y */
    int32_t B, C, T, KW, dil, rows_pad, accumulate;
    float slope, out_scale;
    const int32_t* len_in;    /* optional per-item valid length */
} vv_mrf_args;
VV_API int vv_mrf_resblock(vv_ctx* ctx, const vv_mrf_args* args, void* stream);

/* N6 single-kernel entries (unit parity).  vv_vocos_im2col: the embed conv's operand, out [B * T_max][ld_out] f32 (16-byte aligned,
 * ld_out >= embed_k * n_mel, % 4): out[b * T_max + t][j * n_mel + m] = x[b][ref_len[b] + t + j - embed_k / 2][m] inside the item's
 * generated frames [0, min(min(seq_len[b], N) - ref_len[b], T_max)), 0 elsewhere and in the columns past embed_k * n_mel; ref_len[b] is
 * clamped to [0, max(min(seq_len[b], N), 0)] first, so no device length addresses a row outside the item.
 * vv_istft_head (finalized Vocos context): head [B][T_max][ld_head] f32 (the head GEMM's output, ld_head >= n_fft + 2), n_frames[B]
 * valid frames per item (device) -> pcm [B][ld_pcm] int16, pcm_len[B] = hop * max(T_b - 1, 0), optional wave_f32 [B][T_max * hop];
 * ld_pcm >= T_max * hop.  Reads only each item's valid frames; uses the context arena. */
VV_API int vv_vocos_im2col(vv_ctx* ctx, const float* x, int B, int N, const int32_t* ref_signal_len, const int32_t* seq_len, int T_max,
                           float* out, int ld_out, void* stream);
VV_API int vv_istft_head(vv_ctx* ctx, int B, int T_max, const float* head, int ld_head, const int32_t* n_frames, int16_t* pcm, int ld_pcm,
                         int32_t* pcm_len, float* wave_f32, void* stream);
/* Text-stack single-kernel entries (unit parity): thin wrappers over the kernels vv_preprocess chains (and, for vv_dwconv, the Vocos
 * backbone).  A violated precondition is refused with -22 before anything is launched.  Sequence s of n_seq reads seq_len[s % B].
 * vv_text_embed: out [2 B][N][Dt] f32 = emb[id] + pos[t]; sequences [0, B) take id = ids[b][t] + 1 for t < min(text_len[b], ld_ids)
 *   and the filler id 0 behind it, sequences [B, 2 B) (the drop half) the filler everywhere; id is clamped to [0, vocab_rows - 1].
 *   emb [vocab_rows][Dt], pos [>= N][Dt], out: 16-byte aligned; Dt % 4 == 0; B, N, ld_ids, vocab_rows >= 1.
 * vv_dwconv: depthwise conv along tokens, in / out [n_seq][N][C] f32 (distinct buffers), w [C][KW], bias [C]; tokens outside
 *   [0, min(seq_len, N)) read as zero (seq_len NULL = N; a length <= 0 leaves the bias), every one of the N output rows is written.
 *   in, out, bias 16-byte aligned; C % 4 == 0; KW odd; B >= 1 when seq_len is given.
 * vv_grn: x [n_seq][N][C] of dtype (VV_DTYPE_F32 / VV_DTYPE_BF16), in place: x = x * (gamma * nx + 1) + beta on all N rows, nx = g / (mean_c g + 1e-6),
 *   g[c] = sqrt(sumsq[s][c]), sumsq [n_seq][C] f32 (caller's scratch, written) = the sum of x^2 over the tokens [0, min(seq_len, N)).
 *   x aligned to 4 elements, beta to 16 bytes; C % 64 == 0, C <= 8192; B >= 1 when seq_len is given. */
VV_API int vv_text_embed(vv_ctx* ctx, const int32_t* ids, int ld_ids, const int32_t* text_len, const float* emb, const float* pos,
                         int vocab_rows, float* out, int B, int N, int Dt, void* stream);
VV_API int vv_dwconv(vv_ctx* ctx, const float* in, float* out, const float* w, const float* bias, const int32_t* seq_len, int B, int n_seq,
                     int N, int C, int KW, void* stream);
VV_API int vv_grn(vv_ctx* ctx, int dtype, void* x, float* sumsq, const float* gamma, const float* beta, const int32_t* seq_len, int B,
                  int n_seq, int N, int C, void* stream);
/* K13: pcm [B][ld_pcm] int16 = trunc(clamp(32767 * tanh(conv_k7(lrelu(in)) + bias))), in [B][C][T] f32 read as zero from len_in[b]
 * (optional, clamped to [0, T]) on, w [C][7]; optional wave_f32 [B][T].  Refused with -22 (nothing launched): KW != 7, C outside
 * [1, 64], pre_slope outside (0, 1], B < 1, T < 1, ld_pcm < T, in / w / pcm NULL, a row of 2 GiB or more. */
VV_API int vv_conv_post(vv_ctx* ctx, const float* in, const float* w, float bias, int16_t* pcm, int ld_pcm, float* wave_f32,
                 int B, int C, int T, int KW, float pre_slope, const int32_t* len_in, void* stream);
/* K1: mel [B][F_max][n_mel] f32 = log-mel of audio [B][ld_audio] int16; item b has audio_len[b] / hop + 1 frames, the frames behind them are
 * zeros.  audio_len is a DEVICE array: a value outside [0, ld_audio] is clamped to the row (wrong audio for that call, never a read outside
 * the row).  Refused with -22 (nothing launched): audio / audio_len / mel NULL, ld_audio < 1, B < 1 or above 65535, F_max < 1. */
VV_API int vv_mel(vv_ctx* ctx, const int16_t* audio, int ld_audio, const int32_t* audio_len, float* mel, int B, int F_max,
           void* stream);
/* K5 GroupNorm over channel-major [B][C][T] fp32 (G groups), optional per-channel affine and fused activation code */
VV_API int vv_groupnorm(vv_ctx* ctx, const float* x, float* y, const float* gamma, const float* beta, int B, int C, int T, int G,
                 float eps, int act, void* stream);
/* out[pos][2i] = cos[pos][2i], out[pos][2i+1] = sin[pos][2i]  (tables with duplicated pairs, n rows x 64) */
VV_API int vv_rope_compact(vv_ctx* ctx, const float* cos_t, const float* sin_t, float* out, int n, void* stream);
/* out[r][0..63] = compact[pos[r]][0..63]: the compact table gathered once per call for every packed row */
VV_API int vv_rope_rows(vv_ctx* ctx, const float* compact, const int32_t* pos, float* out, int rows, void* stream);
/* N7: one stage i of an explicit Runge-Kutta step.  k_i = p_c + (p_c - p_u) * g from pred (conditional rows [0, Rc), unconditional
 * [Rc, 2 Rc), ld ldp), g = g_item[row / seq_n] when g_item is given (row = row_src[r] or r), else the scalar; k_i is stored to k_out
 * when that is not NULL.  acc = x[row] + sum_{j < n_prev, coef[j] != 0} coef[j] * k_prev[j][r] + coef[n_prev] * k_i (ascending j, a zero
 * coefficient is skipped and its buffer may be NULL).  x_out != NULL: x_out[r] = acc (packed rows [Rc][n_mel], the next stage's
 * state); x_out == NULL: x[row] = acc in place (the step's last stage).  The coefficients are h * a[i+1][j] (h * b[j] on the last
 * stage).  All buffers fp32, 16-byte aligned. */
typedef struct vv_ode_stage_args {
    float* x; const float* pred; int32_t ldp, Rc, n_mel, n_prev;
    const float* k_prev[3]; float coef[4];
    float* k_out; float* x_out;
    float g; const float* g_item; int32_t seq_n; const int32_t* row_src;
} vv_ode_stage_args;
VV_API int vv_ode_stage(vv_ctx* ctx, const vv_ode_stage_args* args, void* stream);
/* N8: the same stage where only some rows have an unconditional prediction.  u_row [Rc] int32 (device): u_row[r] >= 0 = the ROW OF pred
 * that holds p_u of packed row r (the guided rows compacted behind the conditional ones: values in [Rc, Rc + Ru)); u_row[r] < 0 = row r
 * is not guided, k_i = p_c.  u_row[r] = Rc + r for every r is vv_ode_stage bit for bit, and so is u_row NULL.  The caller keeps the
 * entries inside pred. */
VV_API int vv_ode_stage_guided(vv_ctx* ctx, const vv_ode_stage_args* args, const int32_t* u_row, void* stream);
/* N11 single-kernel entries (unit parity).  vv_apg_coef: the reduction and the coefficients of one evaluation.  Item b owns the packed
 * conditional rows [row_start[b], + len[b]) of pred (device [B] int32, inside [0, Rc), len[b] <= VV_APG_TILE * n_tiles); p_u of row r is
 * pred row Rc + r, or u_row[r] when u_row is given (< 0: not guided); x_e of row r is row row_src[r] of x_e, or r when row_src is NULL.
 * partials [B][n_tiles][3] float64 (scratch: the entries of an item's tiles are written, the rest untouched), coef [B][2] fp32 = {A, C};
 * {0, 0} for an item without rows or not guided.  g_item / eta / norm_rms: device [B], optional (g, 1, no cap). */
typedef struct vv_apg_coef_args {
    const float* pred; int32_t ldp, Rc, n_mel;
    const int32_t* u_row;
    const float* x_e; const int32_t* row_src;
    int32_t B, n_tiles;
    const int32_t* row_start; const int32_t* len;
    float t_e, g;
    const float* g_item; const float* eta; const float* norm_rms;
    double* partials; float* coef;
} vv_apg_coef_args;
VV_API int vv_apg_coef(vv_ctx* ctx, const vv_apg_coef_args* args, void* stream);
/* vv_ode_stage_guided with the projected combine: the strength of row r's item (row_src[r] / seq_n, or r / seq_n) is coef[item][0], and
 * where coef[item][1] != 0 the slope also takes coef[item][1] * fmaf(1 - t_e, p_c, x_e) (x_e row r when x_e_packed, else row_src[r]; x_e
 * must not be an output of the launch).  g and g_item are not read.  apg NULL: the call IS vv_ode_stage_guided. */
typedef struct vv_apg_stage_args { const float* coef; const float* x_e; int32_t x_e_packed; float t_e; } vv_apg_stage_args;
VV_API int vv_ode_stage_apg(vv_ctx* ctx, const vv_ode_stage_args* args, const int32_t* u_row, const vv_apg_stage_args* apg, void* stream);
/* N20 single-kernel entry (unit parity): the sums of the step report.  Item b owns the packed rows [row_start[b], + len[b]) of f and
 * f_prev ([Rc][n_mel] fp32, 16-byte aligned; row_start, len: device [B] int32, clamped into [0, Rc) and to VV_APG_TILE * n_tiles rows).
 * partials [B][n_tiles][2] float64 (scratch: the entries of an item's tiles are written, the rest untouched), report [B][2] float64 =
 * {sum (f - f_prev)^2, sum f^2}: differences, squares and sums in float64, a product and an add each (never fused), tiles of VV_APG_TILE
 * frames from the item's frame 0, float4 q of a tile on thread q % 256, one fixed tree, the tiles added in ascending order -- an item's
 * sums depend on its own rows alone.  f_prev NULL: D2 = 0.  {0, 0} for an item without rows. */
typedef struct vv_ode_diff_args {
    const float* f; const float* f_prev; int32_t Rc, n_mel;
    int32_t B, n_tiles;
    const int32_t* row_start; const int32_t* len;
    double* partials; double* report;
} vv_ode_diff_args;
VV_API int vv_ode_diff_reduce(vv_ctx* ctx, const vv_ode_diff_args* args, void* stream);
/* N21 single-kernel entries (unit parity).  vv_ode_stage_reuse: vv_ode_stage_guided where the guidance difference D = p_c - p_u (one fp32
 * subtraction) of an ITEM can be kept in d_buf ([Rc][n_mel] fp32, packed rows, 16-byte aligned, a buffer of its own).  The mode of packed
 * row r is that of its item row_src[r] / seq_n (or r / seq_n), item_mode_host[item] on the HOST (n_items of them, at most 1024; they travel
 * as kernel arguments): VV_REUSE_LOAD -- where u_row[r] < 0 the row reads D from d_buf and k = p_c + D g (no row of pred holds its p_u);
 * VV_REUSE_STORE -- where u_row[r] >= 0 the row's D is also written to d_buf.  A row with u_row[r] >= 0 is computed whatever LOAD says, a
 * row with u_row[r] < 0 without LOAD is not guided (k = p_c).  Every mode 0: vv_ode_stage_guided bit for bit, and a computed row always is.
 * reuse NULL: the call IS vv_ode_stage_guided.
 * vv_cfg_drift_reduce: the sums of the drift report.  Item b owns the packed rows [row_start[b], + len[b]) (as vv_ode_diff_reduce).  Over
 * its rows with u_row[r] >= 0: D_new = p_c - p_u (fp32, from pred rows r and u_row[r]); report [B][2] float64 = {sum (D_new - d_buf[r])^2,
 * sum D_new^2}, the first sum 0 for an item whose has_old_host[b] (HOST [B], NULL = none) is 0 -- d_buf is not read for it.  Differences of
 * the two, squares and sums in float64, a product and an add each (never fused), vv_ode_diff_reduce's tiles and order.  partials
 * [B][n_tiles][2] float64 scratch. */
#define VV_REUSE_LOAD 1
#define VV_REUSE_STORE 2
typedef struct vv_reuse_stage_args { float* d_buf; const uint8_t* item_mode_host; int32_t n_items; } vv_reuse_stage_args;
VV_API int vv_ode_stage_reuse(vv_ctx* ctx, const vv_ode_stage_args* args, const int32_t* u_row, const vv_reuse_stage_args* reuse, void* stream);
typedef struct vv_cfg_drift_args {
    const float* pred; int32_t ldp, Rc, n_mel;
    const int32_t* u_row;
    const float* d_buf; const uint8_t* has_old_host;
    int32_t B, n_tiles;
    const int32_t* row_start; const int32_t* len;
    double* partials; double* report;
} vv_cfg_drift_args;
VV_API int vv_cfg_drift_reduce(vv_ctx* ctx, const vv_cfg_drift_args* args, void* stream);
/* N24 single-kernel entries (unit parity).  vv_cfg_norm_coef: the Gram sums and the coefficients of one evaluation.  Item b owns the packed
 * conditional rows [row_start[b], + len[b]) of pred (as vv_apg_coef); p_u of row r is pred row Rc + r, or u_row[r] when u_row is given
 * (< 0: not guided); columns >= n_mel of a row are never read.  partials [B][n_tiles][5] float64 = {S_cu, S_uu, S_cc, S_c, S_u} per tile
 * (scratch: the entries of an item's tiles are written, the rest untouched), coef [B][2] fp32 = {s, f}; {1, 1} for an item without rows
 * or not guided.  g_item / star / rescale: device [B], optional (g, off, off).  report: optional second copy of coef.
 * vv_ode_stage_norm: vv_ode_stage_guided where row r's slope is coef[item][1] * (p_c + (p_c - coef[item][0] * p_u) * g), item =
 * row_src[r] / seq_n (or r / seq_n); u_row is required.  coef = {1, 1} everywhere is vv_ode_stage_guided bit for bit.  coef NULL: the
 * call IS vv_ode_stage_guided. */
typedef struct vv_cfg_norm_coef_args {
    const float* pred; int32_t ldp, Rc, n_mel;
    const int32_t* u_row;
    int32_t B, n_tiles;
    const int32_t* row_start; const int32_t* len;
    float g;
    const float* g_item; const float* star; const float* rescale;
    double* partials; float* coef; float* report;
} vv_cfg_norm_coef_args;
VV_API int vv_cfg_norm_coef(vv_ctx* ctx, const vv_cfg_norm_coef_args* args, void* stream);
VV_API int vv_ode_stage_norm(vv_ctx* ctx, const vv_ode_stage_args* args, const int32_t* u_row, const float* coef, void* stream);
/* N23 single-kernel entries (unit parity).  vv_block_span: one launch of the span kernel on contiguous [R][D] planes.  X = (x + (float)d1)
 * + (float)d2 per element (fp32 adds in this order; d1 / d2 of delta_dtype, d2 NULL = one delta, d1 NULL = X is x); VV_SPAN_MARK: buf = X;
 * VV_SPAN_DIFF: buf = X - buf; VV_SPAN_APPLY: x = X + buf.  Nothing else is written.  -22 for R < 1, D < 4 or not a multiple of 4, a null
 * x or buf, d2 without d1, x / buf not 16-byte or a delta not 16-byte (f32) / 8-byte (bf16) aligned, or buf aliasing x.
 * vv_block_drift_reduce: the sums of the block-cache report.  Sequence s of n_seq owns the rows [row_start[s], + len[s]) of d_new and
 * d_prev ([R][D] fp32, 16-byte aligned; row_start, len: device [n_seq] int32, clamped into [0, R) and to VV_APG_TILE * n_tiles rows); it is
 * branch branch0 + s / n_items of item s % n_items (n_seq = n_items, or 2 n_items with branch0 0).  report [n_items][2][2] float64 =
 * {sum (d_new - d_prev)^2, sum d_new^2} at [item][branch]: vv_ode_diff_reduce's arithmetic, tiles and order.  d_prev NULL: the first sum is
 * 0.  partials [n_seq][n_tiles][2] float64 scratch. */
#define VV_SPAN_MARK 0
#define VV_SPAN_DIFF 1
#define VV_SPAN_APPLY 2
typedef struct vv_block_span_args {
    int32_t mode, delta_dtype;
    float* x; const void* d1; const void* d2; float* buf;
    int32_t R, D;
} vv_block_span_args;
VV_API int vv_block_span(vv_ctx* ctx, const vv_block_span_args* args, void* stream);
typedef struct vv_block_drift_args {
    const float* d_new; const float* d_prev; int32_t R, D;
    int32_t n_seq, n_items, branch0, n_tiles;
    const int32_t* row_start; const int32_t* len;
    double* partials; double* report;
} vv_block_drift_args;
VV_API int vv_block_drift_reduce(vv_ctx* ctx, const vv_block_drift_args* args, void* stream);
/* K9: x[r] += dt * (p_c + (p_c - p_u) * cfg) over n_mel columns, p_c = pred row r, p_u = pred row BN + r (ld ldp, fp32).  Refused with
 * -22 (nothing launched): n_mel or ldp not a multiple of 4, BN < 1, n_mel < 4, ldp < n_mel, x or pred NULL or not 16-byte aligned.
 * vv_cfg_euler_rows: the same update on packed rows -- x row row_src[r] (device [BN] int32, the caller keeps it inside x) takes pred rows r
 * and BN + r; row_src NULL is vv_cfg_euler. */
VV_API int vv_cfg_euler(vv_ctx* ctx, float* x, const float* pred, int ldp, int BN, int n_mel, float cfg, float dt, void* stream);
VV_API int vv_cfg_euler_rows(vv_ctx* ctx, float* x, const float* pred, int ldp, int BN, int n_mel, float cfg, float dt, const int32_t* row_src,
                             void* stream);
/* Single-kernel entries (unit parity) of the kernels between the transformer's prediction and the PCM.  Each is the launcher a stage
 * calls; a violated precondition is refused with -22 before anything is launched, and every array must be 4-byte aligned.
 * vv_pack_cat (K2): out [2 BN][ldo] of dtype (VV_DTYPE_F32 / VV_DTYPE_BF16, round to nearest even) = [x | cat | 0] for rows [0, BN) and
 *   [x | cat_drop | 0] for rows [BN, 2 BN): row r of either half reads row row_src[r] (or r when NULL) of x [..][n_mel], cat and cat_drop
 *   [..][cond_dim]; columns [n_mel + cond_dim, ldo) are zeros.  only_x: only the n_mel state columns are written.  n_mel >= 4, n_mel,
 *   cond_dim, ldo multiples of 4, ldo >= n_mel + cond_dim, BN >= 1; x, cat, cat_drop 16-byte aligned, out 16-byte (f32) / 8-byte (bf16).
 * vv_pack_cat_guided (N8): rows [row0, row0 + n_rows) of the same buffer for a guided subset: row r < Rc reads cat row row_src[r], row
 *   Rc + u reads cat_drop row u_src[u]; the state columns come from x row row_src[r] / u_src[u], or with x_packed (x = the packed stage
 *   state [Rc][n_mel]) from x row r / u_crow[u].  Rc >= 1, row0 >= 0, n_rows >= 1, the three tables required; otherwise as vv_pack_cat.
 * vv_row_tables: the packed-row tables from device lengths clamped to [0, N] and to the Rc rows (host count) that exist:
 *   row_start[2 B] (row_start[B + b] = Rc + row_start[b]), kv_len[2 B], row_src[Rc] = b * N + t, row_pos[2 Rc] = t.  Rows no item owns
 *   (device lengths summing to fewer than Rc) map to the last item's padding rows min(len + i, N - 1).  B, N, Rc >= 1.
 * vv_guided_tables: the same with the unconditional half compacted to the items with guided[b] != 0 (HOST [B] bytes), Ru rows:
 *   row_start[B + j] = Rc + u0, rs_rel[j] = u0, kv_len[B + j] for the j-th guided item, row_pos[Rc + Ru], u_src[Ru], u_crow[Ru],
 *   u_row[Rc] (Rc + u, or -1 for a row without an unconditional one).  1 <= B <= 1024, N, Rc >= 1, 0 <= Ru <= Rc.
 * vv_ref_len: ref_len[b] = audio_len[b] / hop + 1.  B, hop >= 1.
 * vv_decode_len: lens[l][b] = tg_b * mult[l] (l < n_levels, mult device [n_levels]), tg_b = min(sl - min(max(ref_len[b], 0), sl), T_max),
 *   sl = max(min(seq_len[b], N), 0): the frames vv_mel_slice hands on.  vv_vocos_lens: lens[b] = the same tg_b.
 * vv_mel_slice (K10): out [B][n_mel][T] f32, out[b][c][t] = x[b][rl + t][c] for t < tg_b (rl = min(max(ref_len[b], 0), sl)), 0 behind;
 *   x [B][N][n_mel].  B, N, n_mel, T >= 1.
 * vv_vocos_im2col_ex: vv_vocos_im2col with n_mel and the (odd) tap count k as arguments; needs no Vocos context.
 * vv_vocos_spectrum: head [R][ld_head] f32 = (log-magnitudes 0..n_fft/2 | phases 0..n_fft/2) -> out [R][n_fft]: column k <= n_fft/2 =
 *   m_k cos p_k, column n_fft/2 + k (1 <= k < n_fft/2) = m_k sin p_k, m_k = min(exp(o_k), 100).  R >= 1, n_fft even >= 4,
 *   ld_head >= n_fft + 2.
 * vv_vocos_ola: frames [B][T_max][ld_f] f32 (windowed, ld_f >= n_fft), lens[B] valid frames (clamped to [0, T_max]), window [n_fft] ->
 *   sample j of item b = the overlap-add at position j + n_fft/2 over the sum of the window squares there, for j < pcm_len[b] =
 *   hop * max(T_b - 1, 0), zeros behind up to T_max * hop; pcm int16 = trunc(clamp(y * 32767)), optional wave f32 and pcm_len.
 *   n_fft even, n_fft % hop == 0, ld_pcm (and ld_wave with wave) >= T_max * hop < 2^31.  Needs no Vocos context. */
VV_API int vv_pack_cat(vv_ctx* ctx, int dtype, const float* x, const float* cat, const float* cat_drop, void* out, int ldo, int BN, int n_mel,
                       int cond_dim, int only_x, const int32_t* row_src, void* stream);
VV_API int vv_pack_cat_guided(vv_ctx* ctx, int dtype, const float* x, const float* cat, const float* cat_drop, void* out, int ldo, int Rc,
                              int row0, int n_rows, int n_mel, int cond_dim, int only_x, int x_packed, const int32_t* row_src,
                              const int32_t* u_src, const int32_t* u_crow, void* stream);
VV_API int vv_row_tables(vv_ctx* ctx, const int32_t* seq_len, int B, int N, int Rc, int32_t* row_start, int32_t* row_src, int32_t* row_pos,
                         int32_t* kv_len, void* stream);
VV_API int vv_guided_tables(vv_ctx* ctx, const int32_t* seq_len, const uint8_t* guided, int B, int N, int Rc, int Ru, int32_t* row_start,
                            int32_t* rs_rel, int32_t* kv_len, int32_t* row_pos, int32_t* u_src, int32_t* u_crow, int32_t* u_row, void* stream);
VV_API int vv_ref_len(vv_ctx* ctx, const int32_t* audio_len, int32_t* ref_len, int B, int hop, void* stream);
VV_API int vv_decode_len(vv_ctx* ctx, const int32_t* seq_len, const int32_t* ref_len, int32_t* lens, int B, int n_levels, const int32_t* mult,
                         int N, int T_max, void* stream);
VV_API int vv_vocos_lens(vv_ctx* ctx, const int32_t* seq_len, const int32_t* ref_len, int32_t* lens, int B, int N, int T_max, void* stream);
VV_API int vv_mel_slice(vv_ctx* ctx, const float* x, int B, int N, int n_mel, const int32_t* ref_len, const int32_t* seq_len, float* out, int T,
                        void* stream);
VV_API int vv_vocos_im2col_ex(vv_ctx* ctx, const float* x, int B, int N, int n_mel, const int32_t* ref_signal_len, const int32_t* seq_len,
                              int T_max, int k, float* out, int ld_out, void* stream);
VV_API int vv_vocos_spectrum(vv_ctx* ctx, const float* head, int ld_head, int R, int n_fft, float* out, void* stream);
VV_API int vv_vocos_ola(vv_ctx* ctx, const float* frames, int ld_f, int B, int T_max, const int32_t* lens, const float* window, int n_fft, int hop,
                        int16_t* pcm, int ld_pcm, int32_t* pcm_len, float* wave, int ld_wave, void* stream);

/* ---- reference-clip ingest on the device (a8 + SURVEY 8(f) N3).  Together they replace the arithmetic of
 * AudioProcessor.load_audio after RIFF parsing (reference core/audio_processor.py:15-44): pydub's set_channels(1) =
 * audioop.tomono(.., 0.5, 0.5), set_frame_rate = audioop.ratecv(.., None), float32 conversion, then normalize_to_int16 =
 * remove DC (numpy's float32 mean, in numpy's summation order), peak -> 29491, truncate.  Bit-exact to stdlib audioop + numpy. */
/* pcm = the clips' interleaved little-endian signed PCM bytes, back to back (each clip 4-byte aligned); desc = n_clips x 8 int64
 * (device): {byte offset, sample width 1|2|4, channels, n_frames, src_rate / g, dst_rate / g, out offset (floats), n_out} with
 * g = gcd(src_rate, dst_rate) and n_out = (n_frames - 1) * (dst_rate / g) / (src_rate / g) + 1 (= n_frames at equal rates).
 * out[out offset + m] = float32 of the mono sample m at the destination rate.  max_out = the largest n_out.  The rows live in device
 * memory, so the library cannot check them: the CALLER validates them against the two buffers before the call (runtime.HipSynth.ingest_pcm does). */
VV_API int vv_ingest_pcm(vv_ctx* ctx, const void* pcm, const int64_t* desc, int n_clips, int64_t max_out, float* out, void* stream);
/* opt-in, NOT the reference's arithmetic: polyphase FIR resampler y[n] = sum_i x[i] * taps[(n + skip) * down - i * up],
 * f64 accumulate, f32 out.  taps = host-designed low-pass already scaled by `up` (f64, device). */
VV_API int vv_resample_poly(vv_ctx* ctx, const float* x, int n_in, const double* taps, int n_taps, int up, int down, int skip,
                     float* y, int n_out, void* stream);
/* n_clips mono f32 clips stored back to back, clip i = [offsets[i], offsets[i+1]); out has the same offsets.
 * scratch = vv_normalize_scratch_bytes(n_clips, offsets[n_clips]) bytes of device memory; clips shorter than 2^24 samples. */
VV_API size_t vv_normalize_scratch_bytes(int n_clips, int64_t total_len);
VV_API int vv_normalize_clips(vv_ctx* ctx, const float* x, const int64_t* offsets, int n_clips, int64_t max_len, void* scratch,
                       int16_t* out, void* stream);

/* ---- N10 the output stage on the device: what the engine did on the host after vv_decode.  No call here synchronises;
 * descriptor rows live in device memory, so the library cannot check them: the CALLER validates them before the call
 * (runtime.HipSynth.join_chunks / pcm_resample / pcm_encode do).  The kernels clamp every index all the same. */
#define VV_JOIN_MAX_N 24576   /* the largest junction: the walk keeps that many joined samples in LDS */
/* AudioProcessor.concatenate_with_crossfade_improved(waves, cross_fade_duration, sample_rate) (reference core/audio_processor.py:122-192)
 * for R requests in one call, bit for bit: a request of one chunk is copied untouched; otherwise every raw chunk that holds a 32767 sample
 * becomes (int16)(x * (26214.0 / 32767)) (float64, truncated), and junction by junction, with n = min(int(cross_fade_duration *
 * sample_rate), joined so far, len(next)) > 0: rms = sqrtf(mean_f32(x_f32 * x_f32)) of the last n joined samples and of the first n of the
 * next chunk in numpy's float32 summation order; if both > 100 the WHOLE next chunk becomes (int16)(int32)(x_f32 * clamp(rms_prev /
 * rms_next, 0.7f, 1.5f)) (low 16 bits kept: a wrap is allowed, as numpy on x86); mixed[k] = (int16)(tail[k] * c[k] + head[k] * s[k]) in
 * float64.  The host owns every length, so it hands over
 *   chunk_rows  n_chunks x 8 int64 {src_off, len, pos, n, fin, tab_off, repair, req}: the chunk is pcm[src_off, +len) (a row of vv_decode's
 *               plane); pos = the position of its first sample in its request's joined signal (joined length before it - n); n = its
 *               junction size (0 for a request's first chunk and where cross_fade_duration <= 0); fin = its samples are final at positions
 *               < fin = the smallest pos of the request's later chunks (INT64_MAX for the last); tab_off = offset in doubles of its
 *               c[n] | s[n] tables in fade; repair = 1 in a request of two or more chunks; req = the index of its request
 *   req_rows    R x 4 int64 {chunk0, n_chunks, out_off, joined_len}: consecutive chunk rows; the result is out[out_off, +joined_len)
 *   fade        float64: per distinct n, c = cos(linspace(0, pi / 2, n)) ** 2 then s = sin(..) ** 2, computed by numpy ON THE HOST (the device
 *               never evaluates cos: a last-bit difference would flip a truncation)
 *   max_n, max_len   the largest n and len of the rows;  ws = 8 * n_chunks bytes of device scratch (8-byte aligned).
 * Every output sample of a request is written exactly once, nothing outside its slice, no atomics.  -22, and nothing is launched, for a
 * null pointer, R < 1, n_chunks < R, out not 16-byte aligned, max_n > VV_JOIN_MAX_N.  chunk_rows_host / req_rows_host (optional, both or
 * neither) = the same rows in HOST memory: the call then checks them itself and also returns -22 for a row that does not fit a buffer, an
 * n above max_n, and a chunk of len <= 0 inside a request of two or more chunks (the reference raises on an empty chunk in
 * fix_clipped_audio). */
VV_API int vv_join_chunks(vv_ctx* ctx, const int16_t* pcm, int64_t n_pcm, const int64_t* chunk_rows, const int64_t* chunk_rows_host,
                          int n_chunks, const int64_t* req_rows, const int64_t* req_rows_host, int R, const double* fade, int64_t n_fade,
                          int max_n, int64_t max_len, int16_t* out, int64_t n_out, void* ws, void* stream);
/* Output rate: batched int16 -> int16 polyphase FIR, y[m] = clamp(rint(sum_i x[i] * taps[(m + skip) * down - i * up]), -32768, 32767), one
 * float64 fma chain over ascending i (the arithmetic of vv_resample_poly), rint = ties to even.  taps = host-designed low-pass already scaled
 * by `up` (f64, device; voice_bank.resample_design).  rows = n_rows x 6 int64 {src_off, n_in, dst_off, n_out, m0, i0}: the row writes outputs
 * m0 ... m0 + n_out - 1 of a signal whose samples i0 ... i0 + n_in - 1 are x[src_off, +n_in); samples outside that range contribute zero (the
 * caller guarantees that the filter reaches none of them inside the signal).  A whole clip: m0 = i0 = 0, n_out = ceil(n_in * up / down).
 * max_out = the largest n_out.  NOT the reference's arithmetic: the reference has no output rate. */
VV_API int vv_pcm_resample(vv_ctx* ctx, const int16_t* x, int64_t n_x, const int64_t* rows, int n_rows, int64_t max_out, const double* taps,
                           int n_taps, int up, int down, int skip, int16_t* y, int64_t n_y, void* stream);
/* G.711: int16 -> uint8, kind 1 = mu-law, 2 = A-law, bit-exact to audioop.lin2ulaw(data, 2) / audioop.lin2alaw(data, 2) for all 65,536
 * inputs (the segment arithmetic of CPython's Modules/audioop.c).  rows = n_rows x 3 int64 {src_off, n, dst_off}; max_n = the largest n;
 * y 8-byte aligned. */
VV_API int vv_pcm_encode(vv_ctx* ctx, const int16_t* x, int64_t n_x, const int64_t* rows, int n_rows, int64_t max_n, int kind, uint8_t* y,
                         int64_t n_y, void* stream);


/* ---- N12 loudness normalisation of the joined signal: ITU-R BS.1770-4 integrated loudness with both gates, a gain to a
 * target level under a SAMPLE-peak ceiling, applied in HBM.  The arithmetic is pinned by core/audio_processor.py (normalize_loudness),
 * which the kernels equal bit for bit; the call never synchronises and reads nothing back.
 *   x        int16, the requests' joined signals at the model rate; sub = rate / 10 samples (a 100 ms sub-block), sub >= VV_LOUD_RUN
 *   rows     R x 4 int64 {src_off, n, dst_off, run_off} in device memory and the same rows in HOST memory (rows_host, checked by the call):
 *            request r is x[src_off, +n) -> y[dst_off, +n); run_off = the sum over the rows before it of
 *            (n / sub) * ceil(sub / VV_LOUD_RUN) + ceil((n % sub) / VV_LOUD_RUN), its first run in the scratch
 *   tables   43 float64 on the device, computed on the host for the rate (audio_processor.loudness_tables): the two biquads b1[3] a1[2]
 *            b2[3] a2[2], the zero-input run tables M_full[4][4] and M_last[4][4] (row major), ABS = 10^((-70 + 0.691) / 10)
 *   params   R x 2 float64 {T, c}: T = 10^((target + 0.691) / 10), T <= 0 = measure only; c = 32767 * 10^(peak_dbfs / 20)
 *   stats    R x 4 float64 {zbar, kept, P, g}: gated mean square, blocks kept, max |x|, the gain (exactly 1 when nothing is kept, T <= 0
 *            or P = 0).  The loudness itself, -0.691 + 10 log10(zbar), is the host's to compute.
 *   y        int16: y[i] = clamp(rint(x[i] * g), -32768, 32767) in float64, ties to even, written once each, nothing outside the rows.
 *            NULL = measure only; y == x with dst_off == src_off = in place.  Rows must not overlap on y (the caller's check).  y may start
 *            at any even byte: the 8-byte stores are laid on its address.
 *   ws       ws_bytes >= what vv_pcm_loudness_ws_bytes returns for the rows' total runs, 8-byte aligned.
 * -22, and nothing is launched, for sub < VV_LOUD_RUN, R < 1, a null or misaligned pointer, a ws that is too small, a row outside
 * n_x / n_y or with a wrong run_off. */
#define VV_LOUD_RUN 128
VV_API uint64_t vv_pcm_loudness_ws_bytes(int64_t total_runs, int R);
VV_API int vv_pcm_loudness(vv_ctx* ctx, const int16_t* x, int64_t n_x, const int64_t* rows, const int64_t* rows_host, int R, int64_t sub,
                           const double* tables, const double* params, int16_t* y, int64_t n_y, double* stats, void* ws, uint64_t ws_bytes,
                           void* stream);


/* ---- N13 look-ahead peak limiter of the joined signal: a sample-peak or 4x oversampled true-peak estimate, the gain
 * that holds it under the ceiling, a sliding minimum and a raised-cosine window average over the look-ahead L, applied in HBM.  The
 * arithmetic is pinned by core/audio_processor.py (limit_peaks), which the kernels equal bit for bit: all of it float64, every product
 * and sum rounded on its own, every sum in ascending order.  Per request, v = 0 outside [0, n) and every other index clamped to it:
 *     v[i] = x[i] * g
 *     e[i] = |v[i]|                                           (mode 0, "sample")
 *          = max(|v[i]|, |u1[i]|, |u2[i]|, |u3[i]|),  u_p[i] = sum_{j = -H+1 .. H} taps[4H + p - 4j] * v[i + j]      (mode 1, "true")
 *     r[i] = c / e[i] where e[i] > c, else 1;    m[i] = min r[i - L .. i + L];    A[i] = sum_{k = -L .. L} window[k + L] * (1 - m[i + k])
 *     s[i] = min(1 - A[i], r[i]);    y[i] = clamp(rint(v[i] * s[i]), -32768, 32767), ties to even
 * so max |y| <= ceil(c) for any input, s is exactly 1 wherever no e > c lies within 2L + H samples, and y[i] depends on
 * x[i - W .. i + W] only, W = 2L + VV_LIMIT_H: a block computed with W samples of context on each side equals the whole signal on its
 * interior, which is all a stream needs.  The call never synchronises and reads nothing back.
 *   x        int16, the requests' joined signals at the model rate
 *   rows     R x 5 int64 {src_off, n, dst_off, out_lo, out_n} in device memory and the same rows in HOST memory (rows_host, checked by
 *            the call): the limiter is computed over x[src_off, +n) as a whole signal; y[out_lo, out_lo + out_n) of it is written at
 *            y[dst_off, +out_n).  Plain use: out_lo = 0, out_n = n
 *   window   2L + 1 float64 on the device: 0.5 (1 + cos(pi k / (L + 1))) over its sum (audio_processor.limiter_window)
 *   taps     8 VV_LIMIT_H + 1 float64 on the device: sinc(k / 4) * kaiser(8H + 1, 8.0) (audio_processor.limiter_taps); read in mode 1
 *   params   R x 3 float64 {T, c, g0}: c = 32767 * 10^(peak_dbfs / 20); the pre-gain g = g0, or with meas given and T > 0
 *            (T = 10^((target + 0.691) / 10)) g = sqrt(T / zbar), NOT capped by the peak, exactly 1 when kept = 0 or P = 0
 *   meas     R x 4 float64 {zbar, kept, P, g}: the stats of a vv_pcm_loudness measure call on the same requests, read on the device; or NULL
 *   stats    R x 4 float64 {g, e_max, s_min, n_limited} over the row's n samples (n_limited = samples with s < 1); exact
 *   y        int16, written once each, nothing outside the rows' windows.  NULL = measure only; y == x with
 *            dst_off == src_off + out_lo = in place.  Rows must not overlap on y (the caller's check).  y may start at any even byte
 *   ws       ws_bytes >= vv_pcm_limit_ws_bytes(sum of n, sum of ceil(n / vv_pcm_limit_tile(L)), R), 8-byte aligned
 * -22, and nothing is launched, for no context, R < 1, L outside 1 ... VV_LIMIT_MAX_L, a mode other than 0 or 1, a null or misaligned
 * pointer, a ws that is too small, a negative field, out_lo + out_n > n, a row outside n_x / n_y.
 * Not bounded: the true peak of the OUTPUT (the gain curve and the rounding change the interpolation), and a later rate change. */
#define VV_LIMIT_H 12
#define VV_LIMIT_MAX_L 1024
VV_API int vv_pcm_limit_tile(int L);      /* samples per workgroup of the gain pass at look-ahead L (-22 outside 1 ... VV_LIMIT_MAX_L) */
VV_API uint64_t vv_pcm_limit_ws_bytes(int64_t total_samples, int64_t total_tiles, int R);
VV_API int vv_pcm_limit(vv_ctx* ctx, const int16_t* x, int64_t n_x, const int64_t* rows, const int64_t* rows_host, int R, int L, int mode,
                        const double* window, const double* taps, const double* params, const double* meas, int16_t* y, int64_t n_y,
                        double* stats, void* ws, uint64_t ws_bytes, void* stream);

/* ---- N14 pitch and tempo of the joined signal: a WSOLA time stretch by p / q; the pitch half is a vv_pcm_resample call
 * on its result.  The arithmetic is pinned by core/audio_processor.py (time_stretch), which the kernels equal bit for bit.  Per request,
 * with N = VV_WSOLA_N, HS = VV_WSOLA_HS, D = VV_WSOLA_D, x = 0 outside [0, n), n_s = ceil(n p / q), M = ceil(n_s / HS), pos_0 = -HS:
 *     for m = 1 ... M:  a_m = floor((m - 1) HS q / p);   c(d) = sum_{k < N} x[pos_{m-1} + HS + k] * x[a_m + d + k],  d = -D ... D - 1,
 *                       an exact integer;   pos_m = a_m + d*, d* = the largest c, among equals the smallest |d|, the negative one first
 *     for i < n_s:      m = i / HS + 1, k = i - (m - 1) HS;
 *                       y[i] = clamp(rint(window[k + HS] * x[pos_{m-1} + HS + k] + window[k] * x[pos_m + k]), -32768, 32767)
 * in float64, the two products rounded on their own, one sum, ties to even.  Every output sample is written exactly once.  The
 * correlation is not normalised.  p == q is NOT an identity of this recipe and is refused.  The call never synchronises and reads
 * nothing back.
 *   x        int16, the requests' joined signals
 *   rows     R x 6 int64 {src_off, n, dst_off, p, q, pos_off} in device memory and the same rows in HOST memory (rows_host, checked by
 *            the call): x[src_off, +n) is stretched to y[dst_off, +n_s), its frame positions go to pos[pos_off, +M + 1)
 *   window   VV_WSOLA_N float64 on the device: 0.5 - 0.5 cos(2 pi k / N) (audio_processor.wsola_window); the device evaluates no cosine
 *   y        int16, must not overlap x; nothing outside the rows' outputs is written.  y may start at any even byte.  NULL = the search
 *            alone: pos is written, no sample
 *   pos      int32 [n_pos]: pos_0 ... pos_M of every request, for the caller
 *   ws       ws_bytes >= vv_pcm_stretch_ws_bytes(R), 8-byte aligned
 * -22, and nothing is launched, for no context, R < 1, p == q, p or q outside 1 ... VV_WSOLA_MAX_PQ, p / q outside [1/4, 4], a null or
 * misaligned pointer, a ws that is too small, a negative field, n > 2^30, a row outside n_x / n_y / n_pos, rows that overlap on y or
 * on pos, y overlapping x. */
#define VV_WSOLA_N 512
#define VV_WSOLA_HS 256
#define VV_WSOLA_D 128
#define VV_WSOLA_MAX_PQ 2048
VV_API uint64_t vv_pcm_stretch_ws_bytes(int R);
VV_API int vv_pcm_stretch(vv_ctx* ctx, const int16_t* x, int64_t n_x, const int64_t* rows, const int64_t* rows_host, int R,
                          const double* window, int16_t* y, int64_t n_y, int32_t* pos, int64_t n_pos, void* ws, uint64_t ws_bytes,
                          void* stream);

/* ---- N15 FLAC output (RFC 9639): the final PCM of R requests as FLAC frames -- mono, 16 bits, frames of VV_FLAC_BLOCK
 * samples (the last one of a signal may be shorter), fixed predictors only.  The recipe is pinned by core/audio_processor.py
 * (flac_choose, flac_encode_frame), which the kernels equal byte for byte.  Per frame of m samples:
 *     constant    if and only if all samples are equal
 *     Fixed(o, po) o = 0 ... min(4, m - 1), po = 0 ... 4 with 2^po | m and (m >> po) > o: the o-th finite difference, Rice coded per
 *                 partition under the k in 0 ... 14 with the fewest bits (the lowest such k)
 *     verbatim    only when strictly smaller than every Fixed candidate
 * the fewest bits win, ties go to the lower o, then the lower po.  The escape code is never written.  Every frame carries its number
 * (frame0 + its index in the row), a CRC-8 of its header and a CRC-16 of the whole.  The stream header (fLaC + STREAMINFO, 42 bytes) is
 * the host's: audio_processor.flac_stream_header.  The call never synchronises and reads nothing back; no global atomics.
 *   x        int16, the requests' final signals
 *   rows     R x 4 int64 {src_off, n, frame0, last} in device memory and the same rows in HOST memory (rows_host, checked by the call):
 *            x[src_off, +n) becomes ceil(n / VV_FLAC_BLOCK) frames.  last = 0: a block of a stream, n a multiple of VV_FLAC_BLOCK
 *   y        uint8 [n_y]: the frames of all rows back to back from y[0], in row order; nothing at or beyond info[R][0] is written.
 *            n_y >= the sum of vv_flac_frame_bound over the frames.  Must not overlap x
 *   info     (R + 1) x 3 int64 on the device: row r = {byte offset of its first frame, smallest frame, largest frame in bytes},
 *            row R = {total bytes, 0, 0}
 *   ws       ws_bytes >= vv_pcm_flac_ws_bytes(sum of the rows' frames, R), 8-byte aligned
 * -22, and nothing is launched, for no context, R < 1 or R > 65535 (a row is one index of the launch grid), a null or misaligned pointer,
 * a negative field, n < 1, frame0 + frames > 2^31, last outside 0 / 1 or last = 0 with a partial frame, a row outside n_x, n_y below the sum of the frame bounds, a ws that is too small,
 * a rate outside 1 ... 655350, y overlapping x. */
#define VV_FLAC_BLOCK 4096
VV_API uint64_t vv_flac_frame_bound(int64_t m);      /* no frame of m samples (1 ... VV_FLAC_BLOCK) is longer; 0 outside that range */
VV_API uint64_t vv_pcm_flac_ws_bytes(int64_t total_frames, int R);
VV_API int vv_pcm_flac(vv_ctx* ctx, const int16_t* x, int64_t n_x, const int64_t* rows, const int64_t* rows_host, int R, int sample_rate,
                       uint8_t* y, int64_t n_y, int64_t* info, void* ws, uint64_t ws_bytes, void* stream);

/* ---- N16 LPC subframes for the FLAC output, opt-in: vv_pcm_flac with linear predictors of order 1 ... lpc_order among
 * the candidates of every frame that is not constant.  vv_pcm_flac itself is unchanged.  The recipe is pinned by core/audio_processor.py
 * (flac_lpc_coefficients, flac_choose(x, lpc_order)), which the kernels equal byte for byte.  Per frame of m >= 3 samples x:
 *     window      w[i] = ((i (m - 1 - i)) << 10) / A, A = h (m - 1 - h), h = (m - 1) / 2, in integers (Welch, 0 ... 1024); xw = x w
 *     lags        R[l] = sum xw[i] xw[i + l], l = 0 ... min(lpc_order, m - 1), exact in int64; R[0] = 0: no LPC candidate
 *     Levinson    float64, every operation rounded to nearest on its own (no fused multiply-add): err = R[0]; for p = 1, 2, ...:
 *                 acc = R[p] - a[1] R[p - 1] - ... - a[p - 1] R[1] (in that order), k = acc / err, a'[j] = a[j] - k a[p - j], a'[p] = k,
 *                 err = err (1 - k k); not err > 0 ends the candidates at order p
 *     quantise    12 bits: shift = min(11 - e, 15) with max |a[j]| = f 2^e, 0.5 <= f < 1 (shift < 0 or a maximum of 0: no candidate at
 *                 this order); fe = 0; for j = 1 ... p: fe += a[j] 2^shift, q[j] = clamp(floor(fe + 0.5), -2048, 2047), fe -= q[j]
 *     residual    r[n] = x[n] - ((sum q[j] x[n - j]) >> shift), n >= p, arithmetic shift; Rice coded exactly as for Fixed
 *     size        8 + 16 p + 4 + 5 + 12 p + 6 + the partitions
 * the fewest bits win among constant / Fixed / LPC / verbatim; ties go to Fixed before LPC, then the lower order, then the lower po;
 * verbatim only when strictly smaller than all others: no frame is larger than vv_pcm_flac's.  Subframe: header byte (32 | (p - 1)) << 1,
 * p warm-up samples, precision - 1 = 11 (4 bits), shift (5 bits), q[1] ... q[p] (12 bits each, two's complement), the residual.
 * Arguments, results and refusals as for vv_pcm_flac, with ws_bytes >= vv_pcm_flac_lpc_ws_bytes(sum of the rows' frames, R, lpc_order);
 * also -22 for lpc_order outside 1 ... VV_FLAC_MAX_LPC_ORDER (the workspace function then returns 0). */
#define VV_FLAC_MAX_LPC_ORDER 12
VV_API uint64_t vv_pcm_flac_lpc_ws_bytes(int64_t total_frames, int R, int lpc_order);
VV_API int vv_pcm_flac_lpc(vv_ctx* ctx, const int16_t* x, int64_t n_x, const int64_t* rows, const int64_t* rows_host, int R, int sample_rate,
                           int lpc_order, uint8_t* y, int64_t n_y, int64_t* info, void* ws, uint64_t ws_bytes, void* stream);

/* ---- N17 FLAC input (RFC 9639): reference clips stored as FLAC become the interleaved PCM vv_ingest_pcm reads, on the
 * device -- 1 ... 8 channels, 8 / 16 / 24 bits, constant / verbatim / Fixed 0 ... 4 / LPC 1 ... 32 subframes, wasted bits, residual methods 0
 * and 1 with partition orders 0 ... 15 and escape partitions, fixed and variable blocking.  The recipe is pinned by core/audio_processor.py
 * (flac_container, flac_frame_index, flac_decode), which the kernels equal sample for sample, and in reason code and byte for a refusal:
 *   host     the container: optional ID3v2 tag, "fLaC", metadata blocks (STREAMINFO first; the rest skipped); one row per clip
 *   chain    frame 0 starts at the clip's first byte, every next frame at the byte after the previous CRC-16; a sync code anywhere else
 *            is not a frame.  total > 0: the chain ends when that many samples came (bytes behind are ignored) and must meet it exactly;
 *            total = 0: the chain must end exactly at the clip's last byte
 *   header   in this order: sync 0xFFF8 | blocking bit; reserved bit, block-size code 0, rate code 15, channel code > 10, depth code 3,
 *            reserved bit (VV_FLAC_RESERVED); the coded number, 1 ... 7 bytes, syntax only; the 8- / 16-bit block size - 1 (65536 is
 *            reserved); the 8- / 16-bit rate (kHz, Hz, tens of Hz); CRC-8 (poly 0x07); then channels, depth and rate equal to the row's,
 *            the blocking bit equal to the clip's first, block <= max block (VV_FLAC_BAD_HEADER)
 *   measure  per subframe: pad bit 0, type (0 constant, 1 verbatim, 8 ... 12 Fixed, 32 ... 63 LPC; others reserved), wasted flag and unary
 *            count (wasted < depth), warm-up samples, LPC: precision - 1 (15 reserved), shift (5 bits signed, negative refused),
 *            coefficients; residual: method (2, 3 reserved), partition order po with 2^po | block and block >> po >= order
 *            (VV_FLAC_PARTITION), per partition a parameter of 4 / 5 bits (all ones = escape: 5 bits raw width, then raw samples) and Rice
 *            codes (unary quotient, then the low bits).  Then zero bits to the byte and the CRC-16 (poly 0x8005).  Nothing at or past
 *            min(clip end, frame start + vv_flac_decode_frame_bound) is read: VV_FLAC_OVERRUN / VV_FLAC_FRAME_TOO_LONG
 *   restore  only after every clip's chain passed: prediction sums in 64 bits, arithmetic shift, + residual; each restored sample must
 *            fit depth - wasted bits (VV_FLAC_RANGE; the side channel has one bit more), then << wasted
 *   channels left/side, side/right, mid/side ((mid << 1 | side & 1) +- side) >> 1; 8 bits -> int8, 16 -> int16 LE, 24 -> int32 LE with the
 *            sign pad in the lowest byte and the sample above it; a value outside the width wraps.  The MD5 is not verified.
 * A refusal's byte is the first byte of the frame that holds the problem (chain: where the next frame was expected), from the clip's first.
 *   data     the frame bytes of the R clips, each 4-byte aligned, 8 bytes of padding behind the last clip; 8-byte aligned
 *   rows     R x 8 int64 on the device, rows_host the same on the host (checked before a launch): {byte offset, n_bytes, channels, bits,
 *            min block, max block, rate, total samples (0 = unknown)}, ascending
 *   info     R x 4 int64 (device): {status, byte, frames, samples}; the host reads it between the two calls
 *   ws       ws_bytes >= vv_flac_index_ws_bytes(n_bytes, R); vv_flac_decode reads the frame table vv_flac_index left there
 *   lay      R x 6 int64 (device, and lay_host): {pcm byte offset, frames, samples, frames in front, samples x channels in front, samples
 *            in front}; a refused clip has frames = samples = 0
 *   info2    R x 2 int64 (device): {status, byte} of the first frame that failed the range check
 *   ws2      ws2_bytes >= vv_flac_decode_ws_bytes(sum of samples x channels, sum of frames)
 * -22 and nothing launched: null or misaligned pointers, rows outside the buffers, R outside 1 ... 65535, a workspace too small,
 * overlapping buffers.  No global atomics; the result does not depend on the batch. */
#define VV_FLAC_MAX_CLIP 67108864
enum { VV_FLAC_OK = 0, VV_FLAC_BAD_HEADER = 1, VV_FLAC_CRC8 = 2, VV_FLAC_CRC16 = 3, VV_FLAC_RESERVED = 4, VV_FLAC_PARTITION = 5, VV_FLAC_RANGE = 6,
       VV_FLAC_OVERRUN = 7, VV_FLAC_CHAIN = 8, VV_FLAC_FRAME_TOO_LONG = 9, VV_FLAC_CLIP_TOO_LONG = 10 };
VV_API uint64_t vv_flac_decode_frame_bound(int block, int channels, int bits);      /* 2 x the verbatim frame + 64; 0 for sizes out of range */
VV_API uint64_t vv_flac_index_ws_bytes(int64_t n_bytes, int R);
VV_API uint64_t vv_flac_decode_ws_bytes(int64_t plane_samples, int64_t total_frames);
VV_API int vv_flac_index(vv_ctx* ctx, const uint8_t* data, int64_t n_bytes, const int64_t* rows, const int64_t* rows_host, int R, int64_t* info,
                         void* ws, uint64_t ws_bytes, void* stream);
VV_API int vv_flac_decode(vv_ctx* ctx, const uint8_t* data, int64_t n_bytes, const int64_t* rows, const int64_t* rows_host, int R, const int64_t* lay,
                          const int64_t* lay_host, const void* ws, uint64_t ws_bytes, uint8_t* pcm, int64_t n_pcm, int64_t* info2, void* ws2,
                          uint64_t ws2_bytes, void* stream);

/* ---- N25 IMA ADPCM output, and IMA ADPCM / G.711 reference clips.  The arithmetic is the Intel/DVI coder of CPython's
 * Modules/audioop.c (lin2adpcm, adpcm2lin, ulaw2lin, alaw2lin), restated by core/audio_processor.py (adpcm_encode_blocks,
 * adpcm_decode_frames, ulaw2lin, alaw2lin), which the kernels equal byte for byte and sample for sample.  Integers only.
 * vv_pcm_adpcm: the blocks of a mono WAVE file with format tag 0x11 for R final signals.
 *   samples_per_block   spb = 8 k + 1 in 9 ... 8185; a block is {int16 first sample, uint8 step index, uint8 0} and (spb - 1) / 2 bytes of
 *            codes, low nibble first: (spb - 1) / 2 + 4 <= VV_ADPCM_MAX_BLOCK_ALIGN bytes
 *   rows     R x 3 int64 on the device, rows_host the same on the host (checked before a launch): {src_off, n >= 1, dst_off in bytes,
 *            a multiple of 4}: x[src_off, +n) becomes ceil(n / spb) blocks at y + dst_off, the last one padded with its last sample;
 *            the rows' blocks lie in ascending order on y, disjoint
 *   search   the header's step index is free: each block tries all 89 and keeps the one with the smallest sum of (x - decoded)^2 over its
 *            real samples, the smallest index of equals.  Blocks are independent: a request alone equals itself in a batch, and a stream
 *            cut at block boundaries equals the whole signal
 *   y        n_y bytes, 8-byte aligned, must not overlap x; the size is known on the host, so nothing is read back but the bytes
 * vv_wav_decode: the coded data chunks of R WAVE clips -> the interleaved int16 frames vv_ingest_pcm reads at width 2.
 *   data     the clips' data chunks, each at a 16-byte aligned offset; 16-byte aligned
 *   rows     R x 8 int64 (device, and rows_host): {data byte offset, n_bytes, format tag (6 A-law, 7 mu-law, 0x11 IMA ADPCM), channels,
 *            nBlockAlign (ADPCM: a multiple of 4 x channels, >= 8 x channels; 1 or 2 channels), frames to write (at most what the bytes
 *            hold: a fact chunk may state fewer), pcm byte offset (16-byte aligned, ascending), 0}
 *   ADPCM    per channel a 4-byte header, then rounds of 4 bytes (8 samples) per channel; a trailing part of a block decodes the codes
 *            it holds; one lane per (block, channel)
 *   status   R x 2 int64 (device): {0, 0}, or {VV_WAV_STEP_INDEX, the byte of the first header step index above 88, from the clip's first
 *            data byte}.  Such a clip's PCM is undefined inside its own frames; nothing outside them is written, other clips are intact
 * -22 and nothing launched: null or misaligned pointers, rows outside the buffers, R outside 1 ... 65535, overlapping buffers. */
#define VV_ADPCM_MAX_BLOCK_ALIGN 4096
#define VV_WAVE_TAG_ALAW 6
#define VV_WAVE_TAG_ULAW 7
#define VV_WAVE_TAG_ADPCM 17
enum { VV_WAV_OK = 0, VV_WAV_STEP_INDEX = 1, VV_WAV_BLOCK_ALIGN = 2, VV_WAV_BITS = 3, VV_WAV_CHANNELS = 4 };
VV_API int vv_pcm_adpcm(vv_ctx* ctx, const int16_t* x, int64_t n_x, const int64_t* rows, const int64_t* rows_host, int R, int samples_per_block,
                        uint8_t* y, int64_t n_y, void* stream);
VV_API int vv_wav_decode(vv_ctx* ctx, const uint8_t* data, int64_t n_bytes, const int64_t* rows, const int64_t* rows_host, int R, uint8_t* pcm,
                         int64_t n_pcm, int64_t* status, void* stream);

/* ---- N18 formant-preserving pitch shift: the envelope correction behind the rate conversion that makes the pitch.  x is a
 * request's joined signal (n samples), y what the prosody step made of it (n_f = ceil(n td / tn) samples, tn / td the tempo fraction), z the
 * result: y filtered so that its LPC envelope is x's again.  The arithmetic is pinned by core/audio_processor.py (formant_filters,
 * apply_formant_filters), which the kernels equal bit for bit.  With P, NA, H, L below, M = ceil(n_f / H), per frame m = 0 ... M and for
 * each of (s, c) = (y, m H) and (x, floor(m H tn / td)), s = 0 outside the signal:
 *     d[k] = s[c - NA/2 + k] - s[c - NA/2 + k - 1];  xw[k] = rint(wa[k] d[k]) as an integer;  R[l] = sum_{k >= l} xw[k] xw[k - l], l <= P, exact
 *     flat if R[0] = 0; else Rf[0] = R[0] + R[0] 2^-20 and the Levinson recurrence of N16 up to order P; flat if err is ever not > 0
 *     A[0] = 1, A[k] = -(a[k] g[k])
 * per frame:  r[t] = (t <= P ? A_y[t] : 0) - A_x[1] r[t - 1] - ... - A_x[min(t, P)] r[t - min(t, P)], t < L (k ascending);
 *             h_m[t] = sqrt(err_x / err_y) r[t]; either analysis flat: h_m = the unit impulse
 * per sample i < n_f, m = i / H + 1, k = i - (m - 1) H:  v_a = sum_{j < L} h_{m-1}[j] y[i - j], v_b with h_m, each from +0.0 with j
 *             ascending, y = 0 in front of the signal;  z[i] = clamp(rint(window[k + H] v_a + window[k] v_b), -32768, 32767)
 * in float64, every operation rounded on its own (no fused multiply-add), ties to even.  The call never synchronises and reads nothing back.
 *   x, y     int16, the signals before and after the prosody step
 *   rows     R x 7 int64 {x_off, n, y_off, n_f, z_off, tn, td} in device memory and the same rows in HOST memory (rows_host, checked by the
 *            call)
 *   wa       VV_FORMANT_NA float64 on the device: 0.5 - 0.5 cos(2 pi k / NA);  g: VV_FORMANT_P + 1 float64: g[0] = 1, g[k] = g[k - 1] * 0.995
 *            (audio_processor.formant_tables);  window: the VV_WSOLA_N float64 of vv_pcm_stretch.  The device evaluates no cosine, no power
 *   z        int16 [n_z], must overlap neither x nor y; nothing outside the rows' outputs is written.  z may start at any even byte
 *   h_out    NULL, or float64 [n_h] for a test: every frame's L taps, request after request, M + 1 frames each
 *   ws       ws_bytes >= vv_pcm_formant_ws_bytes(sum of M + 1, R), 8-byte aligned
 * -22, and nothing is launched, for no context, R < 1 or R > 65535, a null or misaligned pointer, a ws or an h_out that is too small, a
 * negative field, n > 2^30, tn or td outside 1 ... VV_WSOLA_MAX_PQ, n_f != ceil(n td / tn), a row outside n_x / n_y / n_z, rows that overlap
 * on z, z overlapping x or y. */
#define VV_FORMANT_P 24
#define VV_FORMANT_NA 1024
#define VV_FORMANT_H 256
#define VV_FORMANT_L 2048
VV_API uint64_t vv_pcm_formant_ws_bytes(int64_t total_frames, int R);
VV_API int vv_pcm_formant(vv_ctx* ctx, const int16_t* x, int64_t n_x, const int16_t* y, int64_t n_y, const int64_t* rows,
                          const int64_t* rows_host, int R, const double* wa, const double* g, const double* window, int16_t* z, int64_t n_z,
                          double* h_out, int64_t n_h, void* ws, uint64_t ws_bytes, void* stream);

/* ---- N19 vocoder-bias denoiser: spectral subtraction against a stationary profile, first in the output chain (behind the
 * join, before pitch and tempo).  bias is the magnitude spectrum the vocoder emits for an empty mel (vv_pcm_denoise_bias of that output), or
 * the caller's own.  The arithmetic is pinned by core/audio_processor.py (denoise_fft, denoise_pcm, denoise_bias), which the kernels equal
 * bit for bit.  With N, H below, x a request's n int16 samples (0 outside), M = ceil(n / H), frames f = 0 ... M + 2 starting at (f - 3) H:
 *     transform: radix-2 decimation in time behind a bit reversal, stages of half-length h = 1, 2, ... N / 2; per butterfly (a, b) with
 *                (c, s) = twiddles[j N / (2 h)]:  tr = br c - bi s;  ti = br s + bi c;  a' = a + t;  b' = a - t  (the stages with c = 1, s = 0
 *                carry their products out like the others); the inverse negates s and does not scale
 *     per frame: forward transform of w[k] x[(f - 3) H + k] with a zero imaginary part; for all N bins mag = sqrt(re re + im im),
 *                d = mag - strength bias[k <= N / 2 ? k : N - k], g = d > 0 ? d / mag : 0, re g and im g; inverse transform; real part times w[k]
 *     per hop i < M: acc = +0.0, then the contributions of frames i, i + 1, i + 2, i + 3 in that order;
 *                y = clamp(rint(acc / 1536), -32768, 32767) for the samples of the hop inside n
 *     bias of a signal: per bin 0 ... N / 2 the sum of mag over the full frames (start f H >= 0, f H + N <= n) from +0.0 with f ascending,
 *                divided by their count
 * in float64, every operation rounded on its own (no fused multiply-add), ties to even.  Strength 0, or an all-zero bias, gives the input
 * back sample for sample (computed, not short-circuited).  The calls never synchronise and read nothing back.
 *   rows       R x 4 int64 {x_off, n, y_off, bias_row} in device memory and the same rows in HOST memory (rows_host, checked by the call)
 *   strengths  R float64 in device memory and the same values in HOST memory (strengths_host, checked by the call): 0 ... 16
 *   bias       n_bias x 513 float64 on the device;  window: N float64, 0.5 - 0.5 cos(2 pi k / N);  twiddles: N float64, cos(2 pi k / N) for
 *              k < N / 2, then -sin(2 pi k / N) (audio_processor.denoise_tables).  The device evaluates no cosine, no sine
 *   y          int16 [n_y], must not overlap x (a hop reads the input under its neighbours); nothing outside the rows' outputs is written
 *   mag_out    NULL, or float64 [n_mag] for a test: the N magnitudes of every frame, request after request, M + 3 frames each
 *   ws         ws_bytes >= vv_pcm_denoise_ws_bytes(R), 8-byte aligned
 * vv_pcm_denoise_bias takes the same rows (y_off and bias_row are not used) and writes R x 513 float64 to out [n_out]; a signal needs
 * N <= n <= VV_DENOISE_BIAS_MAX_N; ws_bytes >= vv_pcm_denoise_bias_ws_bytes(sum of the full frames, R).
 * -22, and nothing is launched, for no context, R < 1 or R > 65535, a null or misaligned pointer, a ws, a mag_out or an out that is too small,
 * a negative field, n > 2^30, bias_row outside n_bias, a strength that is negative, not finite or above 16, a row outside n_x / n_y, rows that
 * overlap on y, y overlapping x; for the bias a signal without a full frame or above the limit. */
#define VV_DENOISE_N 1024
#define VV_DENOISE_H 256
#define VV_DENOISE_BIAS_MAX_N 1048576
VV_API uint64_t vv_pcm_denoise_ws_bytes(int R);
VV_API int vv_pcm_denoise(vv_ctx* ctx, const int16_t* x, int64_t n_x, const int64_t* rows, const int64_t* rows_host, int R, const double* strengths,
                          const double* strengths_host, const double* bias, int64_t n_bias, const double* window, const double* twiddles, int16_t* y,
                          int64_t n_y, double* mag_out, int64_t n_mag, void* ws, uint64_t ws_bytes, void* stream);
VV_API uint64_t vv_pcm_denoise_bias_ws_bytes(int64_t total_frames, int R);
VV_API int vv_pcm_denoise_bias(vv_ctx* ctx, const int16_t* x, int64_t n_x, const int64_t* rows, const int64_t* rows_host, int R, const double* window,
                               const double* twiddles, double* out, int64_t n_out, void* ws, uint64_t ws_bytes, void* stream);

/* ---- N22 keyed audio watermark: a multiplicative spread-spectrum mark on the frames of N19 (N, H, window, transform and
 * scale 1536 as above), embedded behind pitch and tempo and before the loudness step, and its detector.  The arithmetic is pinned by
 * core/audio_processor.py (watermark_embed, watermark_cells, watermark_stats), which the kernels equal bit for bit.  A cell is (frame f, band
 * bin k), LO <= k < LO + K; at alignment q its group is g = ((f + q) / G) % P, its bit index j = (k - LO + 7 g) % NB and its chip
 * chips[g K + k - LO] (+1 or -1, made from a 64-bit key on the HOST by audio_processor.watermark_chips: the device hashes nothing).  The
 * message is 24 bits, bit j = bit 23 - j of (payload << 8 | CRC-8 of the payload's two big-endian bytes, polynomial 0x07, initial value 0).
 *     embed  per frame: forward transform; re and im of the band bins k and of their mirrors N - k times (chip > 0) == (bit j set) ? gp : gm
 *            at q = 0, every other bin times 1.0; inverse transform, window, overlap-add, y = clamp(rint(acc / 1536)) as N19.  gp = 1 + a
 *            and gm = 1 - a are made by the caller, 0 <= a <= 0.5; a = 0 gives the input back sample for sample (computed, not short-circuited)
 *     detect m[f][k] = the band magnitudes of the F = M + 3 frames; r = 0.5 (m[max(f - G, 0)][k] + m[min(f + G, F - 1)][k]);
 *            d = (int32) rint(32768 (m - r) / (m + r + 1.0)), float64, every operation rounded on its own; for every alignment q < P G and
 *            bit j: num = sum of chip d, den = sum of d d over the cells of bit j (int64) -> stats [R][P G][NB]{num, den}
 * The calls never synchronise and read nothing back; the decision (z = num / sqrt(den), the score, the CRC) is the host's.
 *   rows       R x 4 int64 in device memory and the same rows in HOST memory (rows_host, checked by the call): {x_off, n, y_off, message}
 *              for vv_pcm_watermark, {x_off, n, 0, 0} for vv_pcm_watermark_detect
 *   chips      int8 [n_chips >= P K] on the device, 4-byte aligned;  window, twiddles: as for vv_pcm_denoise
 *   y          int16 [n_y], must not overlap x; nothing outside the rows' outputs is written
 *   stats      int64 [n_stats >= R P G NB 2];  cells_out: NULL, or int32 [n_cells] for a test: the K cell values of every frame, request after
 *              request, M + 3 frames each
 *   ws         ws_bytes >= vv_pcm_watermark_ws_bytes(R) / vv_pcm_watermark_detect_ws_bytes(sum of M + 3, R), 8-byte aligned
 * -22, and nothing is launched, for no context, R < 1 or R > 65535, a null or misaligned pointer, a chips, ws, stats or cells_out that is too
 * small, a negative field, n > 2^30 (detect: n > VV_WATERMARK_DETECT_MAX_N), a message above 2^24 - 1, gains outside 1 <= gp <= 1.5 and
 * 0.5 <= gm <= 1 (a NaN included), a row outside n_x / n_y, rows that overlap on y, y overlapping x. */
#define VV_WATERMARK_LO 22
#define VV_WATERMARK_K 320
#define VV_WATERMARK_G 4
#define VV_WATERMARK_P 64
#define VV_WATERMARK_NB 24
#define VV_WATERMARK_DETECT_MAX_N 16777216
VV_API uint64_t vv_pcm_watermark_ws_bytes(int R);
VV_API int vv_pcm_watermark(vv_ctx* ctx, const int16_t* x, int64_t n_x, const int64_t* rows, const int64_t* rows_host, int R, const int8_t* chips,
                            int64_t n_chips, double gp, double gm, const double* window, const double* twiddles, int16_t* y, int64_t n_y, void* ws,
                            uint64_t ws_bytes, void* stream);
VV_API uint64_t vv_pcm_watermark_detect_ws_bytes(int64_t total_frames, int R);
VV_API int vv_pcm_watermark_detect(vv_ctx* ctx, const int16_t* x, int64_t n_x, const int64_t* rows, const int64_t* rows_host, int R,
                                   const int8_t* chips, int64_t n_chips, const double* window, const double* twiddles, int64_t* stats,
                                   int64_t n_stats, int32_t* cells_out, int64_t n_cells, void* ws, uint64_t ws_bytes, void* stream);

#ifdef __cplusplus
}
#endif
#endif
