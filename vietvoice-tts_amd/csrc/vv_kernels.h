// Internal launcher interface between the kernel translation units and vv_api.hip.
// Every launcher validates operand shapes on the host BEFORE launching (a faulting kernel can
// reset the whole box) and returns 0 / negative errno with a static message in *err.
#pragma once
#include <hip/hip_runtime.h>
#include <algorithm>
#include "../../include/vvtts.h"

typedef vv_gemm_args vvk_gemm_args;

int vvk_gemm(const vv_gemm_args* g, hipStream_t st, const char** err);
void vvk_gemm_tail_plan(int M, int N, int K, int lda, int ldw, int ldc, int* row0, int* parts);
int vvk_attention(const vv_attn_args* a, hipStream_t st, const char** err);
int vvk_ln_mod(const vv_ln_args* a, hipStream_t st, const char** err);
int vvk_posconv(const vv_posconv_args* a, hipStream_t st, const char** err);
int vvk_conv(const vv_conv_args* a, hipStream_t st, const char** err);
int vvk_conv_x3(const vv_conv_args* a, hipStream_t st, const char** err);
size_t vvk_conv_split_bytes(int Cin_pad, int KW, int rows_pad);
int vvk_conv_split_weights(const float* Wt, int Cin_pad, int KW, int rows_pad, void* Wb, hipStream_t st, const char** err);
int vvk_mrf_pair(const vv_mrf_args* a, hipStream_t st, const char** err);
int vvk_conv_post(const float* in, const float* w, float bias, int16_t* pcm, int ld_pcm, float* wave_f32, int B, int C, int T,
                  int KW, float pre_slope, const int* len_in, hipStream_t st, const char** err);
int vvk_mel_slice(const float* x, int B, int N, int n_mel, const int* ref_len, const int* seq_len, float* out, int T,
                  hipStream_t st, const char** err);
int vvk_mel(const int16_t* audio, int ld_audio, const int* audio_len, const float* window, const float* tw_cos,
            const float* tw_sin, const float* fb, float* mel, int B, int F_max, int n_fft, int hop, int n_mel, hipStream_t st,
            const char** err);
int vvk_pack_cat(int dtype, const float* x, const float* cat, const float* cat_drop, void* out, int ldo, int BN, int n_mel,
                 int cond_dim, int only_x, const int* row_src, hipStream_t st, const char** err);
int vvk_cfg_euler(float* x, const float* pred, int ldp, int BN, int n_mel, float cfg, float dt, const int* row_src, hipStream_t st,
                  const char** err);
// u_row (N8, optional [Rc] device): conditional packed row -> the row of pred that holds its unconditional prediction, -1 = none (k = pc)
// apg (N11, optional): the item coefficients {A, C} and the evaluation state of the projected combine
// k_out_ring != 0 (N20, the steps driver under a multistep plan): a->k_out may be the buffer of one of the earlier slopes
// reuse (N21, optional; needs u_row, never with apg): the buffer of the kept guidance differences and the items' modes (HOST, kernel arguments)
// norm_coef (N24, optional; needs u_row, never with apg or reuse): the items' {s, f} of cfg_norm_coef_kernel, device [items][2] fp32
int vvk_ode_stage(const vv_ode_stage_args* a, const int* u_row, const vv_apg_stage_args* apg, hipStream_t st, const char** err, int k_out_ring = 0,
                  const vv_reuse_stage_args* reuse = nullptr, const float* norm_coef = nullptr);
// N24: cfg_gram_reduce_kernel (which & 1) and cfg_norm_coef_kernel (which & 2) of one evaluation
int vvk_cfg_norm_coef(const vv_cfg_norm_coef_args* a, int which, hipStream_t st, const char** err);
// N21: the drift report -- which & 1: cfg_drift_reduce_kernel, which & 2: the item sums
int vvk_cfg_drift_reduce(const vv_cfg_drift_args* a, int which, hipStream_t st, const char** err);
// N23 block caching: one MARK / DIFF / APPLY launch of the span kernel; the report -- which & 1: block_drift_reduce_kernel, which & 2: the
// sequence sums, which == 4: zeros in their place
int vvk_block_span(const vv_block_span_args* a, hipStream_t st, const char** err);
int vvk_block_drift_reduce(const vv_block_drift_args* a, int which, hipStream_t st, const char** err);
// N20: the step report -- which & 1: ode_diff_reduce_kernel, which & 2: the item sums
int vvk_ode_diff_reduce(const vv_ode_diff_args* a, int which, hipStream_t st, const char** err);
// N11: apg_reduce_kernel (which & 1) and apg_coef_kernel (which & 2) of one evaluation
int vvk_apg_coef(const vv_apg_coef_args* a, int which, hipStream_t st, const char** err);
// N8 guidance subsets: flags [B] on the HOST (they travel as kernel arguments), at most VVK_GUIDE_MAX_ITEMS items per launch
#define VVK_GUIDE_MAX_ITEMS 1024
int vvk_guided_tables(const int* seq_len, const unsigned char* flags, int B, int N, int Rc, int Ru, int* row_start, int* rs_rel, int* kv_len,
                      int* row_pos, int* u_src, int* u_crow, int* u_row, hipStream_t st, const char** err);
int vvk_pack_cat_guided(int dtype, const float* x, const float* cat, const float* cat_drop, void* out, int ldo, int Rc, int row0, int n_rows,
                        int n_mel, int cond_dim, int only_x, int x_packed, const int* row_src, const int* u_src, const int* u_crow,
                        hipStream_t st, const char** err);
int vvk_text_embed(const int* ids, int ld_ids, const int* text_len, const float* emb, const float* pos, float* out, int B, int N,
                   int Dt, int vocab_rows, hipStream_t st, const char** err);
int vvk_dwconv(const float* in, float* out, const float* w, const float* bias, const int* seq_len, int B, int n_seq, int N, int C,
               int KW, hipStream_t st, const char** err);
int vvk_grn(int dtype, void* x, float* sumsq, const float* gamma, const float* beta, const int* seq_len, int B, int n_seq, int N,
            int C, hipStream_t st, const char** err);
// keep (optional, [B][ld_keep] device, ld_keep >= N): speech editing's frame mask -- the mel only where keep[b][t] as well
int vvk_build_cat(const float* mel, int F_max, const int* ref_len, const float* text, float* cat, float* cat_drop, int B, int N,
                  int n_mel, int Dt, hipStream_t st, const char** err, const uint8_t* keep = nullptr, int ld_keep = 0);
int vvk_ref_len(const int* audio_len, int* ref_len, int B, int hop, hipStream_t st, const char** err);
// N, T_max: the item's rows and the level-0 plane's columns -- the frame count is clamped to both, as mel_slice_kernel's slice is
int vvk_decode_len(const int* seq_len, const int* ref_len, int* lens, int B, int n_levels, const int* mult, int N, int T_max, hipStream_t st,
                   const char** err);
int vvk_row_tables(const int* seq_len, int B, int N, int Rc, int* row_start, int* row_src, int* row_pos, int* kv_len, hipStream_t st, const char** err);
int vvk_resample_poly(const float* x, int n_in, const double* h, int n_taps, int up, int down, int skip, float* y, int n_out,
                      hipStream_t st, const char** err);
int vvk_ingest_pcm(const void* pcm, const long long* desc, int n_clips, long long max_out, float* out, hipStream_t st, const char** err);
size_t vvk_normalize_scratch_bytes(int n_clips, long long total_len);
int vvk_normalize_clips(const float* x, const long long* off, int n_clips, long long max_len, void* scratch, int16_t* out,
                        hipStream_t st, const char** err);
int vvk_rope_compact(const float* c, const float* s, float* out, int n, hipStream_t st, const char** err);
int vvk_rope_rows(const float* cs, const int* pos, float* out, int rows, hipStream_t st, const char** err);
int vvk_groupnorm(const float* x, float* y, const float* gamma, const float* beta, int B, int C, int T, int G, float eps, int act,
                  hipStream_t st, const char** err);
// N5 speech editing (vv_edit.hip).  Splice rows are {item, src_off, dst_off, n} (n_rows x 4 int64, device), validated by the caller.
int vvk_edit_splice(const int16_t* src, long long n_src, const long long* desc, int n_rows, int B, int16_t* out, int ld_out,
                    hipStream_t st, const char** err);
int vvk_edit_restore(float* x, const float* cat, const uint8_t* keep, int ld_keep, const int* seq_len, int B, int N, int n_mel, int cd,
                     hipStream_t st, const char** err);
// N9 start noise on the device (vv_noise.hip): Philox4x32-10 keyed per item, keys [B][2] = {seed, stream} in device memory
int vvk_noise_fill(float* x, const int* seq_len, const unsigned long long* keys, int B, int N, int n_mel, int kind, hipStream_t st,
                   const char** err);
// N10 output stage (vv_output.hip): chunk join (rows validated by the caller), int16 polyphase rate conversion, G.711
int vvk_join_max_n();
int vvk_join_chunks(const int16_t* pcm, long long n_pcm, const long long* chunk_rows, int n_chunks, const long long* req_rows, int R,
                    const double* fade, long long n_fade, int max_n, long long max_len, int16_t* out, long long n_out, void* ws,
                    hipStream_t st, const char** err);
int vvk_pcm_resample(const int16_t* x, long long n_x, const long long* rows, int n_rows, long long max_out, const double* taps, int n_taps,
                     int up, int down, int skip, int16_t* y, long long n_y, hipStream_t st, const char** err);
int vvk_pcm_encode(const int16_t* x, long long n_x, const long long* rows, int n_rows, long long max_n, int kind, uint8_t* y, long long n_y,
                   hipStream_t st, const char** err);
// N12 loudness normalisation (vv_loudness.hip): BS.1770 gated measurement by runs of 128 samples, gain under a peak ceiling, apply
unsigned long long vvk_pcm_loudness_ws_bytes(long long total_runs, int R);
int vvk_pcm_loudness(const int16_t* x, long long n_x, const long long* rows, int R, long long sub, long long total_runs, long long max_n,
                     const double* tables, const double* params, int16_t* y, long long n_y, double* stats, void* ws, hipStream_t st,
                     const char** err);
// N13 look-ahead peak limiter (vv_limiter.hip): gain plane by tiles (tile = vvk_pcm_limit_tile(L) samples), per-request stats, apply
int vvk_pcm_limit_tile(int L);
unsigned long long vvk_pcm_limit_ws_bytes(long long total_samples, long long total_tiles, int R);
int vvk_pcm_limit(const int16_t* x, long long n_x, const long long* rows, int R, int L, int mode, long long total_samples,
                  long long total_tiles, long long max_tiles, long long max_out, const double* window, const double* taps,
                  const double* params, const double* meas, int16_t* y, long long n_y, double* stats, void* ws, hipStream_t st,
                  const char** err);
// N14 WSOLA time stretch (vv_prosody.hip): the sequential frame search per request, then the blend; rows R x 6 {src_off, n, dst_off, p, q, pos_off}
unsigned long long vvk_pcm_stretch_ws_bytes(int R);
int vvk_pcm_stretch(const int16_t* x, long long n_x, const long long* rows, int R, long long max_out, const double* window, int16_t* y,
                    long long n_y, int* pos, long long n_pos, void* ws, hipStream_t st, const char** err);
// N18 formant-preserving pitch shift (vv_formant.hip): per-frame LPC analysis of y and x, the filter A_y / A_x cut at L taps, the blended FIR;
// rows R x 7 {x_off, n, y_off, n_f, z_off, tn, td}
unsigned long long vvk_pcm_formant_ws_bytes(long long total_frames, int R);
int vvk_pcm_formant(const int16_t* x, long long n_x, const int16_t* y, long long n_y, const long long* rows, int R, long long total_frames,
                    long long max_frames, const double* wa, const double* g, const double* window, int16_t* z, long long n_z, double* h_out,
                    void* ws, hipStream_t st, const char** err);
// N19 vocoder-bias denoiser (vv_denoise.hip): per output hop the four frames above it, forward transform, mag - s bias clamped at zero, inverse,
// overlap-add; rows R x 4 {x_off, n, y_off, bias_row}.  total_frames = the sum of M + 3, max_hops = the largest max(M, 1)
unsigned long long vvk_pcm_denoise_ws_bytes(int R);
int vvk_pcm_denoise(const int16_t* x, long long n_x, const long long* rows, int R, long long total_frames, long long max_hops, const double* strengths,
                    const double* bias, long long n_bias, const double* window, const double* twiddles, int16_t* y, long long n_y, double* mag_out,
                    void* ws, hipStream_t st, const char** err);
// the bias of R signals: the mean magnitude of bins 0 ... 512 over the full frames; total_frames / max_frames count those
unsigned long long vvk_pcm_denoise_bias_ws_bytes(long long total_frames, int R);
int vvk_pcm_denoise_bias(const int16_t* x, long long n_x, const long long* rows, int R, long long total_frames, long long max_frames,
                         const double* window, const double* twiddles, double* out, void* ws, hipStream_t st, const char** err);
// N22 keyed audio watermark (vv_watermark.hip): the denoiser's loop with a keyed gain of gp or gm per band cell; rows R x 4 {x_off, n, y_off,
// message}; chips int8 [64][320].  total_frames = the sum of M + 3, max_hops = the largest max(M, 1)
unsigned long long vvk_pcm_watermark_ws_bytes(int R);
int vvk_pcm_watermark(const int16_t* x, long long n_x, const long long* rows, int R, long long total_frames, long long max_hops, const int8_t* chips,
                      double gp, double gm, const double* window, const double* twiddles, int16_t* y, long long n_y, void* ws, hipStream_t st,
                      const char** err);
// the detector: band magnitudes per frame, one int32 contrast per cell, {num, den} per alignment and bit -> stats [R][256][24][2]; rows R x 4
// {x_off, n, 0, 0}; max_frames = the largest M + 3; cells_out NULL or int32 [total_frames][320]
unsigned long long vvk_pcm_watermark_detect_ws_bytes(long long total_frames, int R);
int vvk_pcm_watermark_detect(const int16_t* x, long long n_x, const long long* rows, int R, long long total_frames, long long max_frames,
                             const int8_t* chips, const double* window, const double* twiddles, long long* stats, int* cells_out, void* ws,
                             hipStream_t st, const char** err);
// N15 FLAC output (vv_flac.hip): per frame of 4096 samples the exhaustive fixed-predictor / Rice search, the frames' offsets, the bit packing;
// rows R x 4 {src_off, n, frame0, last}
unsigned long long vvk_flac_frame_bound(long long m);
// lpc_order 0 = N15; 1 ... 12 = N16: LPC subframes among the candidates, with vvk_pcm_flac_lpc_ws_bytes of scratch
unsigned long long vvk_pcm_flac_ws_bytes(long long total_frames, int R);
unsigned long long vvk_pcm_flac_lpc_ws_bytes(long long total_frames, int R);
int vvk_pcm_flac(const int16_t* x, long long n_x, const long long* rows, int R, int rate, int lpc_order, long long total_frames, long long max_frames,
                 uint8_t* y, long long n_y, long long* info, void* ws, hipStream_t st, const char** err);
// N17 FLAC input (vv_flac_decode.hip): candidate scan, per-candidate measure, per-clip chain; then restore, verdict, interleave.
// rows R x 8 {byte offset, n_bytes, channels, bits, min block, max block, rate, total}; lay R x 6 {pcm byte offset, frames, samples, frames in
// front, plane samples in front, samples in front}
unsigned long long vvk_flac_decode_frame_bound(int block, int channels, int bits);
unsigned long long vvk_flac_index_ws_bytes(long long n_bytes, int R);
unsigned long long vvk_flac_decode_ws_bytes(long long n_plane, long long total_frames);
int vvk_flac_index(const uint8_t* data, long long n_bytes, const long long* rows, int R, long long* info, void* ws, hipStream_t st, const char** err);
int vvk_flac_decode(const uint8_t* data, long long n_bytes, const long long* rows, int R, const long long* lay, long long total_frames,
                    long long total_samples, long long n_plane, int max_channels, void* ws, uint8_t* pcm, long long n_pcm, long long* info2, void* ws2,
                    hipStream_t st, const char** err);
// N25 IMA ADPCM output and ADPCM / G.711 input (vv_adpcm.hip).  Encoder rows R x 3 {src_off, n, dst_off in bytes}, max_blocks = the largest
// ceil(n / spb).  Decoder rows R x 8 {data byte offset, n_bytes, tag, channels, block align, frames, pcm byte offset, 0}; max_heads = the
// largest blocks x channels of an ADPCM clip, max_codes = the largest frames x channels of a G.711 clip (0 = none of that kind)
int vvk_pcm_adpcm(const int16_t* x, long long n_x, const long long* rows, int R, int spb, long long max_blocks, uint8_t* y, long long n_y,
                  hipStream_t st, const char** err);
int vvk_wav_decode(const uint8_t* data, long long n_data, const long long* rows, int R, long long max_heads, long long max_codes, uint8_t* pcm,
                   long long n_pcm, long long* status, hipStream_t st, const char** err);
// N6 Vocos decoder (vv_vocos.hip): generated-frame counts, the embed conv's im2col operand, the ISTFT spectrum and overlap-add
int vvk_vocos_lens(const int* seq_len, const int* ref_len, int* lens, int B, int N, int T_max, hipStream_t st, const char** err);
int vvk_vocos_im2col(const float* x, int B, int N, int M, const int* ref_len, const int* seq_len, int T_max, int k, float* out, int ld_out,
                     hipStream_t st, const char** err);
int vvk_vocos_spectrum(const float* head, int ld_head, int R, int n_fft, float* out, hipStream_t st, const char** err);
int vvk_vocos_ola(const float* frames, int ld_f, int B, int T_max, const int* lens, const float* window, int n_fft, int hop, int16_t* pcm,
                  int ld_pcm, int32_t* pcm_len, float* wave, int ld_wave, hipStream_t st, const char** err);
