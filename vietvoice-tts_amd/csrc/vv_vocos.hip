// N6 Vocos decoder: the kernels around the ConvNeXt backbone.  The backbone itself runs on the shared kernels
// (vv_gemm fp32, vvk_dwconv, vvk_ln_mod); what is new is
//   * the embed conv's im2col operand, read straight from the generated-frame slice of the [B][N][n_mel] state,
//   * the ISTFT head's spectrum (exp, clip at 100, sincos) in the column order of const.istft_basis,
//   * the overlap-add of the windowed frames, divided by the window-square envelope, trimmed by n_fft / 2 (centre padding),
//     quantised to int16 like conv_post (without its tanh).
// Token-major padded planes: row b * T_max + t holds frame t of item b; rows t >= T_b are computed by the GEMMs and never read.
#include <hip/hip_runtime.h>
#include <cstdint>
#include "vv_kernels.h"

namespace {

inline int grid_1d(size_t total) { return (int)std::min<size_t>((total + 255) / 256, 256 * 32); }

// The generated frames of item b are rows [gen_start, gen_start + gen_frames) of its N rows: both ends of the slice are clamped into
// [0, min(seq_len, N)] (mel_slice_kernel's rule), so a negative or oversized device length never addresses a row outside the item.
__device__ __forceinline__ int gen_start(const int* seq_len, const int* ref_len, int b, int N) {
    return min(max(ref_len[b], 0), max(min(seq_len[b], N), 0));
}
__device__ __forceinline__ int gen_frames(const int* seq_len, const int* ref_len, int b, int N, int T_max) {
    return min(max(min(seq_len[b], N), 0) - gen_start(seq_len, ref_len, b, N), T_max);
}

__global__ void vocos_lens_kernel(const int* __restrict__ seq_len, const int* __restrict__ ref_len, int* __restrict__ lens, int B, int N,
                                  int T_max) {
    const int b = blockIdx.x * 64 + threadIdx.x;
    if (b < B) lens[b] = gen_frames(seq_len, ref_len, b, N, T_max);
}

// out[b * T_max + t][j * M + m] = x[b][gen_start(b) + t + j - k / 2][m] inside the item's generated frames [0, T_b), else 0;
// columns [k * M, ld_out) are zero (the GEMM's K padding).  Four columns per thread (M % 4 == 0: a float4 never straddles a tap).
__global__ __launch_bounds__(256) void vocos_im2col_kernel(const float* __restrict__ x, int N, int M, const int* __restrict__ ref_len,
                                                           const int* __restrict__ seq_len, int B, int T_max, int k,
                                                           float* __restrict__ out, int ld_out) {
    const int c4 = ld_out >> 2, KM = k * M, half = k / 2;
    const size_t total = (size_t)B * T_max * c4;
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (size_t)gridDim.x * 256) {
        const int col = (int)(i % c4) * 4;
        const size_t row = i / c4;
        const int t = (int)(row % T_max), b = (int)(row / T_max);
        float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
        if (col < KM) {
            const int tap = col / M, m = col - tap * M;
            const int tt = t + tap - half;
            if (tt >= 0 && tt < gen_frames(seq_len, ref_len, b, N, T_max))
                v = *(const float4*)(x + ((size_t)b * N + gen_start(seq_len, ref_len, b, N) + tt) * M + m);
        }
        *(float4*)(out + row * ld_out + col) = v;
    }
}

// head [R][ld_head] = (log-magnitudes 0..n/2 | phases 0..n/2) -> out [R][n]: column k <= n/2 = mag_k cos p_k, column n/2 + k
// (1 <= k < n/2) = mag_k sin p_k, mag_k = min(exp(o_k), 100).  Precise expf / sincosf: the phases are unbounded (no v_sin / __sinf).
__global__ __launch_bounds__(256) void vocos_spectrum_kernel(const float* __restrict__ head, int ld_head, int R, int n,
                                                             float* __restrict__ out) {
    const int h = n / 2, nb = h + 1;
    const size_t total = (size_t)R * nb;
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (size_t)gridDim.x * 256) {
        const int kk = (int)(i % nb);
        const size_t r = i / nb;
        const float* o = head + r * ld_head;
        const float mag = fminf(expf(o[kk]), 100.0f);
        float s, c;
        sincosf(o[nb + kk], &s, &c);
        out[r * n + kk] = mag * c;
        if (kk > 0 && kk < h) out[r * n + h + kk] = mag * s;
    }
}

// Sample j of item b = position i = j + n/2 of the centred signal: the sum of the windowed frames t (t hop <= i < t hop + n, t < T_b)
// over the sum of their window squares.  Samples j >= hop (T_b - 1) are written as zeros, up to L_out per row.
__global__ __launch_bounds__(256) void vocos_ola_kernel(const float* __restrict__ frames, int ld_f, int T_max, const int* __restrict__ lens,
                                                        const float* __restrict__ window, int n, int hop, int16_t* __restrict__ pcm,
                                                        int ld_pcm, int32_t* __restrict__ pcm_len, float* __restrict__ wave, int ld_wave,
                                                        int L_out) {
    const int b = blockIdx.y;
    const int j = blockIdx.x * 256 + threadIdx.x;
    const int T = min(max(lens[b], 0), T_max);
    const int plen = hop * max(T - 1, 0);
    if (pcm_len && j == 0) pcm_len[b] = plen;
    if (j >= L_out) return;
    float y = 0.f;
    if (j < plen) {
        const int i = j + n / 2;
        const int t_lo = i >= n ? (i - n) / hop + 1 : 0, t_hi = min(i / hop, T - 1);
        float acc = 0.f, env = 0.f;
        for (int t = t_lo; t <= t_hi; ++t) {
            const int o = i - t * hop;
            const float w = window[o];
            acc += frames[((size_t)b * T_max + t) * ld_f + o];
            env = fmaf(w, w, env);
        }
        y = acc / env;
    }
    pcm[(size_t)b * ld_pcm + j] = (int16_t)fminf(fmaxf(y * 32767.0f, -32768.0f), 32767.0f);     // truncation toward zero
    if (wave) wave[(size_t)b * ld_wave + j] = y;
}

}  // namespace

#define VOCOS_CHECK_LAUNCH()                                                   \
    do {                                                                       \
        hipError_t he__ = hipGetLastError();                                   \
        if (he__ != hipSuccess) { *err = hipGetErrorString(he__); return -5; } \
    } while (0)

int vvk_vocos_lens(const int* seq_len, const int* ref_len, int* lens, int B, int N, int T_max, hipStream_t st, const char** err) {
    if (B < 1 || N < 1 || T_max < 1 || !seq_len || !ref_len || !lens) { *err = "vocos_lens: bad arguments"; return -22; }
    vocos_lens_kernel<<<(B + 63) / 64, 64, 0, st>>>(seq_len, ref_len, lens, B, N, T_max);
    VOCOS_CHECK_LAUNCH();
    return 0;
}

int vvk_vocos_im2col(const float* x, int B, int N, int M, const int* ref_len, const int* seq_len, int T_max, int k, float* out, int ld_out,
                     hipStream_t st, const char** err) {
    if (B < 1 || N < 1 || T_max < 1 || M < 4 || M % 4 || k < 1 || k % 2 == 0 || ld_out < k * M || ld_out % 4 || !x || !out || !ref_len || !seq_len) {
        *err = "vocos_im2col: bad arguments (n_mel % 4 == 0, odd k, ld_out >= k * n_mel and % 4 == 0)"; return -22;
    }
    if (((uintptr_t)x | (uintptr_t)out) % 16) { *err = "vocos_im2col: operands must be 16-byte aligned"; return -22; }
    vocos_im2col_kernel<<<grid_1d((size_t)B * T_max * (ld_out / 4)), 256, 0, st>>>(x, N, M, ref_len, seq_len, B, T_max, k, out, ld_out);
    VOCOS_CHECK_LAUNCH();
    return 0;
}

int vvk_vocos_spectrum(const float* head, int ld_head, int R, int n_fft, float* out, hipStream_t st, const char** err) {
    if (R < 1 || n_fft < 4 || n_fft % 2 || ld_head < n_fft + 2 || !head || !out) { *err = "vocos_spectrum: bad arguments (ld_head >= n_fft + 2)"; return -22; }
    vocos_spectrum_kernel<<<grid_1d((size_t)R * (n_fft / 2 + 1)), 256, 0, st>>>(head, ld_head, R, n_fft, out);
    VOCOS_CHECK_LAUNCH();
    return 0;
}

int vvk_vocos_ola(const float* frames, int ld_f, int B, int T_max, const int* lens, const float* window, int n_fft, int hop, int16_t* pcm,
                  int ld_pcm, int32_t* pcm_len, float* wave, int ld_wave, hipStream_t st, const char** err) {
    const long long L_out = (long long)T_max * hop;
    if (B < 1 || T_max < 1 || hop < 1 || n_fft % hop || ld_f < n_fft || !frames || !lens || !window || !pcm || ld_pcm < L_out ||
        (wave && ld_wave < L_out) || L_out >= (1ll << 31)) {
        *err = "vocos_ola: bad arguments (n_fft % hop == 0, ld_f >= n_fft, ld_pcm / ld_wave >= T_max * hop)"; return -22;
    }
    dim3 grid((unsigned)((L_out + 255) / 256), B);
    vocos_ola_kernel<<<grid, 256, 0, st>>>(frames, ld_f, T_max, lens, window, n_fft, hop, pcm, ld_pcm, pcm_len, wave, ld_wave, (int)L_out);
    VOCOS_CHECK_LAUNCH();
    return 0;
}
