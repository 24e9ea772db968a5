// N22: the keyed audio watermark -- a multiplicative spread-spectrum mark on the denoiser's frames (N = 1024, H = 256, Hann), and
// its detector.  The arithmetic is the specification: core/audio_processor.py (watermark_embed, watermark_cells, watermark_stats) computes
// the same operations in the same order, so the two agree bit for bit; behind the cell value everything is an integer, so the order of the
// sums is free.  With M = ceil(n / H), frames f = 0 ... F - 1 = M + 2, frame f starting at sample (f - 3) H, x = 0 outside the signal; the
// band is bins LO ... LO + K - 1; at alignment q the cell (f, k) lies in group g = ((f + q) / G) % P, carries bit j = (k - LO + 7 g) % NB of
// the message and the chip table[g][k - LO] (+-1, from the key, made on the host: nothing is hashed here):
//     embed  : the denoiser's loop (one workgroup of 256 threads per output hop over its four frames, no intermediate in HBM, no atomics) with
//              the gain (chip > 0) == (bit_j set) ? gp : gm on the band bins k and their mirrors N - k at q = 0, and 1.0 on every other bin.
//     detect : (1) one workgroup per frame: forward transform, the K band magnitudes to the workspace;  (2) one thread per cell:
//              r = 0.5 (m[max(f - G, 0)] + m[min(f + G, F - 1)]), d = (int)rint(32768 (m - r) / (m + r + 1.0));  (3) one workgroup per
//              (alignment, request): num[j] = sum chip d, den[j] = sum d d.  Thread t < 240 owns bit j = t % 24 and the frames f = t / 24 +
//              10 i: in a frame of group g its bins are k - LO = (j + 17 g) % 24 + 24 i (17 = -7 mod 24), so it sums into two registers
//              and nothing is indexed at run time; then one 64-bit integer LDS add per thread and value.
#pragma clang fp contract(off)
#ifndef VV_WATERMARK_HOST_CHECK       // tools/watermark_host_check.cpp compiles the kernels below for the host, on tools/hip_host_shim.h
#include "vv_common.h"
#include "vv_kernels.h"
#endif
#include "vv_denoise_fft.h"      // two_stages, transform, load_frame (shared with vv_denoise.hip)

namespace {

constexpr int WLO = 22;                       // VV_WATERMARK_LO
constexpr int WK = 320;                       // VV_WATERMARK_K
constexpr int WG = 4;                         // VV_WATERMARK_G
constexpr int WP = 64;                        // VV_WATERMARK_P
constexpr int WNB = 24;                       // VV_WATERMARK_NB
constexpr int WQ = WP * WG;                   // alignments
constexpr long long MAX_N = 1ll << 30;
constexpr long long DETECT_MAX_N = 1ll << 24;
static_assert(WLO + WK <= DN / 2 && (7 * WNB) % WNB == 0 && (7 + 17) % WNB == 0 && WK <= 14 * WNB, "the index arithmetic below assumes these");

// plan R x 2 int64 {frames in front, hops of this request = max(M, 1), or -1: the row is not followed}; rows R x 4 {x_off, n, y_off, message}.
// The host has checked the rows; checked all the same
__global__ void watermark_plan_kernel(const long long* __restrict__ rows, int R, long long n_x, long long n_y, long long total_frames,
                                      long long* __restrict__ plan) {
    if (blockIdx.x || threadIdx.x) return;
    long long at = 0;
    for (int r = 0; r < R; ++r) {
        const long long* q = rows + 4 * (long long)r;
        const bool ok = q[0] >= 0 && q[1] >= 0 && q[1] <= MAX_N && q[1] <= n_x && q[0] <= n_x - q[1] && q[2] >= 0 && q[1] <= n_y &&
                        q[2] <= n_y - q[1] && q[3] >= 0 && q[3] < (1ll << WNB);
        const long long M = ok ? (q[1] + DH - 1) / DH : 0;
        const bool fit = ok && M + 3 <= total_frames - at;
        plan[2 * r] = at;
        plan[2 * r + 1] = fit ? (M > 0 ? M : 1) : -1;
        if (fit) at += M + 3;
    }
}

// plan R x 2 int64 {frames in front, frames F of this request = M + 3, or -1}; rows R x 4 {x_off, n, 0, 0}
__global__ void detect_plan_kernel(const long long* __restrict__ rows, int R, long long n_x, long long total_frames, long long* __restrict__ plan) {
    if (blockIdx.x || threadIdx.x) return;
    long long at = 0;
    for (int r = 0; r < R; ++r) {
        const long long* q = rows + 4 * (long long)r;
        const bool ok = q[0] >= 0 && q[1] >= 0 && q[1] <= DETECT_MAX_N && q[1] <= n_x && q[0] <= n_x - q[1];
        const long long F = ok ? (q[1] + DH - 1) / DH + 3 : 0;
        const bool fit = ok && F <= total_frames - at;
        plan[2 * r] = at;
        plan[2 * r + 1] = fit ? F : -1;
        if (fit) at += F;
    }
}

__global__ __launch_bounds__(256) void watermark_kernel(const int16_t* __restrict__ x, const long long* __restrict__ rows,
                                                        const long long* __restrict__ plan, const signed char* __restrict__ chips, double gp,
                                                        double gm, const double* __restrict__ window, const double* __restrict__ twiddles,
                                                        int16_t* __restrict__ y) {
    __shared__ double s_re[DLDS], s_im[DLDS], s_tw[DN];
    const long long req = blockIdx.y, i = blockIdx.x;
    const int t = threadIdx.x;
    const long long hops = plan[2 * req + 1];
    if (i >= hops) return;                                                         // uniform over the workgroup; -1 = the row is not followed
    const long long* r = rows + 4 * req;
    const long long n = r[1], M = (n + DH - 1) / DH;
    const unsigned msg = (unsigned)r[3];
    const int16_t* xr = x + r[0];
    for (int k = t; k < DN; k += 256) s_tw[k] = twiddles[k];
    double acc = 0.0;
    for (int q = 0; q < 4; ++q) {
        const long long f = i + q;
        if (f > M + 2) break;                                                      // uniform; only a request without samples has fewer than four
        load_frame(xr, n, (f - 3) * DH, window, s_re, s_im, t);
        __syncthreads();
        transform(s_re, s_im, s_tw, t, false);
        const int g = (int)((f / WG) % WP);
        const signed char* __restrict__ c = chips + g * WK;
        double vr[4], vi[4];
#pragma unroll
        for (int m = 0; m < 4; ++m) {
            const int k = rev10(t + 256 * m);
            const int kk = (k <= DN / 2 ? k : DN - k) - WLO;                       // bin N - k carries the gain of bin k
            const int kc = kk < 0 ? 0 : kk < WK ? kk : WK - 1, j = (kc + 7 * g) % WNB;   // the chip is read in any case: no branch round a load
            const double on = ((c[kc] > 0) == (((msg >> (WNB - 1 - j)) & 1u) != 0u)) ? gp : gm;
            const double gain = kk == kc ? on : 1.0;
            vr[m] = s_re[pad(k)] * gain;
            vi[m] = s_im[pad(k)] * gain;
        }
        __syncthreads();
#pragma unroll
        for (int m = 0; m < 4; ++m) {
            s_re[pad(t + 256 * m)] = vr[m];
            s_im[pad(t + 256 * m)] = vi[m];
        }
        __syncthreads();
        transform(s_re, s_im, s_tw, t, true);
        const int k = (3 - q) * DH + t;
        acc = acc + s_re[pad(k)] * window[k];
        __syncthreads();                                                           // the next frame overwrites the planes
    }
    const long long at = i * DH + t;
    if (at < n) y[r[2] + at] = (int16_t)(int)fmin(fmax(rint(acc / 1536.0), -32768.0), 32767.0);
}

// (1) the band magnitudes of every frame: mags [frames][K]
__global__ __launch_bounds__(256) void detect_frames_kernel(const int16_t* __restrict__ x, const long long* __restrict__ rows,
                                                            const long long* __restrict__ plan, const double* __restrict__ window,
                                                            const double* __restrict__ twiddles, double* __restrict__ mags) {
    __shared__ double s_re[DLDS], s_im[DLDS], s_tw[DN];
    const long long req = blockIdx.y, f = blockIdx.x;
    const int t = threadIdx.x;
    if (f >= plan[2 * req + 1]) return;                                            // uniform over the workgroup
    const long long* r = rows + 4 * req;
    for (int k = t; k < DN; k += 256) s_tw[k] = twiddles[k];
    load_frame(x + r[0], r[1], (f - 3) * DH, window, s_re, s_im, t);
    __syncthreads();
    transform(s_re, s_im, s_tw, t, false);
    double* out = mags + (plan[2 * req] + f) * WK;
    for (int kk = t; kk < WK; kk += 256) {
        const double re = s_re[pad(WLO + kk)], im = s_im[pad(WLO + kk)];
        out[kk] = sqrt(re * re + im * im);
    }
}

// (2) the cell values: cells [frames][K]
__global__ __launch_bounds__(256) void detect_cells_kernel(const long long* __restrict__ plan, const double* __restrict__ mags, int* __restrict__ cells) {
    const long long req = blockIdx.y, e = (long long)blockIdx.x * 256 + threadIdx.x, F = plan[2 * req + 1];
    if (e >= F * WK) return;                                                       // -1 = the row is not followed
    const long long f = e / WK, lo = f - WG > 0 ? f - WG : 0, hi = f + WG < F - 1 ? f + WG : F - 1;
    const int kk = (int)(e % WK);
    const double* m0 = mags + plan[2 * req] * WK + kk;
    const double m = m0[f * WK];
    const double r = 0.5 * (m0[lo * WK] + m0[hi * WK]);
    cells[plan[2 * req] * WK + e] = (int)rint(32768.0 * (m - r) / (m + r + 1.0));
}

// (3) the statistic of one alignment of one request: stats [R][256][24][2]
__global__ __launch_bounds__(256) void detect_stats_kernel(const long long* __restrict__ plan, const int* __restrict__ cells,
                                                           const signed char* __restrict__ chips, long long* __restrict__ stats) {
    __shared__ __attribute__((aligned(16))) signed char s_chip[WP * WK];
    __shared__ unsigned long long s_sum[2 * WNB];
    const int q = blockIdx.x, t = threadIdx.x;
    const long long req = blockIdx.y, F = plan[2 * req + 1];
    if (F < 0) return;                                                             // uniform; the row is not followed: its stats stay as they were
    for (int e = t; e < WP * WK / 4; e += 256) ((int*)s_chip)[e] = ((const int*)chips)[e];
    if (t < 2 * WNB) s_sum[t] = 0ull;
    __syncthreads();
    if (t < 10 * WNB) {
        const int j = t % WNB;
        const int* __restrict__ d0 = cells + plan[2 * req] * WK;
        long long num = 0, den = 0;
        for (long long f = t / WNB; f < F; f += 10) {
            const int g = (int)(((f + q) / WG) % WP);
            const int c0 = (j + 17 * g) % WNB;
            const int* __restrict__ d = d0 + f * WK + c0;
            const signed char* __restrict__ c = s_chip + g * WK + c0;
            auto cell = [&](int i) {
                const long long v = d[WNB * i];
                num += c[WNB * i] > 0 ? v : -v;
                den += v * v;
            };
#pragma unroll
            for (int i = 0; i < WK / WNB; ++i) cell(i);                            // 13 rounds that every c0 has
            if (c0 < WK % WNB) cell(WK / WNB);                                     // and the bins 312 ... 319
        }
        atomicAdd(&s_sum[2 * j], (unsigned long long)num);
        atomicAdd(&s_sum[2 * j + 1], (unsigned long long)den);
    }
    __syncthreads();
    if (t < 2 * WNB) stats[(req * WQ + q) * (2 * WNB) + t] = (long long)s_sum[t];
}

}  // namespace

// scratch: R x 2 int64 {frames in front, hops}
unsigned long long vvk_pcm_watermark_ws_bytes(int R) { return 16ull * (unsigned long long)(R > 0 ? R : 1); }

// scratch: R x 2 int64 {frames in front, frames}, then K magnitudes (float64) and K cell values (int32) per frame
unsigned long long vvk_pcm_watermark_detect_ws_bytes(long long total_frames, int R) {
    return 16ull * (unsigned long long)(R > 0 ? R : 1) + (unsigned long long)(total_frames > 0 ? total_frames : 1) * (12ull * WK);
}

#ifndef VV_WATERMARK_HOST_CHECK
int vvk_pcm_watermark(const int16_t* x, long long n_x, const long long* rows, int R, long long total_frames, long long max_hops, const int8_t* chips,
                      double gp, double gm, const double* window, const double* twiddles, int16_t* y, long long n_y, void* ws, hipStream_t st,
                      const char** err) {
    if (R < 1 || R > 65535 || n_x < 0 || n_y < 0 || total_frames < 3 || max_hops < 1 || max_hops > total_frames) {
        *err = "pcm_watermark: bad sizes (1 <= R <= 65535)";
        return -22;
    }
    if (!x || !rows || !chips || !window || !twiddles || !y || !ws) { *err = "pcm_watermark: null pointer"; return -22; }
    if (!(gp >= 1.0 && gp <= 1.5 && gm >= 0.5 && gm <= 1.0)) { *err = "pcm_watermark: gains outside 1 +- 0.5"; return -22; }
    long long* plan = (long long*)ws;
    watermark_plan_kernel<<<1, 64, 0, st>>>(rows, R, n_x, n_y, total_frames, plan);
    watermark_kernel<<<dim3((unsigned)max_hops, R), 256, 0, st>>>(x, rows, plan, (const signed char*)chips, gp, gm, window, twiddles, y);
    hipError_t he = hipGetLastError();
    if (he != hipSuccess) { *err = hipGetErrorString(he); return -5; }
    return 0;
}

int vvk_pcm_watermark_detect(const int16_t* x, long long n_x, const long long* rows, int R, long long total_frames, long long max_frames,
                             const int8_t* chips, const double* window, const double* twiddles, long long* stats, int* cells_out, void* ws,
                             hipStream_t st, const char** err) {
    if (R < 1 || R > 65535 || n_x < 0 || total_frames < 3 || max_frames < 3 || max_frames > total_frames) {
        *err = "pcm_watermark_detect: bad sizes (1 <= R <= 65535)";
        return -22;
    }
    if (!x || !rows || !chips || !window || !twiddles || !stats || !ws) { *err = "pcm_watermark_detect: null pointer"; return -22; }
    long long* plan = (long long*)ws;
    double* mags = (double*)(plan + 2 * (long long)R);
    int* cells = cells_out ? cells_out : (int*)(mags + total_frames * WK);
    detect_plan_kernel<<<1, 64, 0, st>>>(rows, R, n_x, total_frames, plan);
    detect_frames_kernel<<<dim3((unsigned)max_frames, R), 256, 0, st>>>(x, rows, plan, window, twiddles, mags);
    detect_cells_kernel<<<dim3((unsigned)((max_frames * WK + 255) / 256), R), 256, 0, st>>>(plan, mags, cells);
    detect_stats_kernel<<<dim3(WQ, R), 256, 0, st>>>(plan, cells, (const signed char*)chips, stats);
    hipError_t he = hipGetLastError();
    if (he != hipSuccess) { *err = hipGetErrorString(he); return -5; }
    return 0;
}
#endif
