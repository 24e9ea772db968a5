// N19: the vocoder-bias denoiser -- spectral subtraction against a stationary profile, first in the output chain.  Per request
// the STFT of the joined signal (N = 1024, H = 256, Hann), per bin mag - s bias clamped at zero with the phase kept, the inverse transform
// and the overlap-add.  The arithmetic is the specification: core/audio_processor.py (denoise_fft, denoise_pcm, denoise_bias) computes the
// same operations in the same order, so the two agree bit for bit.  With M = ceil(n / H), frames f = 0 ... M + 2, frame f starting at
// sample (f - 3) H, x = 0 outside the signal:
//     transform: radix-2 decimation in time behind a bit reversal, stages of half-length h = 1, 2, ... N / 2; per butterfly (a, b) with
//                (c, s) = twiddle[j N / (2 h)]:  tr = br c - bi s;  ti = br s + bi c;  a' = a + t;  b' = a - t.  The stages with c = 1,
//                s = 0 carry their products out like the others.  The inverse negates s and does not scale.
//     denoise  : one workgroup of 256 threads per output hop i.  It transforms frames i ... i + 3 one after another in LDS: load w[k] u[k]
//                bit-reversed, forward, per bin mag = sqrt(re re + im im), d = mag - s bias[k <= N / 2 ? k : N - k], g = d > 0 ? d / mag : 0,
//                re g and im g written bit-reversed, inverse; thread t adds re[(3 - q) H + t] w[..] of frame i + q to its accumulator,
//                from +0.0 with q ascending; z = clamp(rint(acc / 1536)).  A thread owns four points through two stages at a time, so a
//                transform is five passes over LDS; the operations a value sees are those of the ten stages.
//     bias     : one workgroup per full frame (start f H, f H + N <= n): forward, the 513 magnitudes to the workspace; then one thread per
//                (request, bin) sums them with f ascending from +0.0 and divides by the count.
// Four times the minimal number of transforms, and in exchange no intermediate in HBM, no atomics, no ordering between workgroups.  The
// tables w and twiddle are the host's (the device evaluates neither a cosine nor a sine).  LDS: element i of a frame lies at i + i / 4, so
// the four-point groups of the first passes (strides of 4 and 16 doubles) fall on distinct banks.
#pragma clang fp contract(off)
#ifndef VV_DENOISE_HOST_CHECK         // tools/denoise_host_check.cpp compiles the kernels below for the host, on tools/hip_host_shim.h
#include "vv_common.h"
#include "vv_kernels.h"
#endif
#include "vv_denoise_fft.h"      // two_stages, transform, load_frame (shared with vv_watermark.hip)

namespace {

constexpr int DB = DN / 2 + 1;                // entries of a bias row
constexpr long long MAX_N = 1ll << 30;
constexpr long long BIAS_MAX_N = 1ll << 20;

// a row {x_off, n, y_off, bias_row} that the denoise kernel may follow.  The host has checked it; checked all the same
__device__ __forceinline__ bool row_ok(const long long* __restrict__ r, double s, long long n_x, long long n_y, long long n_bias) {
    return r[0] >= 0 && r[1] >= 0 && r[1] <= MAX_N && r[1] <= n_x && r[0] <= n_x - r[1] && r[2] >= 0 && r[1] <= n_y && r[2] <= n_y - r[1] &&
           r[3] >= 0 && r[3] < n_bias && s >= 0.0 && s <= 16.0;
}

// plan R x 2 int64 {frames in front, hops of this request = max(M, 1), or -1: the row is not followed}
__global__ void denoise_plan_kernel(const long long* __restrict__ rows, const double* __restrict__ strengths, int R, long long n_x, long long n_y,
                                    long long n_bias, long long total_frames, long long* __restrict__ plan) {
    if (blockIdx.x || threadIdx.x) return;
    long long at = 0;
    for (int r = 0; r < R; ++r) {
        const long long* q = rows + 4 * (long long)r;
        const bool ok = row_ok(q, strengths[r], n_x, n_y, n_bias);
        const long long M = ok ? (q[1] + DH - 1) / DH : 0;
        const bool fit = ok && M + 3 <= total_frames - at;
        plan[2 * r] = at;
        plan[2 * r + 1] = fit ? (M > 0 ? M : 1) : -1;
        if (fit) at += M + 3;
    }
}

// plan R x 2 int64 {full frames in front, full frames of this request, or -1}
__global__ void denoise_bias_plan_kernel(const long long* __restrict__ rows, int R, long long n_x, long long total_frames, long long* __restrict__ plan) {
    if (blockIdx.x || threadIdx.x) return;
    long long at = 0;
    for (int r = 0; r < R; ++r) {
        const long long* q = rows + 4 * (long long)r;
        const bool ok = q[0] >= 0 && q[1] >= DN && q[1] <= BIAS_MAX_N && q[1] <= n_x && q[0] <= n_x - q[1];
        const long long F = ok ? (q[1] - DN) / DH + 1 : 0;
        const bool fit = ok && F <= total_frames - at;
        plan[2 * r] = at;
        plan[2 * r + 1] = fit ? F : -1;
        if (fit) at += F;
    }
}

__global__ __launch_bounds__(256) void denoise_kernel(const int16_t* __restrict__ x, const long long* __restrict__ rows,
                                                      const long long* __restrict__ plan, const double* __restrict__ strengths,
                                                      const double* __restrict__ bias, const double* __restrict__ window,
                                                      const double* __restrict__ twiddles, int16_t* __restrict__ y, double* __restrict__ mag_out) {
    __shared__ double s_re[DLDS], s_im[DLDS], s_tw[DN];
    const long long req = blockIdx.y, i = blockIdx.x;
    const int t = threadIdx.x;
    const long long hops = plan[2 * req + 1];
    if (i >= hops) return;                                                         // uniform over the workgroup; -1 = the row is not followed
    const long long* r = rows + 4 * req;
    const long long n = r[1], M = (n + DH - 1) / DH;
    const int16_t* xr = x + r[0];
    const double s = strengths[req];
    const double* __restrict__ b = bias + r[3] * DB;
    for (int k = t; k < DN; k += 256) s_tw[k] = twiddles[k];
    double acc = 0.0;
    for (int q = 0; q < 4; ++q) {
        const long long f = i + q;
        if (f > M + 2) break;                                                      // uniform; only a request without samples has fewer than four
        load_frame(xr, n, (f - 3) * DH, window, s_re, s_im, t);
        __syncthreads();
        transform(s_re, s_im, s_tw, t, false);
        const bool record = mag_out && (q == 0 || i == hops - 1);                  // every frame once: by its own hop, the last three by the last hop
        double vr[4], vi[4];
#pragma unroll
        for (int m = 0; m < 4; ++m) {
            const int k = rev10(t + 256 * m);
            const double re = s_re[pad(k)], im = s_im[pad(k)];
            const double mag = sqrt(re * re + im * im);
            const double d = mag - s * b[k <= DN / 2 ? k : DN - k];
            const double g = d > 0.0 ? d / mag : 0.0;
            vr[m] = re * g;
            vi[m] = im * g;
            if (record) mag_out[(plan[2 * req] + f) * DN + k] = mag;
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

__global__ __launch_bounds__(256) void denoise_bias_frames_kernel(const int16_t* __restrict__ x, const long long* __restrict__ rows,
                                                                  const long long* __restrict__ plan, const double* __restrict__ window,
                                                                  const double* __restrict__ twiddles, double* __restrict__ mags) {
    __shared__ double s_re[DLDS], s_im[DLDS], s_tw[DN];
    const long long req = blockIdx.y, f = blockIdx.x;
    const int t = threadIdx.x;
    if (f >= plan[2 * req + 1]) return;                                            // uniform over the workgroup
    const long long* r = rows + 4 * req;
    for (int k = t; k < DN; k += 256) s_tw[k] = twiddles[k];
    load_frame(x + r[0], r[1], f * DH, window, s_re, s_im, t);
    __syncthreads();
    transform(s_re, s_im, s_tw, t, false);
    double* out = mags + (plan[2 * req] + f) * DB;
    for (int k = t; k < DB; k += 256) {
        const double re = s_re[pad(k)], im = s_im[pad(k)];
        out[k] = sqrt(re * re + im * im);
    }
}

__global__ __launch_bounds__(256) void denoise_bias_mean_kernel(const long long* __restrict__ plan, const double* __restrict__ mags, int R,
                                                                double* __restrict__ out) {
    const long long e = (long long)blockIdx.x * 256 + threadIdx.x;
    if (e >= (long long)R * DB) return;
    const long long req = e / DB, k = e % DB, F = plan[2 * req + 1];
    if (F < 1) return;
    const double* m = mags + plan[2 * req] * DB + k;
    double acc = 0.0;
    for (long long f = 0; f < F; ++f) acc = acc + m[f * DB];
    out[e] = acc / (double)F;
}

}  // namespace

// scratch: R x 2 int64 {frames in front, hops}
unsigned long long vvk_pcm_denoise_ws_bytes(int R) { return 16ull * (unsigned long long)(R > 0 ? R : 1); }

// scratch: R x 2 int64 {full frames in front, full frames}, then 513 magnitudes per full frame
unsigned long long vvk_pcm_denoise_bias_ws_bytes(long long total_frames, int R) {
    return 16ull * (unsigned long long)(R > 0 ? R : 1) + (unsigned long long)(total_frames > 0 ? total_frames : 1) * (8ull * DB);
}

#ifndef VV_DENOISE_HOST_CHECK
int vvk_pcm_denoise(const int16_t* x, long long n_x, const long long* rows, int R, long long total_frames, long long max_hops, const double* strengths,
                    const double* bias, long long n_bias, const double* window, const double* twiddles, int16_t* y, long long n_y, double* mag_out,
                    void* ws, hipStream_t st, const char** err) {
    if (R < 1 || R > 65535 || n_x < 0 || n_y < 0 || n_bias < 1 || total_frames < 3 || max_hops < 1 || max_hops > total_frames) {
        *err = "pcm_denoise: bad sizes (1 <= R <= 65535)";
        return -22;
    }
    if (!x || !rows || !strengths || !bias || !window || !twiddles || !y || !ws) { *err = "pcm_denoise: null pointer"; return -22; }
    long long* plan = (long long*)ws;
    denoise_plan_kernel<<<1, 64, 0, st>>>(rows, strengths, R, n_x, n_y, n_bias, total_frames, plan);
    denoise_kernel<<<dim3((unsigned)max_hops, R), 256, 0, st>>>(x, rows, plan, strengths, bias, window, twiddles, y, mag_out);
    hipError_t he = hipGetLastError();
    if (he != hipSuccess) { *err = hipGetErrorString(he); return -5; }
    return 0;
}

int vvk_pcm_denoise_bias(const int16_t* x, long long n_x, const long long* rows, int R, long long total_frames, long long max_frames,
                         const double* window, const double* twiddles, double* out, void* ws, hipStream_t st, const char** err) {
    if (R < 1 || R > 65535 || n_x < 0 || total_frames < 1 || max_frames < 1 || max_frames > total_frames) {
        *err = "pcm_denoise_bias: bad sizes (1 <= R <= 65535)";
        return -22;
    }
    if (!x || !rows || !window || !twiddles || !out || !ws) { *err = "pcm_denoise_bias: null pointer"; return -22; }
    long long* plan = (long long*)ws;
    double* mags = (double*)(plan + 2 * (long long)R);
    denoise_bias_plan_kernel<<<1, 64, 0, st>>>(rows, R, n_x, total_frames, plan);
    denoise_bias_frames_kernel<<<dim3((unsigned)max_frames, R), 256, 0, st>>>(x, rows, plan, window, twiddles, mags);
    denoise_bias_mean_kernel<<<(unsigned)(((long long)R * DB + 255) / 256), 256, 0, st>>>(plan, mags, R, out);
    hipError_t he = hipGetLastError();
    if (he != hipSuccess) { *err = hipGetErrorString(he); return -5; }
    return 0;
}
#endif
