// N18: formant-preserving pitch shift -- the envelope correction behind the rate conversion that makes the pitch.  y is what
// the prosody step made of x; per hop of H samples an all-pole envelope of y and of x at the same moment, the filter A_y(z) / A_x(z) cut
// at L taps, and the two filters of a hop blended under the WSOLA window.
// The arithmetic is the specification: core/audio_processor.py (formant_filters, apply_formant_filters) computes the same operations in
// the same order, so the two agree bit for bit.  With P = 24, NA = 1024, H = 256, L = 2048, M = ceil(n_f / H), frames m = 0 ... M:
//     plan     : one thread walks the rows: frames in front of each request, -1 for a row that the kernels must not follow.
//     analysis : one workgroup per (frame, signal).  u[k] = s[c - NA / 2 + k] (zero outside the signal), c = m H for y and
//                floor(m H tn / td) for x; xw[k] = rint(wa[k] (u[k] - u[k - 1])) as an integer; R[l] = sum_k xw[k] xw[k - l], l <= P, an
//                exact integer below 2^44, so the split over the threads and the order are free.  Then ONE thread: Rf[0] += Rf[0] 2^-20
//                and the Levinson-Durbin recurrence of vv_flac.hip up to order P; R[0] = 0 or an err that is not > 0 makes the frame
//                flat.  It leaves A[0] = 1, A[k] = -(a[k] g[k]), err; a flat frame leaves the unit polynomial and err = 1.
//     filter   : one thread per frame.  r[t] = (t <= P ? A_y[t] : 0) - A_x[1] r[t - 1] - ... - A_x[min(t, P)] r[t - min(t, P)], k ascending;
//                h[t] = gain r[t], gain = sqrt(err_x / err_y); either side flat: the unit impulse.  The last 32 r of a thread live in
//                registers (the steps are unrolled by 32, so the window never moves); LDS only stages 32 steps of the wave's 64 frames
//                for one coalesced store.
//     apply    : one wave per hop, four output samples per lane.  The y tile with L samples of history lies in LDS as float64; the two
//                filters of the hop are read with wave-uniform loads.  v_a = sum_j h_{m-1}[j] y[i - j], v_b with h_m: from +0.0, j
//                ascending, every product rounded on its own; z[i] = clamp(rint(w[k + H] v_a + w[k] v_b)).
// No atomics, no readback; the tables wa, g and w are the host's (the device evaluates neither a cosine nor a power):
#pragma clang fp contract(off)
#ifndef VV_FORMANT_HOST_CHECK         // tools/formant_host_check.cpp compiles the kernels below for the host, on tools/hip_host_shim.h
#include "vv_common.h"
#include "vv_kernels.h"
#endif

namespace {

constexpr int FP = 24;                        // VV_FORMANT_P
constexpr int FNA = 1024;                     // VV_FORMANT_NA
constexpr int FH = 256;                       // VV_FORMANT_H
constexpr int FL = 2048;                      // VV_FORMANT_L
constexpr int COEF = 32;                      // doubles per (frame, signal): A[0 ... P], err, flat
constexpr int PARTS = 8;                      // the sum over k of one lag is split over PARTS threads
constexpr int FLUSH = 32;                     // steps of the filter pass per coalesced store, and the length of a thread's register window of r
constexpr long long MAX_PQ = 2048;
constexpr long long MAX_N = 1ll << 30;
static_assert(FL % FLUSH == 0 && (FLUSH & (FLUSH - 1)) == 0 && FP < FLUSH && (FP + 1) * PARTS <= 256 && FL % 4 == 0 && FH == 256, "the index arithmetic below assumes these");

__device__ __forceinline__ long long sample_at(const int16_t* __restrict__ s, long long n, long long i) { return i >= 0 && i < n ? (long long)s[i] : 0; }

// a row {x_off, n, y_off, n_f, z_off, tn, td} that the kernels may follow.  The host has checked it; checked all the same
__device__ __forceinline__ bool row_ok(const long long* __restrict__ r, long long n_x, long long n_y, long long n_z) {
    if (r[0] < 0 || r[1] < 0 || r[1] > MAX_N || r[1] > n_x || r[0] > n_x - r[1] || r[5] < 1 || r[5] > MAX_PQ || r[6] < 1 || r[6] > MAX_PQ) return false;
    const long long n_f = (r[1] * r[6] + r[5] - 1) / r[5];
    return r[3] == n_f && r[2] >= 0 && n_f <= n_y && r[2] <= n_y - n_f && r[4] >= 0 && n_f <= n_z && r[4] <= n_z - n_f;
}

// plan R x 2 int64 {frames in front, frames of this request = M + 1, or -1: the row is not followed}
__global__ void formant_plan_kernel(const long long* __restrict__ rows, int R, long long n_x, long long n_y, long long n_z, long long total_frames,
                                    long long* __restrict__ plan) {
    if (blockIdx.x || threadIdx.x) return;
    long long at = 0;
    for (int r = 0; r < R; ++r) {
        const long long* q = rows + 7 * (long long)r;
        const bool ok = row_ok(q, n_x, n_y, n_z);
        const long long frames = ok ? (q[3] + FH - 1) / FH + 1 : 0;
        const bool fit = ok && frames <= total_frames - at;
        plan[2 * r] = at;
        plan[2 * r + 1] = fit ? frames : -1;
        if (fit) at += frames;
    }
}

__global__ __launch_bounds__(256) void formant_analysis_kernel(const int16_t* __restrict__ x, const int16_t* __restrict__ y,
                                                               const long long* __restrict__ rows, const long long* __restrict__ plan,
                                                               const double* __restrict__ wa, const double* __restrict__ g,
                                                               double* __restrict__ coef) {
    __shared__ int s_xw[FNA];
    __shared__ long long s_part[(FP + 1) * PARTS];
    __shared__ double s_rf[FP + 1];
    __shared__ double s_a[2][FP + 1];
    const long long req = blockIdx.y, m = blockIdx.x;
    const int sig = blockIdx.z, tid = threadIdx.x;                                 // 0 = y, 1 = x
    const long long frames = plan[2 * req + 1];
    if (m >= frames) return;                                                       // uniform over the workgroup; -1 = the row is not followed
    const long long* r = rows + 7 * req;
    const int16_t* s = sig ? x + r[0] : y + r[2];
    const long long n = sig ? r[1] : r[3];
    const long long c = sig ? (m * FH * r[5]) / r[6] : m * FH;
    for (int k = tid; k < FNA; k += 256) {
        const long long i = c - FNA / 2 + k;
        const long long d = sample_at(s, n, i) - sample_at(s, n, i - 1);
        s_xw[k] = (int)rint(wa[k] * (double)d);                                    // |xw| < 2^17
    }
    __syncthreads();
    if (tid < (FP + 1) * PARTS) {
        const int lag = tid / PARTS;
        long long acc = 0;
        for (int k = lag + tid % PARTS; k < FNA; k += PARTS) acc += (long long)s_xw[k] * (long long)s_xw[k - lag];
        s_part[tid] = acc;
    }
    __syncthreads();
    if (tid) return;
    double* out = coef + ((plan[2 * req] + m) * 2 + sig) * COEF;
    bool flat = false;
    for (int l = 0; l <= FP; ++l) {
        long long v = 0;
        for (int p = 0; p < PARTS; ++p) v += s_part[l * PARTS + p];
        if (l == 0 && v == 0) flat = true;
        s_rf[l] = (double)v;
    }
    double err = 1.0;
    int cur = 0;
    if (!flat) {
        s_rf[0] = s_rf[0] + s_rf[0] * 9.5367431640625e-07;                         // 2^-20
        err = s_rf[0];
        for (int p = 1; p <= FP; ++p) {
            double acc = s_rf[p];
            for (int j = 1; j < p; ++j) acc = acc - s_a[cur][j] * s_rf[p - j];
            const double k = acc / err;
            for (int j = 1; j < p; ++j) s_a[cur ^ 1][j] = s_a[cur][j] - k * s_a[cur][p - j];
            s_a[cur ^ 1][p] = k;
            cur ^= 1;
            err = err * (1.0 - k * k);
            if (!(err > 0.0)) { flat = true; break; }
        }
    }
    out[0] = 1.0;
    for (int k = 1; k <= FP; ++k) out[k] = flat ? 0.0 : -(s_a[cur][k] * g[k]);
    out[FP + 1] = flat ? 1.0 : err;
    out[FP + 2] = flat ? 1.0 : 0.0;
}

// FLUSH steps of the recursion for one frame: r[t - k] is hist[(t - k) % FLUSH], in registers (every index below is a constant once the
// loops are unrolled); FIRST: steps 0 ... FLUSH - 1, where the sum stops at k = t and A_y comes in
template <bool FIRST>
__device__ __forceinline__ void filter_steps(const double (&Ay)[FP + 1], const double (&Ax)[FP + 1], double (&hist)[FLUSH], double (*s_r)[65], int lane) {
#pragma unroll
    for (int u = 0; u < FLUSH; ++u) {
        double acc = FIRST && u <= FP ? Ay[u] : 0.0;
#pragma unroll
        for (int k = 1; k <= FP; ++k)
            if (!FIRST || k <= u) acc = acc - Ax[k] * hist[(u - k) & (FLUSH - 1)];
        hist[u] = acc;
        s_r[u][lane] = acc;
    }
}

__global__ __launch_bounds__(64) void formant_filter_kernel(const long long* __restrict__ plan, const double* __restrict__ coef,
                                                            double* __restrict__ taps) {
    __shared__ double s_r[FLUSH][65];                                              // [step][lane]: the staging of one coalesced store
    __shared__ double s_gain[64];
    const long long req = blockIdx.y, m0 = (long long)blockIdx.x * 64;
    const int lane = threadIdx.x;
    const long long frames = plan[2 * req + 1], f0 = plan[2 * req];
    if (m0 >= frames) return;                                                      // uniform over the wave
    const bool live = m0 + lane < frames;
    double Ay[FP + 1], Ax[FP + 1], hist[FLUSH], gain = 1.0;
    const double* cy = coef + ((f0 + m0 + (live ? lane : 0)) * 2) * COEF;
    const bool unit = !live || cy[FP + 2] != 0.0 || cy[COEF + FP + 2] != 0.0;      // either analysis flat: the unit impulse
#pragma unroll
    for (int k = 0; k <= FP; ++k) {
        Ay[k] = unit ? (k ? 0.0 : 1.0) : cy[k];
        Ax[k] = unit ? (k ? 0.0 : 1.0) : cy[COEF + k];
    }
    if (!unit) gain = sqrt(cy[COEF + FP + 1] / cy[FP + 1]);
    s_gain[lane] = gain;                                                           // read by other lanes behind the first barrier below
    for (int t0 = 0; t0 < FL; t0 += FLUSH) {
        if (t0 == 0) filter_steps<true>(Ay, Ax, hist, s_r, lane);
        else filter_steps<false>(Ay, Ax, hist, s_r, lane);
        __syncthreads();                                                           // steps t0 ... t0 + FLUSH - 1 are complete: 64 frames x FLUSH taps go out
        for (int e = lane; e < 64 * FLUSH; e += 64) {
            const int f = e / FLUSH, tt = e % FLUSH;
            if (m0 + f < frames) taps[(f0 + m0 + f) * FL + t0 + tt] = s_gain[f] * s_r[tt][f];
        }
        __syncthreads();
    }
}

__global__ __launch_bounds__(64) void formant_apply_kernel(const int16_t* __restrict__ y, const long long* __restrict__ rows,
                                                           const long long* __restrict__ plan, const double* __restrict__ taps,
                                                           const double* __restrict__ window, int16_t* __restrict__ z) {
    __shared__ __attribute__((aligned(32))) double s_y[FL + FH];                   // s_y[k] = y[m1 H - L + k], zero outside the signal
    const long long req = blockIdx.y, m1 = blockIdx.x;                             // m1 = m - 1: the hop
    const int lane = threadIdx.x;
    const long long frames = plan[2 * req + 1];
    if (m1 + 1 >= frames) return;                                                  // uniform over the wave; a request of M hops has M + 1 frames
    const long long* r = rows + 7 * req;
    const long long n_f = r[3];
    const int16_t* yr = y + r[2];
    for (int k = lane; k < FL + FH; k += 64) s_y[k] = (double)sample_at(yr, n_f, m1 * FH - FL + k);
    __syncthreads();
    const double* __restrict__ ha = taps + (plan[2 * req] + m1) * FL;
    const double* __restrict__ hb = ha + FL;
    double va[4] = {0.0, 0.0, 0.0, 0.0}, vb[4] = {0.0, 0.0, 0.0, 0.0};
    double hi[4], lo[4];                                                           // hi = s_y[p ... p + 3], lo = s_y[p - 4 ... p - 1], p = L + 4 lane - j0
#pragma unroll
    for (int c = 0; c < 4; ++c) hi[c] = s_y[FL + 4 * lane + c];
#pragma unroll 2
    for (int j0 = 0; j0 < FL; j0 += 4) {
#pragma unroll
        for (int c = 0; c < 4; ++c) lo[c] = s_y[FL + 4 * lane - j0 - 4 + c];
#pragma unroll
        for (int jj = 0; jj < 4; ++jj) {
            const double a = ha[j0 + jj], b = hb[j0 + jj];
#pragma unroll
            for (int c = 0; c < 4; ++c) {                                          // output 4 lane + c reads y[i - j] = s_y[p + c - jj]
                const double v = c >= jj ? hi[c - jj] : lo[4 + c - jj];
                va[c] = va[c] + a * v;
                vb[c] = vb[c] + b * v;
            }
        }
#pragma unroll
        for (int c = 0; c < 4; ++c) hi[c] = lo[c];
    }
    int16_t* zr = z + r[4];
#pragma unroll
    for (int c = 0; c < 4; ++c) {
        const int k = 4 * lane + c;
        const long long i = m1 * FH + k;
        if (i < n_f) zr[i] = (int16_t)(int)fmin(fmax(rint(window[k + FH] * va[c] + window[k] * vb[c]), -32768.0), 32767.0);
    }
}

}  // namespace

// scratch: R x 2 int64 {frames in front, frames}, the (frame, signal) coefficient blocks, every frame's L taps
unsigned long long vvk_pcm_formant_ws_bytes(long long total_frames, int R) {
    const unsigned long long F = (unsigned long long)(total_frames > 0 ? total_frames : 1);
    return 16ull * (unsigned long long)(R > 0 ? R : 1) + F * (2ull * COEF * 8ull) + F * (8ull * FL);
}

#ifndef VV_FORMANT_HOST_CHECK
int vvk_pcm_formant(const int16_t* x, long long n_x, const int16_t* y, long long n_y, const long long* rows, int R, long long total_frames,
                    long long max_frames, const double* wa, const double* g, const double* window, int16_t* z, long long n_z, double* h_out,
                    void* ws, hipStream_t st, const char** err) {
    if (R < 1 || R > 65535 || n_x < 0 || n_y < 0 || n_z < 0 || total_frames < 1 || max_frames < 1 || max_frames > total_frames) {
        *err = "pcm_formant: bad sizes (1 <= R <= 65535)";
        return -22;
    }
    if (!x || !y || !rows || !wa || !g || !window || !z || !ws) { *err = "pcm_formant: null pointer"; return -22; }
    long long* plan = (long long*)ws;
    double* coef = (double*)(plan + 2 * (long long)R);
    double* taps = h_out ? h_out : coef + total_frames * 2 * COEF;
    formant_plan_kernel<<<1, 64, 0, st>>>(rows, R, n_x, n_y, n_z, total_frames, plan);
    formant_analysis_kernel<<<dim3((unsigned)max_frames, R, 2), 256, 0, st>>>(x, y, rows, plan, wa, g, coef);
    formant_filter_kernel<<<dim3((unsigned)((max_frames + 63) / 64), R), 64, 0, st>>>(plan, coef, taps);
    if (max_frames > 1) formant_apply_kernel<<<dim3((unsigned)(max_frames - 1), R), 64, 0, st>>>(y, rows, plan, taps, window, z);
    hipError_t he = hipGetLastError();
    if (he != hipSuccess) { *err = hipGetErrorString(he); return -5; }
    return 0;
}
#endif
