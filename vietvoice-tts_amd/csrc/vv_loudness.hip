// N12: loudness normalisation of the joined signal on the device -- ITU-R BS.1770-4 integrated loudness (K-weighting, 400 ms
// blocks with 75 % overlap, absolute and relative gate), a gain to a target level under a sample-peak ceiling, applied in HBM.
// The arithmetic is the specification: core/audio_processor.py (normalize_loudness) computes the same float64 operations in the same
// order, so the two agree bit for bit, and a request measures the same alone or among others.
//   The K-weighting is a linear recurrence; it is cut into independent runs of VV_LOUD_RUN = 128 samples counted from each 100 ms
//   sub-block's first sample (the last run of a sub-block holds the remainder):
//     pass A : one thread per run: the end state E_r of the run started from ZERO state; max |x| of the run (also over the unmeasured tail)
//     pass B : one workgroup per request, sequential over its runs: S' = M S + E_r with the host's 4x4 zero-input tables M_full / M_last
//              (the device never recomputes them); every run's true start state replaces E_r in place
//     pass C : one thread per run: the same steps from the true start state, p_r = sum of y2^2 in sample order
//     gate   : one workgroup per request: q_j = ascending sum of the sub-block's p_r, z_j, both gates, the two sequential means, the gain
//     apply  : y = clamp(rint(x * g)), four samples per thread on the 8-byte grid of the destination's address, a scalar head and tail
// No atomics, no reordered sums, no logarithm; every product and sum is rounded on its own:
#pragma clang fp contract(off)
#ifndef VV_LOUDNESS_HOST_CHECK        // tools/loudness_host_check.cpp compiles the kernels below for the host, with its own stand-ins
#include "vv_common.h"
#include "vv_kernels.h"
#endif

namespace {

constexpr int RUN = 128;                      // VV_LOUD_RUN
constexpr int RPB = 64;                       // runs (= threads) per workgroup of passes A and C: one wave
constexpr int LDS_STRIDE = RUN + 2;           // int16 per staged run: 65 dwords, so the 64 lanes read 64 different banks

// tables (float64): b1[3] a1[2] | b2[3] a2[2] | M_full[4][4] | M_last[4][4] | ABS
constexpr int T_M_FULL = 10, T_M_LAST = 26, T_ABS = 42;

struct RunPos {
    long long src;        // first sample of the run in x
    int len;              // 0: no such run
    int measured;         // inside a complete sub-block (else: the tail, peak only)
};

// rows R x 4 int64 {src_off, n, dst_off, run_off}; run_off ascending.  The request of global run g = the last row with run_off <= g.
__device__ __forceinline__ RunPos locate_run(const long long* __restrict__ rows, int R, long long sub, int rps, long long g, long long n_x) {
    int lo = 0, hi = R - 1;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (rows[4 * (long long)mid + 3] <= g) lo = mid; else hi = mid - 1;
    }
    const long long* r = rows + 4 * (long long)lo;
    const long long so = r[0], n = r[1], l = g - r[3];
    const long long J = n / sub, meas = J * rps;
    RunPos p{0, 0, 0};
    long long start;
    if (l < 0) return p;
    if (l < meas) {
        const long long j = l / rps;
        const int k = (int)(l - j * rps);
        start = j * sub + (long long)k * RUN;
        p.len = k == rps - 1 ? (int)(sub - (long long)k * RUN) : RUN;
        p.measured = 1;
    } else {
        start = J * sub + (l - meas) * RUN;
        const long long left = n - start;
        if (left <= 0) return p;                                                 // a row whose run count the host got wrong: nothing to do
        p.len = left < RUN ? (int)left : RUN;
    }
    p.src = so + start;
    if (p.src < 0 || p.src + p.len > n_x) { p.len = 0; p.measured = 0; }         // the rows were validated on the host; clamped all the same
    return p;
}

struct Coef { double b10, b11, b12, a10, a11, b20, b21, b22, a20, a21; };

__device__ __forceinline__ Coef load_coef(const double* __restrict__ t) {
    return Coef{t[0], t[1], t[2], t[3], t[4], t[5], t[6], t[7], t[8], t[9]};
}

// one sample, direct form II transposed, in the order of the specification; returns y2
__device__ __forceinline__ double kw_step(const Coef& c, double u, double& s0, double& s1, double& s2, double& s3) {
    const double y1 = c.b10 * u + s0;
    s0 = (c.b11 * u - c.a10 * y1) + s1;
    s1 = c.b12 * u - c.a11 * y1;
    const double y2 = c.b20 * y1 + s2;
    s2 = (c.b21 * y1 - c.a20 * y2) + s3;
    s3 = c.b22 * y1 - c.a21 * y2;
    return y2;
}

// PASS 0 = A (zero start state -> E, peak), 1 = C (true start state -> p)
template <int PASS>
__global__ __launch_bounds__(RPB) void loud_run_kernel(const int16_t* __restrict__ x, long long n_x, const long long* __restrict__ rows, int R,
                                                       long long sub, int rps, long long total_runs, const double* __restrict__ tables,
                                                       double* __restrict__ state, double* __restrict__ power, long long* __restrict__ peak) {
    __shared__ int16_t stage[RPB * LDS_STRIDE];
    __shared__ long long s_src[RPB];
    __shared__ int s_len[RPB];
    const int tid = threadIdx.x;
    const long long g = (long long)blockIdx.x * RPB + tid;
    RunPos p{0, 0, 0};
    if (g < total_runs) p = locate_run(rows, R, sub, rps, g, n_x);
    const bool work = PASS == 0 ? p.len > 0 : p.measured != 0;
    s_src[tid] = p.src;
    s_len[tid] = work ? p.len : 0;
    __syncthreads();
    for (int k = 0; k < RPB; ++k) {                                              // coalesced: the wave reads one run's samples side by side
        const int len = s_len[k];
        const long long src = s_src[k];
        for (int j = tid; j < len; j += RPB) stage[k * LDS_STRIDE + j] = x[src + j];
    }
    __syncthreads();
    if (!work) return;
    const int16_t* mine = stage + tid * LDS_STRIDE;
    if (PASS == 0) {
        int pk = 0;
        for (int j = 0; j < p.len; ++j) {
            const int v = mine[j];
            const int a = v < 0 ? -v : v;
            pk = a > pk ? a : pk;
        }
        peak[g] = pk;
        if (!p.measured) return;
    }
    const Coef c = load_coef(tables);
    double s0 = 0.0, s1 = 0.0, s2 = 0.0, s3 = 0.0, acc = 0.0;
    if (PASS == 1) { s0 = state[4 * g]; s1 = state[4 * g + 1]; s2 = state[4 * g + 2]; s3 = state[4 * g + 3]; }
    for (int j = 0; j < p.len; ++j) {
        const double u = (double)mine[j] / 32768.0;
        const double y2 = kw_step(c, u, s0, s1, s2, s3);
        if (PASS == 1) acc = acc + y2 * y2;
    }
    if (PASS == 0) { state[4 * g] = s0; state[4 * g + 1] = s1; state[4 * g + 2] = s2; state[4 * g + 3] = s3; }
    else power[g] = acc;
}

// pass B: the request's measured runs in ascending order, 64 at a time through LDS (coalesced in and out); lane 0 walks them
__global__ __launch_bounds__(64) void loud_scan_kernel(const long long* __restrict__ rows, long long sub, int rps, long long total_runs,
                                                       const double* __restrict__ tables, double* __restrict__ state) {
    __shared__ double buf[64 * 4];
    __shared__ double Mt[32];
    const long long* r = rows + 4 * (long long)blockIdx.x;
    const long long n = r[1], base = r[3];
    long long meas = (n / sub) * rps;
    const int tid = threadIdx.x;
    if (base < 0 || base > total_runs) return;
    if (meas > total_runs - base) meas = total_runs - base;
    if (tid < 32) Mt[tid] = tables[T_M_FULL + tid];
    double S0 = 0.0, S1 = 0.0, S2 = 0.0, S3 = 0.0;
    int k = 0;                                                                   // run index inside its sub-block (lane 0's own counter)
    for (long long c0 = 0; c0 < meas; c0 += 64) {
        const int cnt = meas - c0 < 64 ? (int)(meas - c0) : 64;
        __syncthreads();
        for (int i = tid; i < cnt * 4; i += 64) buf[i] = state[4 * (base + c0) + i];
        __syncthreads();
        if (tid == 0) {
            for (int l = 0; l < cnt; ++l) {
                const double* M = Mt + (k == rps - 1 ? 16 : 0);
                const double e0 = buf[4 * l], e1 = buf[4 * l + 1], e2 = buf[4 * l + 2], e3 = buf[4 * l + 3];
                buf[4 * l] = S0; buf[4 * l + 1] = S1; buf[4 * l + 2] = S2; buf[4 * l + 3] = S3;
                const double n0 = ((((M[0] * S0 + M[1] * S1) + M[2] * S2) + M[3] * S3) + e0);
                const double n1 = ((((M[4] * S0 + M[5] * S1) + M[6] * S2) + M[7] * S3) + e1);
                const double n2 = ((((M[8] * S0 + M[9] * S1) + M[10] * S2) + M[11] * S3) + e2);
                const double n3 = ((((M[12] * S0 + M[13] * S1) + M[14] * S2) + M[15] * S3) + e3);
                S0 = n0; S1 = n1; S2 = n2; S3 = n3;
                k = k == rps - 1 ? 0 : k + 1;
            }
        }
        __syncthreads();
        for (int i = tid; i < cnt * 4; i += 64) state[4 * (base + c0) + i] = buf[i];
    }
}

// gate and gain: one workgroup per request.  q_j and z_j go to scratch (z_j into the request's own state slots, which pass C has read),
// the sequential means are lane 0's.  stats[r] = {zbar, kept, P, g}
__global__ __launch_bounds__(256) void loud_gate_kernel(const long long* __restrict__ rows, long long sub, int rps, long long total_runs,
                                                        const double* __restrict__ tables, const double* __restrict__ params,
                                                        const double* __restrict__ power, const long long* __restrict__ peak,
                                                        double* __restrict__ qbuf, double* __restrict__ zbuf, double* __restrict__ stats) {
    __shared__ long long red[256];
    const long long* r = rows + 4 * (long long)blockIdx.x;
    const long long n = r[1], base = r[3];
    const int tid = threadIdx.x;
    long long J = n / sub;
    long long runs = J * rps + ((n - J * sub) + RUN - 1) / RUN;
    if (base < 0 || base > total_runs) { J = 0; runs = 0; }
    else if (runs > total_runs - base) { runs = total_runs - base; if (J * rps > runs) J = runs / rps; }
    long long pk = 0;
    for (long long i = tid; i < runs; i += 256) { const long long v = peak[base + i]; pk = v > pk ? v : pk; }
    red[tid] = pk;
    for (long long j = tid; j < J; j += 256) {
        double q = 0.0;
        for (int k = 0; k < rps; ++k) q = q + power[base + j * rps + k];
        qbuf[base + j] = q;
    }
    __syncthreads();
    for (int s = 128; s > 0; s >>= 1) {                                          // an integer maximum: exact in any order
        if (tid < s) red[tid] = red[tid + s] > red[tid] ? red[tid + s] : red[tid];
        __syncthreads();
    }
    const long long nz = J >= 4 ? J - 3 : 0;
    const double den = (double)(4 * sub);
    for (long long j = tid; j < nz; j += 256)
        zbuf[4 * base + j] = (((qbuf[base + j] + qbuf[base + j + 1]) + qbuf[base + j + 2]) + qbuf[base + j + 3]) / den;
    __syncthreads();
    if (tid != 0) return;
    const double ABS = tables[T_ABS];
    const double* z = zbuf + 4 * base;
    double sum = 0.0, zbar = 0.0;
    long long cnt = 0, kept = 0;
    for (long long j = 0; j < nz; ++j) {
        const double v = z[j];
        if (v > ABS) { sum = sum + v; ++cnt; }
    }
    if (cnt > 0) {
        const double gamma = 0.1 * (sum / (double)cnt);
        sum = 0.0;
        for (long long j = 0; j < nz; ++j) {
            const double v = z[j];
            if (v > ABS && v > gamma) { sum = sum + v; ++kept; }
        }
        if (kept > 0) zbar = sum / (double)kept;
    }
    const double P = (double)red[0];
    const double T = params[2 * (long long)blockIdx.x], c = params[2 * (long long)blockIdx.x + 1];
    double g = 1.0;
    if (kept > 0 && T > 0.0 && P > 0.0) {
        g = sqrt(T / zbar);
        if (P * g > c) g = c / P;
    }
    double* st = stats + 4 * (long long)blockIdx.x;
    st[0] = zbar; st[1] = (double)kept; st[2] = P; st[3] = g;
}

__device__ __forceinline__ int scaled(int v, double g) { return (int)fmin(fmax(rint((double)v * g), -32768.0), 32767.0); }

// y[dst_off + i] = scaled(x[src_off + i]) for i < n; the thread that stores a sample is the only one that reads it, so y may be x itself
__global__ __launch_bounds__(256) void loud_apply_kernel(const int16_t* x, long long n_x, const long long* __restrict__ rows,
                                                         const double* __restrict__ stats, int16_t* y, long long n_y) {
    const long long* r = rows + 4 * (long long)blockIdx.y;
    const long long so = r[0], A = r[2];
    long long B = r[2] + r[1];
    if (B > n_y) B = n_y;
    if (A < 0 || B <= A || so < 0 || so + (B - A) > n_x) return;
    const double g = stats[4 * (long long)blockIdx.y + 3];
    const long long src0 = so - A;
    // the groups of four are laid on y's ADDRESS, not on its index: y may start at any even byte, the 8-byte stores stay aligned
    const long long off = (long long)(((uintptr_t)y >> 1) & 3);
    for (long long q = ((A + off) >> 2) + (long long)blockIdx.x * 256 + threadIdx.x; q <= ((B - 1 + off) >> 2); q += (long long)gridDim.x * 256) {
        const long long j0 = q * 4 - off;
        if (j0 >= A && j0 + 4 <= B) {
            int w[4];
#pragma unroll
            for (int k = 0; k < 4; ++k) w[k] = scaled((int)x[src0 + j0 + k], g);
            uint2 u;
            u.x = (uint32_t)(uint16_t)w[0] | ((uint32_t)(uint16_t)w[1] << 16);
            u.y = (uint32_t)(uint16_t)w[2] | ((uint32_t)(uint16_t)w[3] << 16);
            *(uint2*)(y + j0) = u;
        } else {
            for (long long j = j0 > A ? j0 : A; j < j0 + 4 && j < B; ++j) y[j] = (int16_t)scaled((int)x[src0 + j], g);
        }
    }
}

}  // namespace

#ifndef VV_LOUDNESS_HOST_CHECK
// scratch: per run 4 doubles of state, its power, its sub-block slot q, its peak (int64)
unsigned long long vvk_pcm_loudness_ws_bytes(long long total_runs, int R) {
    (void)R;
    return 56ull * (unsigned long long)(total_runs > 0 ? total_runs : 1);
}

int vvk_pcm_loudness(const int16_t* x, long long n_x, const long long* rows, int R, long long sub, long long total_runs, long long max_n,
                     const double* tables, const double* params, int16_t* y, long long n_y, double* stats, void* ws, hipStream_t st,
                     const char** err) {
    if (R < 1 || R > 65535 || sub < RUN || total_runs < 0 || total_runs >= (1ll << 31) * RPB || n_x < 0 || n_y < 0 || max_n < 0) {
        *err = "pcm_loudness: bad sizes (1 <= R <= 65535, sub >= 128)";
        return -22;
    }
    if (!x || !rows || !tables || !params || !stats || !ws) { *err = "pcm_loudness: null pointer"; return -22; }
    const int rps = (int)((sub + RUN - 1) / RUN);
    double* state = (double*)ws;
    double* power = state + 4 * total_runs;
    double* qbuf = power + total_runs;
    long long* peak = (long long*)(qbuf + total_runs);
    if (total_runs > 0) {
        const unsigned blocks = (unsigned)((total_runs + RPB - 1) / RPB);
        loud_run_kernel<0><<<blocks, RPB, 0, st>>>(x, n_x, rows, R, sub, rps, total_runs, tables, state, power, peak);
        loud_scan_kernel<<<R, 64, 0, st>>>(rows, sub, rps, total_runs, tables, state);
        loud_run_kernel<1><<<blocks, RPB, 0, st>>>(x, n_x, rows, R, sub, rps, total_runs, tables, state, power, peak);
    }
    loud_gate_kernel<<<R, 256, 0, st>>>(rows, sub, rps, total_runs, tables, params, power, peak, qbuf, state, stats);
    if (y && max_n > 0) {
        long long bx = (max_n / 4 + 256) / 256;
        if (bx > 2048) bx = 2048;
        loud_apply_kernel<<<dim3((unsigned)bx, R), 256, 0, st>>>(x, n_x, rows, stats, y, n_y);
    }
    hipError_t he = hipGetLastError();
    if (he != hipSuccess) { *err = hipGetErrorString(he); return -5; }
    return 0;
}
#endif
