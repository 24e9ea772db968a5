// N13: look-ahead peak limiter of the joined signal on the device -- a sample-peak or 4x oversampled true-peak estimate, the
// gain that holds it under the ceiling, a sliding minimum and a raised-cosine window average over the look-ahead, applied in HBM.
// The arithmetic is the specification: core/audio_processor.py (limit_peaks) computes the same float64 operations in the same order,
// so the two agree bit for bit.  Every quantity is a finite-window function of the input (no recursion): a sample depends on the
// W = 2L + H samples on either side only, so a request is the same alone, in a batch, or cut into blocks with W samples of context.
//     offsets: one thread: every request's first slot in the gain plane and in the tile records (prefix sums of n and of its tiles)
//     gain   : grid (tile, request): x of the tile +- W into LDS; r = c / e over the tile +- 2L; d = 1 - min r over the tile +- L;
//              s = min(1 - sum w d, r) over the tile -> the gain plane (float64), and the tile's {e_max, s_min, count of s < 1}
//     stats  : one wave per request folds its tile records (min, max and a count: exact in any order) -> {g, e_max, s_min, n_limited}
//     apply  : y = clamp(rint((x * g) * s)) over the row's output window, four samples per thread on the 8-byte grid of the
//              destination's address, a scalar head and tail.  It writes what the gain pass reads, hence a launch of its own.
// No atomics, no reordered sums; every product and sum is rounded on its own:
#pragma clang fp contract(off)
#ifndef VV_LIMITER_HOST_CHECK         // tools/limiter_host_check.cpp compiles the kernels below for the host, with its own stand-ins
#include "vv_common.h"
#include "vv_kernels.h"
#endif

namespace {

constexpr int LH = 12;                        // VV_LIMIT_H
constexpr int MAX_L = 1024;                   // VV_LIMIT_MAX_L
constexpr int POOL = 7424;                    // float64 slots of LDS for r (tile + 4L) and d (tile + 2L); x is staged where d goes later
constexpr int NT = 256;                       // threads of the gain pass

// the tile (output samples per workgroup) for a look-ahead: the largest of 2048, 1024, 512 with 2 tile + 6 L <= POOL
__host__ __device__ inline int limit_tile(int L) { return 4096 + 6 * L <= POOL ? 2048 : 2048 + 6 * L <= POOL ? 1024 : 512; }
static_assert(1024 + 6 * MAX_L <= POOL, "the smallest tile must fit the largest look-ahead");
static_assert(POOL * 8 + NT * 20 <= 65536, "static LDS");

// rows R x 5 int64 {src_off, n, dst_off, out_lo, out_n}; offs R x 2 int64 {first gain slot, first tile record}
__global__ __launch_bounds__(64) void limit_offsets_kernel(const long long* __restrict__ rows, int R, int tile, long long* __restrict__ offs) {
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    long long s = 0, t = 0;
    for (int r = 0; r < R; ++r) {
        const long long n = rows[5 * (long long)r + 1];
        offs[2 * (long long)r] = s;
        offs[2 * (long long)r + 1] = t;
        if (n > 0) { s += n; t += (n + tile - 1) / tile; }
    }
}

// the pre-gain of request r: under a loudness target sqrt(T / zbar) from the measure call's {zbar, kept, P, g}, uncapped; else g0
__device__ __forceinline__ double limit_pregain(const double* __restrict__ params, const double* __restrict__ meas, long long r) {
    const double T = params[3 * r];
    if (meas && T > 0.0) {
        const double zbar = meas[4 * r], kept = meas[4 * r + 1], P = meas[4 * r + 2];
        return kept > 0.0 && P > 0.0 ? sqrt(T / zbar) : 1.0;
    }
    return params[3 * r + 2];
}

__global__ __launch_bounds__(NT) void limit_gain_kernel(const int16_t* __restrict__ x, long long n_x, const long long* __restrict__ rows,
                                                        const long long* __restrict__ offs, int L, int tile, int mode,
                                                        const double* __restrict__ window, const double* __restrict__ taps,
                                                        const double* __restrict__ params, const double* __restrict__ meas,
                                                        long long total_samples, long long total_tiles, double* __restrict__ gains,
                                                        double* __restrict__ recs) {
    __shared__ double pool[POOL];
    __shared__ double red_e[NT];
    __shared__ double red_s[NT];
    __shared__ int red_c[NT];
    const long long req = blockIdx.y;
    const long long so = rows[5 * req], n = rows[5 * req + 1];
    const long long t0 = (long long)blockIdx.x * tile;
    const int tid = threadIdx.x;
    if (n <= 0 || t0 >= n || so < 0 || so + n > n_x) return;                       // the rows were validated on the host; checked all the same
    const long long s_off = offs[2 * req], t_off = offs[2 * req + 1] + blockIdx.x;
    if (s_off < 0 || s_off + n > total_samples || t_off < 0 || t_off >= total_tiles) return;
    const int tl = n - t0 < tile ? (int)(n - t0) : tile;                           // samples of this tile
    const int W = 2 * L + LH;
    double* rbuf = pool;                                                           // r[q] of sample t0 - 2L + q, q < tl + 4L
    double* dbuf = pool + tile + 4 * L;                                            // d[p] of sample t0 - L + p, p < tl + 2L
    int16_t* xs = (int16_t*)dbuf;                                                  // x[idx] of sample t0 - W + idx, idx < tl + 2W; zero outside [0, n)
    for (int idx = tid; idx < tl + 2 * W; idx += NT) {
        const long long gi = t0 - W + idx;
        xs[idx] = gi >= 0 && gi < n ? x[so + gi] : (int16_t)0;
    }
    __syncthreads();
    const double g = limit_pregain(params, meas, req);
    const double c = params[3 * req + 1];
    double e_max = 0.0;
    for (int q = tid; q < tl + 4 * L; q += NT) {
        const long long gi = t0 - 2 * L + q;
        double r = 1.0;
        if (gi >= 0 && gi < n) {
            double e = fabs((double)xs[q + LH] * g);
            if (mode == 1) {
#pragma unroll
                for (int p = 1; p <= 3; ++p) {
                    double u = 0.0;
                    for (int j = -LH + 1; j <= LH; ++j) u = u + taps[4 * LH + p - 4 * j] * ((double)xs[q + LH + j] * g);
                    e = fmax(e, fabs(u));
                }
            }
            if (e > c) r = c / e;
            if (q >= 2 * L && q < 2 * L + tl) e_max = fmax(e_max, e);
        }
        rbuf[q] = r;
    }
    __syncthreads();                                                               // xs has been read: d takes its place
    const long long qbase = t0 - 2 * L;                                            // sample of rbuf[0]
    for (int p = tid; p < tl + 2 * L; p += NT) {
        const long long gi = t0 - L + p;
        double m = 1.0;
        if (gi >= 0 && gi < n) {
            for (long long j = gi - L; j <= gi + L; ++j) {
                const long long jc = j < 0 ? 0 : j > n - 1 ? n - 1 : j;
                m = fmin(m, rbuf[jc - qbase]);
            }
        }
        dbuf[p] = 1.0 - m;
    }
    __syncthreads();
    const long long pbase = t0 - L;                                                // sample of dbuf[0]
    double s_min = 1.0;
    int cnt = 0;
    for (int i = tid; i < tl; i += NT) {
        const long long gi = t0 + i;
        double A = 0.0;
        for (int k = -L; k <= L; ++k) {
            const long long j = gi + k;
            const long long jc = j < 0 ? 0 : j > n - 1 ? n - 1 : j;
            A = A + window[k + L] * dbuf[jc - pbase];
        }
        const double s = fmin(1.0 - A, rbuf[i + 2 * L]);
        gains[s_off + gi] = s;
        s_min = fmin(s_min, s);
        cnt += s < 1.0 ? 1 : 0;
    }
    red_e[tid] = e_max; red_s[tid] = s_min; red_c[tid] = cnt;
    __syncthreads();
    for (int h = NT / 2; h > 0; h >>= 1) {                                         // a maximum, a minimum and an integer count: exact in any order
        if (tid < h) {
            red_e[tid] = fmax(red_e[tid], red_e[tid + h]);
            red_s[tid] = fmin(red_s[tid], red_s[tid + h]);
            red_c[tid] += red_c[tid + h];
        }
        __syncthreads();
    }
    if (tid == 0) { recs[3 * t_off] = red_e[0]; recs[3 * t_off + 1] = red_s[0]; recs[3 * t_off + 2] = (double)red_c[0]; }
}

// stats[r] = {g, e_max, s_min, n_limited} over the row's n samples
__global__ __launch_bounds__(64) void limit_stats_kernel(const long long* __restrict__ rows, const long long* __restrict__ offs, int tile,
                                                         const double* __restrict__ params, const double* __restrict__ meas,
                                                         long long total_tiles, const double* __restrict__ recs, double* __restrict__ stats) {
    __shared__ double red_e[64];
    __shared__ double red_s[64];
    __shared__ double red_c[64];
    const long long req = blockIdx.x;
    const long long n = rows[5 * req + 1], t_off = offs[2 * req + 1];
    long long nt = n > 0 ? (n + tile - 1) / tile : 0;
    if (t_off < 0 || t_off > total_tiles) nt = 0;
    else if (nt > total_tiles - t_off) nt = total_tiles - t_off;
    const int tid = threadIdx.x;
    double e_max = 0.0, s_min = 1.0, cnt = 0.0;                                    // the count stays below 2^53: exact in float64
    for (long long t = tid; t < nt; t += 64) {
        e_max = fmax(e_max, recs[3 * (t_off + t)]);
        s_min = fmin(s_min, recs[3 * (t_off + t) + 1]);
        cnt = cnt + recs[3 * (t_off + t) + 2];
    }
    red_e[tid] = e_max; red_s[tid] = s_min; red_c[tid] = cnt;
    __syncthreads();
    for (int h = 32; h > 0; h >>= 1) {
        if (tid < h) {
            red_e[tid] = fmax(red_e[tid], red_e[tid + h]);
            red_s[tid] = fmin(red_s[tid], red_s[tid + h]);
            red_c[tid] = red_c[tid] + red_c[tid + h];
        }
        __syncthreads();
    }
    if (tid == 0) {
        double* st = stats + 4 * req;
        st[0] = limit_pregain(params, meas, req); st[1] = red_e[0]; st[2] = red_s[0]; st[3] = red_c[0];
    }
}

__device__ __forceinline__ int limited(int v, double g, double s) { return (int)fmin(fmax(rint(((double)v * g) * s), -32768.0), 32767.0); }

// y[dst_off + i] = limited(x[src_off + out_lo + i]) for i < out_n; the thread that stores a sample is the only one that reads it, so
// y may be x itself with dst_off == src_off + out_lo
__global__ __launch_bounds__(256) void limit_apply_kernel(const int16_t* x, long long n_x, const long long* __restrict__ rows,
                                                          const long long* __restrict__ offs, const double* __restrict__ params,
                                                          const double* __restrict__ meas, long long total_samples,
                                                          const double* __restrict__ gains, int16_t* y, long long n_y) {
    const long long req = blockIdx.y;
    const long long* r = rows + 5 * req;
    const long long so = r[0], n = r[1], A = r[2], lo = r[3], on = r[4];
    const long long B = A + on, s_off = offs[2 * req];
    if (so < 0 || n < 0 || A < 0 || lo < 0 || on <= 0 || lo + on > n || so + n > n_x || B > n_y || s_off < 0 || s_off + n > total_samples) return;
    const double g = limit_pregain(params, meas, req);
    const long long src0 = so + lo - A;                                            // x index of destination index j: src0 + j
    const long long gain0 = s_off + lo - A;                                        // gain slot of destination index j: gain0 + j
    // the groups of four are laid on y's ADDRESS, not on its index: y may start at any even byte, the 8-byte stores stay aligned
    const long long off = (long long)(((uintptr_t)y >> 1) & 3);
    for (long long q = ((A + off) >> 2) + (long long)blockIdx.x * 256 + threadIdx.x; q <= ((B - 1 + off) >> 2); q += (long long)gridDim.x * 256) {
        const long long j0 = q * 4 - off;
        if (j0 >= A && j0 + 4 <= B) {
            int w[4];
#pragma unroll
            for (int k = 0; k < 4; ++k) w[k] = limited((int)x[src0 + j0 + k], g, gains[gain0 + j0 + k]);
            uint2 u;
            u.x = (uint32_t)(uint16_t)w[0] | ((uint32_t)(uint16_t)w[1] << 16);
            u.y = (uint32_t)(uint16_t)w[2] | ((uint32_t)(uint16_t)w[3] << 16);
            *(uint2*)(y + j0) = u;
        } else {
            for (long long j = j0 > A ? j0 : A; j < j0 + 4 && j < B; ++j) y[j] = (int16_t)limited((int)x[src0 + j], g, gains[gain0 + j]);
        }
    }
}

}  // namespace

#ifndef VV_LIMITER_HOST_CHECK
int vvk_pcm_limit_tile(int L) { return limit_tile(L); }

// scratch: R x 2 int64 offsets | the gain plane, one float64 per sample | three float64 per tile
unsigned long long vvk_pcm_limit_ws_bytes(long long total_samples, long long total_tiles, int R) {
    return 16ull * (unsigned long long)(R > 0 ? R : 1) + 8ull * (unsigned long long)(total_samples > 0 ? total_samples : 0) +
           24ull * (unsigned long long)(total_tiles > 0 ? total_tiles : 0);
}

int vvk_pcm_limit(const int16_t* x, long long n_x, const long long* rows, int R, int L, int mode, long long total_samples,
                  long long total_tiles, long long max_tiles, long long max_out, const double* window, const double* taps,
                  const double* params, const double* meas, int16_t* y, long long n_y, double* stats, void* ws, hipStream_t st,
                  const char** err) {
    if (R < 1 || R > 65535 || L < 1 || L > MAX_L || (mode != 0 && mode != 1) || n_x < 0 || n_y < 0 || total_samples < 0 || total_tiles < 0 ||
        max_tiles < 0 || max_tiles >= (1ll << 31) || max_out < 0) {
        *err = "pcm_limit: bad sizes (1 <= R <= 65535, 1 <= L <= 1024, mode 0 or 1)";
        return -22;
    }
    if (!x || !rows || !window || !taps || !params || !stats || !ws) { *err = "pcm_limit: null pointer"; return -22; }
    const int tile = limit_tile(L);
    long long* offs = (long long*)ws;
    double* gains = (double*)(offs + 2 * (long long)R);
    double* recs = gains + total_samples;
    limit_offsets_kernel<<<1, 64, 0, st>>>(rows, R, tile, offs);
    if (max_tiles > 0)
        limit_gain_kernel<<<dim3((unsigned)max_tiles, R), NT, 0, st>>>(x, n_x, rows, offs, L, tile, mode, window, taps, params, meas,
                                                                        total_samples, total_tiles, gains, recs);
    limit_stats_kernel<<<R, 64, 0, st>>>(rows, offs, tile, params, meas, total_tiles, recs, stats);
    if (y && max_out > 0) {
        long long bx = (max_out / 4 + 256) / 256;
        if (bx > 2048) bx = 2048;
        limit_apply_kernel<<<dim3((unsigned)bx, R), 256, 0, st>>>(x, n_x, rows, offs, params, meas, total_samples, gains, y, n_y);
    }
    hipError_t he = hipGetLastError();
    if (he != hipSuccess) { *err = hipGetErrorString(he); return -5; }
    return 0;
}
#endif
