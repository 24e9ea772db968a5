// N14: pitch and tempo of the joined signal on the device -- a WSOLA time stretch (waveform-similarity overlap-add, Verhelst &
// Roelands 1993) by a ratio p / q; the pitch half is a rate conversion by vv_pcm_resample afterwards.
// The arithmetic is the specification: core/audio_processor.py (time_stretch) computes the same operations, so the two agree bit for bit.
// With N = 512 (frame), HS = 256 (synthesis hop), D = 128 (search radius), x = 0 outside [0, n), n_s = ceil(n p / q), M = ceil(n_s / HS):
//     search : one workgroup per request, frames m = 1 ... M in order (pos_0 = -HS).  The template t[k] = x[pos_{m-1} + HS + k] and the
//              span x[a_m - D, + N + 2D), a_m = floor((m - 1) HS q / p), go to LDS; thread (part, j) sums t[k] x[a_m - D + j + k] over its
//              quarter of k for candidate delta = j - D: an exact integer (|c| < 2^40), so the split and the order are free.  The arg-max
//              runs on the key c * 512 + (511 - rank), rank = 0, 1, 2, 3, 4 ... for delta = 0, -1, 1, -2, 2 ...: among equal c the smallest
//              |delta| wins, the negative one first.  pos_m = a_m + delta, stored as int32 for the caller.
//     blend  : fully parallel over the n_s outputs: y[i] = clamp(rint(w[k + HS] x[pos_{m-1} + HS + k] + w[k] x[pos_m + k])), m = i / HS + 1,
//              k = i - (m - 1) HS, in float64 -- two products rounded on their own, one sum; every sample is written exactly once, four
//              per thread on the 8-byte grid of the destination's address, a scalar head and tail.
// No atomics, no readback; the window w is the host's table (the device never evaluates a cosine):
#pragma clang fp contract(off)
#ifndef VV_PROSODY_HOST_CHECK         // tools/prosody_host_check.cpp compiles the kernels below for the host, with its own stand-ins
#include "vv_common.h"
#include "vv_kernels.h"
#endif

namespace {

constexpr int WN = 512;                       // VV_WSOLA_N
constexpr int WHS = 256;                      // VV_WSOLA_HS
constexpr int WD = 128;                       // VV_WSOLA_D
constexpr int SPAN = WN + 2 * WD;             // samples of x one frame's candidates touch
constexpr int NC = 2 * WD;                    // candidates per frame
constexpr int KS = 4;                         // the sum over k is split over KS groups of NC threads
constexpr int NT = NC * KS;                   // threads of the search pass
constexpr int KPART = WN / KS;
constexpr long long MAX_PQ = 2048;
constexpr long long MAX_N = 1ll << 30;        // samples per request: every position fits an int32, every product below an int64
static_assert(WN == 2 * WHS && NC == 256 && NT == 1024, "the index arithmetic below assumes these");

// the request's signal, zero outside [0, n)
__device__ __forceinline__ int sample_at(const int16_t* __restrict__ xr, long long n, long long i) { return i >= 0 && i < n ? (int)xr[i] : 0; }

// a row {src_off, n, dst_off, p, q, pos_off} that the kernels may follow: inside x, a legal ratio.  The host has checked it; checked all the same
__device__ __forceinline__ bool row_ok(const long long* __restrict__ r, long long n_x) {
    return r[0] >= 0 && r[1] >= 0 && r[1] <= MAX_N && r[1] <= n_x && r[0] <= n_x - r[1] && r[3] >= 1 && r[3] <= MAX_PQ && r[4] >= 1 && r[4] <= MAX_PQ;
}

// plan R x 2 int64 {n_s, M} (n_s = -1: the row was not followed), written here and read by the blend pass
__global__ __launch_bounds__(NT) void stretch_search_kernel(const int16_t* __restrict__ x, long long n_x, const long long* __restrict__ rows,
                                                            int* __restrict__ pos, long long n_pos, long long* __restrict__ plan) {
    __shared__ int s_t[WN];
    __shared__ int s_span[SPAN];
    __shared__ long long s_part[KS * NC];
    __shared__ long long s_key[NC];
    __shared__ long long s_top[16];
    const long long req = blockIdx.x;
    const long long* r = rows + 6 * req;
    const int tid = threadIdx.x;
    const long long n = r[1], p = r[3], q = r[4], po = r[5];
    const bool ok = row_ok(r, n_x);
    const long long n_s = ok ? (n * p + q - 1) / q : 0, M = (n_s + WHS - 1) / WHS;
    if (!ok || po < 0 || po > n_pos || M + 1 > n_pos - po) {                       // uniform over the workgroup
        if (tid == 0) { plan[2 * req] = -1; plan[2 * req + 1] = 0; }
        return;
    }
    if (tid == 0) { plan[2 * req] = n_s; plan[2 * req + 1] = M; pos[po] = -WHS; }
    const int16_t* xr = x + r[0];
    const int j = tid & (NC - 1), k0 = (tid >> 8) * KPART;
    long long prev = -WHS;
    for (long long m = 1; m <= M; ++m) {
        const long long a = ((m - 1) * WHS * q) / p;
        for (int i = tid; i < WN + SPAN; i += NT) {
            if (i < WN) s_t[i] = sample_at(xr, n, prev + WHS + i);
            else s_span[i - WN] = sample_at(xr, n, a - WD + (i - WN));
        }
        __syncthreads();
        long long acc = 0;
#pragma unroll 8
        for (int k = 0; k < KPART; ++k) acc += (long long)s_t[k0 + k] * (long long)s_span[j + k0 + k];
        s_part[tid] = acc;
        __syncthreads();
        if (tid < NC) {
            const long long c = ((s_part[j] + s_part[NC + j]) + s_part[2 * NC + j]) + s_part[3 * NC + j];
            const int d = j - WD;
            const int rank = d < 0 ? -2 * d - 1 : 2 * d;
            s_key[j] = c * 512 + (511 - rank);
        }
        __syncthreads();
        if (tid < 16) {
            long long best = s_key[16 * tid];
            for (int i = 1; i < 16; ++i) { const long long v = s_key[16 * tid + i]; best = v > best ? v : best; }
            s_top[tid] = best;
        }
        __syncthreads();
        long long best = s_top[0];                                                 // every thread folds the 16: no broadcast step
        for (int i = 1; i < 16; ++i) { const long long v = s_top[i]; best = v > best ? v : best; }
        const int rank = 511 - (int)(best & 511);                                  // c * 512 has nine zero bits at the bottom, negative or not
        prev = a + ((rank & 1) ? -((rank + 1) >> 1) : (rank >> 1));
        if (tid == 0) pos[po + m] = (int)prev;
    }
}

__device__ __forceinline__ int blended(const int16_t* __restrict__ xr, long long n, const double* __restrict__ w, const int* __restrict__ pr,
                                       long long i) {
    const long long m1 = i / WHS;                                                  // m - 1
    const int k = (int)(i - m1 * WHS);
    const double tail = w[k + WHS] * (double)sample_at(xr, n, (long long)pr[m1] + WHS + k);
    const double head = w[k] * (double)sample_at(xr, n, (long long)pr[m1 + 1] + k);
    return (int)fmin(fmax(rint(tail + head), -32768.0), 32767.0);
}

__global__ __launch_bounds__(256) void stretch_blend_kernel(const int16_t* __restrict__ x, long long n_x, const long long* __restrict__ rows,
                                                            const double* __restrict__ window, const int* __restrict__ pos, long long n_pos,
                                                            const long long* __restrict__ plan, int16_t* __restrict__ y, long long n_y) {
    const long long req = blockIdx.y;
    const long long* r = rows + 6 * req;
    const long long n = r[1], A = r[2], po = r[5];
    const long long n_s = plan[2 * req], M = plan[2 * req + 1];
    if (n_s <= 0 || !row_ok(r, n_x) || A < 0 || n_s > n_y || A > n_y - n_s || po < 0 || po > n_pos || M + 1 > n_pos - po || n_s > M * WHS) return;
    const long long B = A + n_s;
    const int16_t* xr = x + r[0];
    const int* pr = pos + po;
    // the groups of four are laid on y's ADDRESS, not on its index: y may start at any even byte, the 8-byte stores stay aligned
    const long long off = (long long)(((uintptr_t)y >> 1) & 3);
    for (long long g = ((A + off) >> 2) + (long long)blockIdx.x * 256 + threadIdx.x; g <= ((B - 1 + off) >> 2); g += (long long)gridDim.x * 256) {
        const long long j0 = g * 4 - off;
        if (j0 >= A && j0 + 4 <= B) {
            int v[4];
#pragma unroll
            for (int k = 0; k < 4; ++k) v[k] = blended(xr, n, window, pr, j0 + k - A);
            uint2 u;
            u.x = (uint32_t)(uint16_t)v[0] | ((uint32_t)(uint16_t)v[1] << 16);
            u.y = (uint32_t)(uint16_t)v[2] | ((uint32_t)(uint16_t)v[3] << 16);
            *(uint2*)(y + j0) = u;
        } else {
            for (long long jj = j0 > A ? j0 : A; jj < j0 + 4 && jj < B; ++jj) y[jj] = (int16_t)blended(xr, n, window, pr, jj - A);
        }
    }
}

}  // namespace

#ifndef VV_PROSODY_HOST_CHECK
// scratch: R x 2 int64 {n_s, M}, what the search pass derived from each row and the blend pass follows
unsigned long long vvk_pcm_stretch_ws_bytes(int R) { return 16ull * (unsigned long long)(R > 0 ? R : 1); }

int vvk_pcm_stretch(const int16_t* x, long long n_x, const long long* rows, int R, long long max_out, const double* window, int16_t* y,
                    long long n_y, int* pos, long long n_pos, void* ws, hipStream_t st, const char** err) {
    if (R < 1 || R > 65535 || n_x < 0 || n_y < 0 || n_pos < 0 || max_out < 0) { *err = "pcm_stretch: bad sizes (1 <= R <= 65535)"; return -22; }
    if (!x || !rows || !window || !pos || !ws) { *err = "pcm_stretch: null pointer"; return -22; }
    long long* plan = (long long*)ws;
    stretch_search_kernel<<<R, NT, 0, st>>>(x, n_x, rows, pos, n_pos, plan);
    if (y && max_out > 0) {                                                        // y == NULL: the positions alone
        long long bx = (max_out / 4 + 256) / 256;
        if (bx > 2048) bx = 2048;
        stretch_blend_kernel<<<dim3((unsigned)bx, R), 256, 0, st>>>(x, n_x, rows, window, pos, n_pos, plan, y, n_y);
    }
    hipError_t he = hipGetLastError();
    if (he != hipSuccess) { *err = hipGetErrorString(he); return -5; }
    return 0;
}
#endif
