// N10: the output stage on the device -- what TTSEngine.synthesize did on the host after vv_decode.
//   join     : AudioProcessor.concatenate_with_crossfade_improved (reference core/audio_processor.py:122-192) for R requests per call,
//              BIT-EXACT to the reference function (tests/golden/output_golden.npz is produced by running it): clip repair per raw
//              chunk, RMS level match in numpy's float32 summation order (vv_np_sum.h, the order of the clip ingest), cos^2 mix in
//              float64 with the host's own linspace / cos / sin tables (the device never evaluates cos: a last-bit difference would flip
//              a truncation).  Every length is known on the host, so positions, junction sizes and final owners arrive as descriptor rows.
//                flag pass : one workgroup per chunk: does it hold a 32767 sample?
//                walk      : one workgroup per request walks its junctions in order (gain i depends on the joined tail, which depends
//                            on gain i-1 after truncation, and on earlier mixes when a chunk is shorter than 2n); the running tail of
//                            at most max_n samples lives in an LDS ring indexed by position; writes the gains and the FINAL mixed samples
//                body      : every other sample once, repair -> gain -> store
//              no atomics; every output sample of a request is written exactly once, nothing outside [0, joined_len) of its slice.
//   resample : int16 -> int16 polyphase FIR, the arithmetic of resample_poly_kernel (vv_ingest.hip): one float64 fma chain over ascending
//              input index, then clamp(rint(acc)); rows carry (m0, i0) so that a clip cut into blocks equals the whole clip bit for bit.
//   encode   : G.711 mu-law / A-law, the segment arithmetic of CPython's Modules/audioop.c (lin2ulaw / lin2alaw at width 2), plain
//              integer code, eight samples packed per store where the destination allows.
// Rounding matters in every line of the join: no fma may form where numpy rounds a product and a sum separately.
#pragma clang fp contract(off)
#ifndef VV_OUTPUT_HOST_CHECK          // tools/output_host_check.cpp compiles the kernels below for the host, on tools/hip_host_shim.h
#include "vv_common.h"
#include "vv_kernels.h"
#endif
#include "vv_np_sum.h"

namespace {

constexpr int JOIN_MAX_N = 24576;             // VV_JOIN_MAX_N: the walk keeps 2 * n bytes of joined tail in LDS (48 KB)
constexpr double CLIP_REPAIR = 26214.0 / 32767;   // fix_clipped_audio: 80 % of full scale over the peak, float64 like numpy's scalar

__device__ __forceinline__ int ld_pcm(const int16_t* __restrict__ pcm, long long n_pcm, long long j) {
    return (j >= 0 && j < n_pcm) ? (int)pcm[j] : 0;                              // the rows were validated by the caller; clamped all the same
}
// fix_clipped_audio on a chunk that holds a 32767 sample: (int16)(x * (26214.0 / 32767)) in float64, truncated toward zero
__device__ __forceinline__ int repaired(int x, int flag) { return flag ? (int)((double)x * CLIP_REPAIR) : x; }
// (nxt.astype(float32) * gain).astype(int16): numpy on x86 truncates to int32 and keeps the low 16 bits (a wrap is allowed)
__device__ __forceinline__ int gained(int x, float g) { return (int)(int16_t)(int)((float)x * g); }

// ---------------------------------------------------------------- join
// chunk row (8 int64): {src_off, len, pos, n, fin, tab_off, repair, req}
//   pos = position of the chunk's first sample inside its request's joined signal (= joined length so far - n), n = junction size with
//   what was joined before (0: first chunk / appended), fin = samples of this chunk are FINAL at positions < fin (a later junction rewrites
//   the rest), tab_off = offset (doubles) of this junction's c[n] | s[n] in `fade`, repair = 1 in a request of >= 2 chunks, req = its request
// request row (4 int64): {chunk0, n_chunks, out_off, joined_len}
__global__ __launch_bounds__(256) void join_flag_kernel(const int16_t* __restrict__ pcm, long long n_pcm, const long long* __restrict__ rows,
                                                        int* __restrict__ flags) {
    const long long* r = rows + 8 * (long long)blockIdx.x;
    long long so = r[0], len = r[1];
    if (!r[6] || len <= 0 || so < 0 || so >= n_pcm) {
        if (threadIdx.x == 0) flags[blockIdx.x] = 0;
        return;
    }
    if (so + len > n_pcm) len = n_pcm - so;
    const int16_t* p = pcm + so;
    long long head = (long long)((16 - ((uintptr_t)p & 15)) & 15) >> 1;          // samples up to the next 16-byte boundary
    if (head > len) head = len;
    int hit = 0;
    for (long long i = threadIdx.x; i < head; i += 256) hit |= p[i] == 32767;
    const long long nvec = (len - head) >> 3;
    const uint4* q = (const uint4*)(p + head);
    for (long long i = threadIdx.x; i < nvec; i += 256) {
        const uint4 w = q[i];
        const unsigned ww[4] = {w.x, w.y, w.z, w.w};
#pragma unroll
        for (int k = 0; k < 4; ++k) hit |= ((ww[k] & 0xffffu) == 0x7fffu) | ((ww[k] >> 16) == 0x7fffu);
    }
    for (long long i = head + nvec * 8 + threadIdx.x; i < len; i += 256) hit |= p[i] == 32767;
    hit = __syncthreads_or(hit);
    if (threadIdx.x == 0) flags[blockIdx.x] = hit ? 1 : 0;
}

__global__ __launch_bounds__(256) void join_walk_kernel(const int16_t* __restrict__ pcm, long long n_pcm, const long long* __restrict__ rows,
                                                        const long long* __restrict__ reqs, const double* __restrict__ fade, long long n_fade,
                                                        const int* __restrict__ flags, float* __restrict__ gains, int16_t* __restrict__ out,
                                                        long long n_out, int C, int n_chunks) {
#ifndef VV_OUTPUT_HOST_CHECK
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
#else
    unsigned char* const smem = vv_host::dynamic_lds();                         // the block of the size given at launch
#endif
    float* v = (float*)smem;                                                     // 128 floats of the pairwise tree
    int16_t* S = (int16_t*)(smem + 512);                                         // S[p % C] = joined sample at position p, the last C positions
    const long long* rq = reqs + 4 * (long long)blockIdx.x;
    const long long c0 = rq[0], oo = rq[2], jl = rq[3];
    const int nc = (int)rq[1];
    const int tid = threadIdx.x;
    if (c0 < 0 || nc < 1 || c0 + nc > n_chunks) return;
    if (tid == 0) gains[c0] = 1.f;
    if (nc < 2) return;                                                          // a single chunk is copied untouched by the body kernel
    long long total;
    {
        const long long* r = rows + 8 * c0;
        const long long so = r[0];
        const int fl = flags[c0];
        total = r[1];
        for (long long p = (total > C ? total - C : 0) + tid; p < total; p += 256) S[p % C] = (int16_t)repaired(ld_pcm(pcm, n_pcm, so + p), fl);
    }
    __syncthreads();
    for (int k = 1; k < nc; ++k) {
        const long long* r = rows + 8 * (c0 + k);
        const long long so = r[0], len = r[1], P = r[2], fin = r[4], tab = r[5];
        const int n = (int)r[3];
        const int fl = flags[c0 + k];
        if (P < 0 || len <= 0) return;                                           // refused by the caller's validation; uniform over the workgroup
        float g = 1.f;
        if (n > 0 && n <= C) {
            float sp = 0.f, sn = 0.f;                                            // np.mean's buffer sums, accumulated in order
            for (int b = 0; b < n; b += NP_BUF) {
                const int L = n - b < NP_BUF ? n - b : NP_BUF;
                const int base = (int)((P + b) % C);
                sp += np_buffer_sum([&](int i) { int j = base + i; if (j >= C) j -= C; const float f = (float)S[j]; return f * f; }, L, v);
                sn += np_buffer_sum([&](int i) { const float f = (float)repaired(ld_pcm(pcm, n_pcm, so + b + i), fl); return f * f; }, L, v);
            }
            // float32 quotient and root through float64: the double rounding is innocuous for / and sqrt at these widths
            const float rms_prev = (float)sqrt((double)(float)((double)sp / (double)n));
            const float rms_next = (float)sqrt((double)(float)((double)sn / (double)n));
            if (rms_prev > 100.f && rms_next > 100.f) g = fminf(fmaxf((float)((double)rms_prev / (double)rms_next), 0.7f), 1.5f);
            const double* ct = fade + tab;
            const bool tab_ok = tab >= 0 && tab + 2ll * n <= n_fade;
            const int base = (int)(P % C);
            for (int i = tid; i < n; i += 256) {
                int j = base + i;
                if (j >= C) j -= C;
                const double t = (double)S[j];
                const double h = (double)gained(repaired(ld_pcm(pcm, n_pcm, so + i), fl), g);
                const double c = tab_ok ? ct[i] : 1.0, s = tab_ok ? ct[n + i] : 0.0;
                const int m = (int)(int16_t)(int)(t * c + h * s);                // float64, every operation rounded; truncated toward zero
                S[j] = (int16_t)m;
                const long long p = P + i;
                if (p < fin && p < jl && oo + p >= 0 && oo + p < n_out) out[oo + p] = (int16_t)m;
            }
        }
        if (tid == 0) gains[c0 + k] = g;
        __syncthreads();
        const long long prev = P + (n > 0 ? n : 0), total_new = P + len;         // the chunk's remaining samples enter the ring
        for (long long p = (total_new - C > prev ? total_new - C : prev) + tid; p < total_new; p += 256)
            S[p % C] = (int16_t)gained(repaired(ld_pcm(pcm, n_pcm, so + (p - P)), fl), g);
        total = total_new;
        __syncthreads();
    }
    (void)total;
}

// every sample that no junction rewrites: positions [pos + n, min(pos + len, fin)) of each chunk, four per thread on the output's 8-byte grid
__global__ __launch_bounds__(256) void join_body_kernel(const int16_t* __restrict__ pcm, long long n_pcm, const long long* __restrict__ rows,
                                                        const long long* __restrict__ reqs, const int* __restrict__ flags,
                                                        const float* __restrict__ gains, int16_t* __restrict__ out, long long n_out, int R) {
    const long long* r = rows + 8 * (long long)blockIdx.y;
    const long long so = r[0], len = r[1], P = r[2], n = r[3] > 0 ? r[3] : 0, fin = r[4];
    if (r[7] < 0 || r[7] >= R) return;
    const long long* rq = reqs + 4 * r[7];
    const long long oo = rq[2], jl = rq[3];
    long long b = P + len;
    if (b > fin) b = fin;
    if (b > jl) b = jl;
    const long long A = oo + P + n;
    long long B = oo + b;
    if (B > n_out) B = n_out;
    if (A < 0 || B <= A) return;
    const int fl = flags[blockIdx.y];
    const float g = gains[blockIdx.y];
    const long long src0 = so - (oo + P);                                        // source index = src0 + absolute output index
    for (long long q = (A >> 2) + (long long)blockIdx.x * 256 + threadIdx.x; q <= ((B - 1) >> 2); q += (long long)gridDim.x * 256) {
        const long long j0 = q * 4;
        if (j0 >= A && j0 + 4 <= B) {
            int w[4];
#pragma unroll
            for (int k = 0; k < 4; ++k) w[k] = gained(repaired(ld_pcm(pcm, n_pcm, src0 + j0 + k), fl), g);
            uint2 u;
            u.x = (uint32_t)(uint16_t)w[0] | ((uint32_t)(uint16_t)w[1] << 16);
            u.y = (uint32_t)(uint16_t)w[2] | ((uint32_t)(uint16_t)w[3] << 16);
            *(uint2*)(out + j0) = u;
        } else {
            for (long long j = j0 > A ? j0 : A; j < j0 + 4 && j < B; ++j) out[j] = (int16_t)gained(repaired(ld_pcm(pcm, n_pcm, src0 + j), fl), g);
        }
    }
}

// ---------------------------------------------------------------- polyphase rate conversion, int16 -> int16
// row (6 int64): {src_off, n_in, dst_off, n_out, m0, i0}: outputs m0 ... m0 + n_out - 1 of a signal whose samples i0 ... i0 + n_in - 1 are given
__global__ __launch_bounds__(256) void pcm_resample_kernel(const int16_t* __restrict__ x, long long n_x, const long long* __restrict__ rows,
                                                           const double* __restrict__ h, int n_taps, int up, int down, int skip,
                                                           int16_t* __restrict__ y, long long n_y) {
    const long long* r = rows + 6 * (long long)blockIdx.y;
    const long long so = r[0], n_in = r[1], dof = r[2], n_out = r[3], m0 = r[4], i0 = r[5];
    for (long long j = (long long)blockIdx.x * 256 + threadIdx.x; j < n_out; j += (long long)gridDim.x * 256) {
        const long long pos = (m0 + j + skip) * down;                            // index into the zero-stuffed signal
        // taps k = pos - i * up in [0, n_taps): i in [ceil((pos - n_taps + 1) / up), floor(pos / up)], cut to the samples given
        long long i_hi = pos / up;
        const long long lo_num = pos - n_taps + 1;
        long long i_lo = lo_num <= 0 ? 0 : (lo_num + up - 1) / up;
        if (i_lo < i0) i_lo = i0;
        if (i_hi > i0 + n_in - 1) i_hi = i0 + n_in - 1;
        if (so + (i_lo - i0) < 0) i_lo = i0 - so;
        if (so + (i_hi - i0) > n_x - 1) i_hi = n_x - 1 - so + i0;
        double acc = 0.0;
        for (long long i = i_lo; i <= i_hi; ++i) acc = fma((double)x[so + (i - i0)], h[pos - i * up], acc);
        const double v = fmin(fmax(rint(acc), -32768.0), 32767.0);                // ties to even, then the int16 range
        if (dof + j >= 0 && dof + j < n_y) y[dof + j] = (int16_t)(int)v;
    }
}

// ---------------------------------------------------------------- G.711 (CPython Modules/audioop.c: st_14linear2ulaw, st_linear2alaw)
__device__ __forceinline__ unsigned lin2ulaw(int sample) {
    int v = sample >> 2;                                                         // lin2ulaw works on the 14-bit value
    const unsigned mask = v < 0 ? 0x7Fu : 0xFFu;
    if (v < 0) v = -v;
    if (v > 8159) v = 8159;                                                      // CLIP
    v += 0x21;                                                                   // BIAS >> 2
    int seg = 0;
    while (seg < 8 && v > ((0x40 << seg) - 1)) ++seg;                            // seg_uend = 0x3F, 0x7F, ... 0x1FFF
    if (seg >= 8) return 0x7Fu ^ mask;
    return ((unsigned)(seg << 4) | (unsigned)((v >> (seg + 1)) & 0xF)) ^ mask;
}

__device__ __forceinline__ unsigned lin2alaw(int sample) {
    int v = sample >> 3;                                                         // lin2alaw works on the 13-bit value
    const unsigned mask = v >= 0 ? 0xD5u : 0x55u;
    if (v < 0) v = -v - 1;
    int seg = 0;
    while (seg < 8 && v > ((0x20 << seg) - 1)) ++seg;                            // seg_aend = 0x1F, 0x3F, ... 0xFFF
    if (seg >= 8) return 0x7Fu ^ mask;
    const unsigned q = (unsigned)((seg < 2 ? v >> 1 : v >> seg) & 0xF);
    return ((unsigned)(seg << 4) | q) ^ mask;
}

// row (3 int64): {src_off, n, dst_off}; eight samples per thread on the destination's 8-byte grid, a scalar head and tail
template <int KIND>
__global__ __launch_bounds__(256) void pcm_encode_kernel(const int16_t* __restrict__ x, long long n_x, const long long* __restrict__ rows,
                                                         uint8_t* __restrict__ y, long long n_y) {
    const long long* r = rows + 3 * (long long)blockIdx.y;
    const long long so = r[0], A = r[2];
    long long B = r[2] + r[1];
    if (B > n_y) B = n_y;
    if (A < 0 || B <= A) return;
    const long long src0 = so - A;
    for (long long q = (A >> 3) + (long long)blockIdx.x * 256 + threadIdx.x; q <= ((B - 1) >> 3); q += (long long)gridDim.x * 256) {
        const long long j0 = q * 8;
        if (j0 >= A && j0 + 8 <= B) {
            int w[8];
            const long long s0 = src0 + j0;
            if (s0 >= 0 && s0 + 8 <= n_x && (((uintptr_t)(x + s0)) & 15) == 0) {
                const uint4 u = *(const uint4*)(x + s0);
                const unsigned uu[4] = {u.x, u.y, u.z, u.w};
#pragma unroll
                for (int k = 0; k < 4; ++k) { w[2 * k] = (int)(int16_t)(uu[k] & 0xffffu); w[2 * k + 1] = (int)(int16_t)(uu[k] >> 16); }
            } else {
#pragma unroll
                for (int k = 0; k < 8; ++k) w[k] = ld_pcm(x, n_x, s0 + k);
            }
            unsigned b[8];
#pragma unroll
            for (int k = 0; k < 8; ++k) b[k] = KIND == 1 ? lin2ulaw(w[k]) : lin2alaw(w[k]);
            uint2 o;
            o.x = b[0] | (b[1] << 8) | (b[2] << 16) | (b[3] << 24);
            o.y = b[4] | (b[5] << 8) | (b[6] << 16) | (b[7] << 24);
            *(uint2*)(y + j0) = o;
        } else {
            for (long long j = j0 > A ? j0 : A; j < j0 + 8 && j < B; ++j) {
                const int s = ld_pcm(x, n_x, src0 + j);
                y[j] = (uint8_t)(KIND == 1 ? lin2ulaw(s) : lin2alaw(s));
            }
        }
    }
}

#ifndef VV_OUTPUT_HOST_CHECK
inline int launched(const char** err) {
    hipError_t he = hipGetLastError();
    if (he != hipSuccess) { *err = hipGetErrorString(he); return -5; }
    return 0;
}
#endif

}  // namespace

#ifndef VV_OUTPUT_HOST_CHECK
int vvk_join_max_n() { return JOIN_MAX_N; }

int vvk_join_chunks(const int16_t* pcm, long long n_pcm, const long long* chunk_rows, int n_chunks, const long long* req_rows, int R,
                    const double* fade, long long n_fade, int max_n, long long max_len, int16_t* out, long long n_out, void* ws,
                    hipStream_t st, const char** err) {
    if (R < 1 || n_chunks < R || n_chunks > 65535 || n_pcm < 0 || n_out < 0 || n_fade < 0 || max_len < 0 || max_n < 0) {
        *err = "join_chunks: bad sizes (1 <= R <= n_chunks <= 65535)";
        return -22;
    }
    if (max_n > JOIN_MAX_N) { *err = "join_chunks: a junction of more than 24576 samples (VV_JOIN_MAX_N)"; return -22; }
    if (!pcm || !chunk_rows || !req_rows || !out || !ws || (max_n > 0 && !fade)) { *err = "join_chunks: null pointer"; return -22; }
    if ((uintptr_t)out % 16 || (uintptr_t)ws % 8 || (uintptr_t)fade % 8) { *err = "join_chunks: misaligned buffer (out 16 bytes; ws, fade 8)"; return -22; }
    int* flags = (int*)ws;
    float* gains = (float*)(flags + n_chunks);
    const int C = max_n > 8 ? (max_n + 7) / 8 * 8 : 8;
    join_flag_kernel<<<n_chunks, 256, 0, st>>>(pcm, n_pcm, chunk_rows, flags);
    join_walk_kernel<<<R, 256, 512 + 2 * (size_t)C, st>>>(pcm, n_pcm, chunk_rows, req_rows, fade, n_fade, flags, gains, out, n_out, C, n_chunks);
    long long bx = (max_len / 4 + 256) / 256;
    if (bx > 1024) bx = 1024;
    if (bx < 1) bx = 1;
    join_body_kernel<<<dim3((unsigned)bx, n_chunks), 256, 0, st>>>(pcm, n_pcm, chunk_rows, req_rows, flags, gains, out, n_out, R);
    return launched(err);
}

int vvk_pcm_resample(const int16_t* x, long long n_x, const long long* rows, int n_rows, long long max_out, const double* taps, int n_taps,
                     int up, int down, int skip, int16_t* y, long long n_y, hipStream_t st, const char** err) {
    if (n_rows < 1 || n_rows > 65535 || n_x < 0 || n_y < 0 || max_out < 0 || n_taps < 1 || up < 1 || down < 1 || skip < 0) {
        *err = "pcm_resample: bad sizes";
        return -22;
    }
    if (!x || !rows || !taps || !y || (uintptr_t)taps % 8 || (uintptr_t)rows % 8) { *err = "pcm_resample: null or misaligned pointer"; return -22; }
    if (max_out == 0) return 0;
    long long bx = (max_out + 255) / 256;
    if (bx > 4096) bx = 4096;
    pcm_resample_kernel<<<dim3((unsigned)bx, n_rows), 256, 0, st>>>(x, n_x, rows, taps, n_taps, up, down, skip, y, n_y);
    return launched(err);
}

int vvk_pcm_encode(const int16_t* x, long long n_x, const long long* rows, int n_rows, long long max_n, int kind, uint8_t* y, long long n_y,
                   hipStream_t st, const char** err) {
    if (n_rows < 1 || n_rows > 65535 || n_x < 0 || n_y < 0 || max_n < 0) { *err = "pcm_encode: bad sizes"; return -22; }
    if (kind != 1 && kind != 2) { *err = "pcm_encode: kind is 1 (mu-law) or 2 (A-law)"; return -22; }
    if (!x || !rows || !y || (uintptr_t)y % 8 || (uintptr_t)rows % 8) { *err = "pcm_encode: null or misaligned pointer (y 8 bytes)"; return -22; }
    if (max_n == 0) return 0;
    long long bx = (max_n / 8 + 256) / 256;
    if (bx > 2048) bx = 2048;
    const dim3 grid((unsigned)bx, n_rows);
    if (kind == 1) pcm_encode_kernel<1><<<grid, 256, 0, st>>>(x, n_x, rows, y, n_y);
    else pcm_encode_kernel<2><<<grid, 256, 0, st>>>(x, n_x, rows, y, n_y);
    return launched(err);
}
#endif
