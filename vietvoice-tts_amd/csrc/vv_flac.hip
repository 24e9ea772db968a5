// N15: FLAC output on the device (RFC 9639) -- mono, 16 bits, frames of 4096 samples, fixed predictors (LPC: N16, below).
// The arithmetic is the specification: core/audio_processor.py (flac_choose, flac_encode_frame) makes the same choices and packs the same
// bits, so the two agree byte for byte.  Everything is integer arithmetic.  Per frame of m samples (the last one of a signal may be short):
//     analyse : one workgroup per frame, 16 samples per thread, the samples in LDS as int32.  For the difference orders o = 0 ... min(4, m - 1)
//               the sums of u >> k (u = the zigzag of the residual, k = 0 ... 14) are taken per FINEST partition (2^pmax of them,
//               pmax = min(4, trailing zero bits of m)): a thread adds its run inside a partition in registers and then into a table in LDS
//               with integer atomics (exact, so the order is free).  The sums are additive, so the coarser partition orders come by
//               pairwise addition up a binary tree.  Per (o, node) the best k (the lowest of equals) and its bits; per (o, po) the size
//               8 + 16 o + 6 + sum (4 + bits); the fewest bits win, ties to the lower o, then the lower po.  All samples equal = a
//               constant subframe; verbatim only when strictly smaller than every Fixed candidate.  |order-4 difference| < 2^20, so
//               u < 2^21 and k <= 14 always suffices: the escape code is never written.  The choice and the frame's bytes go to ws.
//     scan    : one workgroup: the exclusive sum of the frame sizes = each frame's offset in y, and info.
//     pack    : one workgroup per frame again.  Every thread takes the lengths of its 16 codes, a workgroup exclusive sum gives its
//               first bit; bits go most significant first into a zeroed LDS image with atomic OR (a run of zeros is a skipped position).
//               CRC-16 with initial value 0 and no reflection is linear and blind to leading zero bytes: the frame is cut into 32-byte
//               pieces counted from its END, piece t's CRC times x^(256 t) mod P, all XORed.  Then byte stores to the frame's offset.
// No atomics on global memory, no dependence on the execution order, no readback; a frame is written by one workgroup, once.
//
// N16: LPC subframes, opt-in (vv_pcm_flac_lpc, lpc_order 1 ... 12; mirror: flac_lpc_coefficients, flac_choose(x, lpc_order)).  vv_pcm_flac
// launches the LPC = false instances of the kernels below, which are N15 as it was.  The LPC = true analysis has 17 predictors per frame:
// Fixed 0 ... 4 as before, then LPC of order 1 ... min(lpc_order, m - 1):
//     window  : Welch, in integers: w[i] = ((i (m - 1 - i)) << 10) / A, A = h (m - 1 - h), h = (m - 1) / 2 (m >= 3); xw = x w, |xw| <= 2^25
//     lags    : R[l] = sum xw[i] xw[i + l] in int64 (|R| <= 2^62), a thread's 16 products per lag, added in LDS: exact, so the order is free
//     Levinson: one thread, float64, one rounding per operation and no contraction (lpc_quantise at the end of this file, the only
//               floating point here); order p is a candidate while the error stays > 0; its coefficients are quantised to 12 bits with
//               shift = min(11 - exponent of the largest, 15) >= 0 and the rounding error fed forward
//     residual: x[n] - ((sum q[j] x[n - j]) >> shift), n >= p, |sum| < 12 * 2^26: int holds it; u < 2^32, the sums of u >> k in 64 bits
// and the same partition tree and arg-min.  Size 8 + 16 p + 4 + 5 + 12 p + 6 + the partitions; the fewest bits win, Fixed before LPC of
// equals, then the lower order.  The record of a frame grows by {shift, q1 ... q12}; pack writes precision - 1 = 11 (4 bits), the shift
// (5 bits), the coefficients (12 bits each, two's complement) after the warm-up samples and recomputes the residual from those integers.
#ifndef VV_FLAC_HOST_CHECK            // tools/flac_host_check.cpp compiles the kernels below for the host, with its own stand-ins
#include "vv_common.h"
#include "vv_kernels.h"
#endif
#include <type_traits>

namespace {

constexpr int FB = 4096;                      // VV_FLAC_BLOCK
constexpr int NT = 256;                       // threads of every kernel here
constexpr int SPT = FB / NT;                  // samples per thread
constexpr int MAXO = 4;                       // highest fixed predictor order
constexpr int MAXPO = 4;                      // highest partition order searched
constexpr int NK = 15;                        // Rice parameters 0 ... 14
constexpr int NODES = (2 << MAXPO) - 1;       // partitions of every order 0 ... 4 as a binary tree: node (1 << po) - 1 + p
constexpr int HDR_MAX = 15;                   // frame header: 4 fixed bytes, <= 6 of frame number, 2 of block size, 2 of rate, CRC-8
constexpr int IMG_WORDS = (HDR_MAX + 1 + 2 * FB + 2 + 3) / 4 + 1;
constexpr int REC = 4;                        // ints per frame record {bytes, kind | o << 8 | po << 16, k of partitions 0-7, 8-15 (4 bits each)}
constexpr unsigned NODE_CAP = 1u << 24;       // a partition that needs more bits than this loses to verbatim (65,544 bits) anyway
constexpr long long MAX_FRAMES = 1ll << 31;
constexpr int MAXL = 12;                      // highest LPC order (N16)
constexpr int NCAND = MAXO + 1 + MAXL;        // predictors of the LPC analysis: c = 0 ... 4 Fixed of order c, c = 5 ... 16 LPC of order c - 4
constexpr int LPREC = 12;                     // bits of a quantised LPC coefficient
constexpr int LREC = 16;                      // ints per frame of the LPC record {shift, q1 ... q12, 3 unused}
static_assert(SPT == 16 && NODES == 31 && IMG_WORDS * 4 >= HDR_MAX + 1 + 2 * FB + 2 + 4, "the index arithmetic below assumes these");

enum { KIND_CONSTANT = 0, KIND_VERBATIM = 1, KIND_FIXED = 2, KIND_LPC = 3 };

__device__ __forceinline__ long long frames_of(long long n) { return (n + FB - 1) / FB; }

// a row {src_off, n, frame0, last} that the kernels may follow.  The host has checked it; checked all the same
__device__ __forceinline__ bool row_ok(const long long* __restrict__ r, long long n_x) {
    return r[0] >= 0 && r[1] >= 1 && r[1] <= n_x && r[0] <= n_x - r[1] && r[2] >= 0 && r[2] <= MAX_FRAMES - frames_of(r[1]);
}

__device__ __forceinline__ int rate_code(int rate) {
    switch (rate) {
        case 88200: return 1;  case 176400: return 2;  case 192000: return 3;  case 8000: return 4;  case 16000: return 5;  case 22050: return 6;
        case 24000: return 7;  case 32000: return 8;   case 44100: return 9;   case 48000: return 10; case 96000: return 11;
    }
    return rate <= 65535 ? 13 : rate % 10 == 0 ? 14 : 0;
}

__device__ __forceinline__ int number_bytes(long long v) {
    return v < 0x80 ? 1 : v < 0x800 ? 2 : v < 0x10000 ? 3 : v < 0x200000 ? 4 : v < 0x4000000 ? 5 : 6;
}

__device__ __forceinline__ int header_bytes(int m, int rate, long long number) {
    const int rc = rate_code(rate);
    return 4 + number_bytes(number) + (m == FB ? 0 : 2) + (rc == 13 || rc == 14 ? 2 : 0) + 1;
}

// the frame header with its CRC-8 (polynomial 0x07): -> its length, <= HDR_MAX
__device__ int frame_header(unsigned char* h, int m, int rate, long long number) {
    const int rc = rate_code(rate);
    int n = 0;
    h[n++] = 0xFF;
    h[n++] = 0xF8;                                                       // sync, reserved 0, fixed block size
    h[n++] = (unsigned char)(((m == FB ? 12 : 7) << 4) | rc);
    h[n++] = 0x08;                                                       // one channel, 16 bits, reserved 0
    const int nb = number_bytes(number);
    if (nb == 1) {
        h[n++] = (unsigned char)number;
    } else {
        h[n++] = (unsigned char)(((0xFF << (8 - nb)) & 0xFF) | (int)(number >> (6 * (nb - 1))));
        for (int i = nb - 2; i >= 0; --i) h[n++] = (unsigned char)(0x80 | (int)((number >> (6 * i)) & 0x3F));
    }
    if (m != FB) { h[n++] = (unsigned char)((m - 1) >> 8); h[n++] = (unsigned char)((m - 1) & 0xFF); }
    if (rc == 13 || rc == 14) {
        const int v = rc == 13 ? rate : rate / 10;
        h[n++] = (unsigned char)(v >> 8);
        h[n++] = (unsigned char)(v & 0xFF);
    }
    unsigned c = 0;
    for (int i = 0; i < n; ++i) {
        c ^= h[i];
        for (int b = 0; b < 8; ++b) c = (c & 0x80) ? ((c << 1) ^ 0x07) & 0xFF : (c << 1) & 0xFF;
    }
    h[n++] = (unsigned char)c;
    return n;
}

// the frame of this workgroup: blockIdx.y = the row, blockIdx.x = the frame inside it.  False: nothing to do (uniform over the workgroup)
__device__ __forceinline__ bool my_frame(const long long* __restrict__ rows, const long long* __restrict__ fbase, long long n_x, long long& frame,
                                         long long& src, int& m, long long& number) {
    const long long row = blockIdx.y, f = blockIdx.x;
    const long long* r = rows + 4 * row;
    if (!row_ok(r, n_x) || f >= fbase[row + 1] - fbase[row] || f >= frames_of(r[1])) return false;
    frame = fbase[row] + f;
    src = r[0] + f * FB;
    const long long left = r[1] - f * FB;
    m = (int)(left < FB ? left : FB);
    number = r[2] + f;
    return true;
}

// samples into LDS at index i + MAXO, zeros in front and behind
__device__ __forceinline__ void load_frame(int* s_x, const int16_t* __restrict__ x, long long src, int m) {
    for (int i = threadIdx.x; i < FB + MAXO; i += NT) s_x[i] = i >= MAXO && i - MAXO < m ? (int)x[src + i - MAXO] : 0;
}

// residual of order o at sample i >= o (s = s_x + MAXO), as its zigzag u
__device__ __forceinline__ unsigned zigzag_residual(const int* s, int i, int o) {
    int r = s[i];
    if (o == 1) r = s[i] - s[i - 1];
    else if (o == 2) r = s[i] - 2 * s[i - 1] + s[i - 2];
    else if (o == 3) r = s[i] - 3 * s[i - 1] + 3 * s[i - 2] - s[i - 3];
    else if (o == 4) r = s[i] - 4 * s[i - 1] + 6 * s[i - 2] - 4 * s[i - 3] + s[i - 4];
    return r >= 0 ? 2u * (unsigned)r : 2u * (unsigned)(-(r + 1)) + 1u;
}

// the same for an LPC predictor {q1 ... qo, shift}: |sum| < 12 * 2^26 and |r| < 2^31 for 16-bit samples and 12-bit coefficients
__device__ __forceinline__ unsigned zigzag_lpc(const int* s, int i, int o, const int* q, int shift) {
    int sum = 0;
#pragma unroll
    for (int j = 0; j < MAXL; ++j)
        if (j < o) sum += q[j] * s[i - 1 - j];
    const int r = s[i] - (sum >> shift);
    return r >= 0 ? 2u * (unsigned)r : 2u * (unsigned)(-(r + 1)) + 1u;
}

// the bits of a Fixed or LPC subframe of order o in front of its partitions
__device__ __forceinline__ unsigned head_bits(bool lpc, int o) { return 8u + 16u * (unsigned)o + (lpc ? 4u + 5u + (unsigned)(LPREC * o) : 0u) + 6u; }

// N16: the quantised predictors of orders 1 ... lags from the lags R[0 ... lags] (R[0] != 0): shift[p - 1] >= 0 and q[p - 1][0 ... p - 1]
// where order p is a candidate.  Defined at the end of this file, outside this integer-only part
__device__ void lpc_quantise(const unsigned long long* R, int lags, int* shift, int (*q)[MAXL]);

__device__ __forceinline__ int max_part_order(int m) {
    int p = 0;
    while (p < MAXPO && m % (2 << p) == 0) ++p;
    return p;
}

// frames in front of each row: fbase[R + 1], by one workgroup (a thread sums a run of rows, thread 0 scans the runs)
__global__ __launch_bounds__(NT) void flac_plan_kernel(const long long* __restrict__ rows, int R, long long n_x, long long* __restrict__ fbase) {
    __shared__ long long s_sum[NT];
    const int tid = threadIdx.x, per = (R + NT - 1) / NT;
    const int lo = tid * per < R ? tid * per : R, hi = lo + per < R ? lo + per : R;
    long long sum = 0;
    for (int r = lo; r < hi; ++r) sum += row_ok(rows + 4 * (long long)r, n_x) ? frames_of(rows[4 * (long long)r + 1]) : 0;
    s_sum[tid] = sum;
    __syncthreads();
    if (tid == 0) {
        long long run = 0;
        for (int t = 0; t < NT; ++t) { const long long v = s_sum[t]; s_sum[t] = run; run += v; }
        fbase[R] = run;
    }
    __syncthreads();
    long long at = s_sum[tid];
    for (int r = lo; r < hi; ++r) {
        fbase[r] = at;
        at += row_ok(rows + 4 * (long long)r, n_x) ? frames_of(rows[4 * (long long)r + 1]) : 0;
    }
}

// LPC = false: N15.  LPC = true (N16): the NCAND predictors; one that is no candidate (order > m - 1 or lpc_order, s_shift < 0) is skipped
template <bool LPC>
__global__ __launch_bounds__(NT) void flac_analyse_kernel(const int16_t* __restrict__ x, long long n_x, const long long* __restrict__ rows, int rate,
                                                          const long long* __restrict__ fbase, long long n_frames, int* __restrict__ rec,
                                                          int lpc_order, int* __restrict__ lrec) {
    constexpr int NC = LPC ? NCAND : MAXO + 1;
    using acc_t = typename std::conditional<LPC, unsigned long long, unsigned>::type;      // u < 2^32 (LPC), < 2^21 (Fixed); 16 of them
    __shared__ int s_x[FB + 2 * MAXO];
    __shared__ unsigned long long s_sum[NC][NODES][NK];            // sum of u >> k per (predictor, partition node, k)
    __shared__ unsigned s_bits[NC][NODES];                         // 4 + the bits of the node under its best k, capped
    __shared__ unsigned char s_k[NC][NODES];
    __shared__ unsigned s_differs;
    __shared__ unsigned long long s_R[MAXL + 1];                   // LPC only, as the next two
    __shared__ int s_shift[MAXL];
    __shared__ int s_q[MAXL][MAXL];
    long long frame, src, number;
    int m;
    if (!my_frame(rows, fbase, n_x, frame, src, m, number) || frame >= n_frames) return;
    const int tid = threadIdx.x;
    load_frame(s_x, x, src, m);
    for (int i = tid; i < NC * NODES * NK; i += NT) (&s_sum[0][0][0])[i] = 0;
    if (tid == 0) s_differs = 0;
    if constexpr (LPC) {
        if (tid <= MAXL) s_R[tid] = 0;
        if (tid < MAXL) s_shift[tid] = -1;
    }
    __syncthreads();
    const int* s = s_x + MAXO;
    const int omax = m - 1 < MAXO ? m - 1 : MAXO, pmax = max_part_order(m), ps = m >> pmax, leaf0 = (1 << pmax) - 1;
    const int i0 = tid * SPT, i1 = i0 + SPT < m ? i0 + SPT : m;
    const int lags = !LPC ? 0 : lpc_order < m - 1 ? lpc_order : m - 1, cmax = LPC ? NC - 1 : omax;
    if constexpr (LPC) {
        if (m >= 3 && i0 < m) {                                            // this thread's windowed samples and the MAXL behind them
            const unsigned h = (unsigned)(m - 1) / 2, A = h * ((unsigned)(m - 1) - h);
            int xw[SPT + MAXL];
#pragma unroll
            for (int j = 0; j < SPT + MAXL; ++j) {
                const int i = i0 + j;
                xw[j] = i < m ? s[i] * (int)((((unsigned)i * (unsigned)(m - 1 - i)) << 10) / A) : 0;
            }
#pragma unroll
            for (int l = 0; l <= MAXL; ++l) {
                long long r = 0;
#pragma unroll
                for (int j = 0; j < SPT; ++j) r += (long long)xw[j] * xw[j + l];
                if (l <= lags && r) atomicAdd(&s_R[l], (unsigned long long)r);
            }
        }
        __syncthreads();
        if (tid == 0 && m >= 3 && s_R[0]) lpc_quantise(s_R, lags, s_shift, s_q);
        __syncthreads();
    }
    const auto candidate = [&](int c) { return !LPC ? true : c <= MAXO ? c <= omax : c - MAXO <= lags && s_shift[c - MAXO - 1] >= 0; };
    if (i0 < m) {
        bool differs = false;
        for (int i = i0; i < i1; ++i) differs |= s[i] != s[0];
        if (differs) atomicOr(&s_differs, 1u);
        for (int c = 0; c <= cmax; ++c) {
            if (!candidate(c)) continue;
            const int o = LPC && c > MAXO ? c - MAXO : c;
            int shift = 0, q[MAXL];
            if constexpr (LPC) {
                if (c > MAXO) {
                    shift = s_shift[o - 1];
#pragma unroll
                    for (int j = 0; j < MAXL; ++j) q[j] = s_q[o - 1][j];
                }
            }
            acc_t acc[NK];
#pragma unroll
            for (int k = 0; k < NK; ++k) acc[k] = 0;
            int p = i0 / ps, next = (p + 1) * ps;
            for (int i = i0; i < i1; ++i) {
                if (i == next) {                                           // the run crosses into the next partition: flush
#pragma unroll
                    for (int k = 0; k < NK; ++k) { atomicAdd(&s_sum[c][leaf0 + p][k], (unsigned long long)acc[k]); acc[k] = 0; }
                    ++p;
                    next += ps;
                }
                if (i >= o) {
                    const unsigned u = LPC && c > MAXO ? zigzag_lpc(s, i, o, q, shift) : zigzag_residual(s, i, o);
#pragma unroll
                    for (int k = 0; k < NK; ++k) acc[k] += u >> k;
                }
            }
#pragma unroll
            for (int k = 0; k < NK; ++k) atomicAdd(&s_sum[c][leaf0 + p][k], (unsigned long long)acc[k]);
        }
    }
    __syncthreads();
    for (int l = pmax - 1; l >= 0; --l) {                                  // the coarser partition orders: pairwise sums
        const int n = (1 << l) * NK;
        for (int i = tid; i < (cmax + 1) * n; i += NT) {
            const int c = i / n, p = (i - c * n) / NK, k = i - c * n - p * NK;
            s_sum[c][(1 << l) - 1 + p][k] = s_sum[c][(2 << l) - 1 + 2 * p][k] + s_sum[c][(2 << l) - 1 + 2 * p + 1][k];
        }
        __syncthreads();
    }
    for (int i = tid; i < (cmax + 1) * NODES; i += NT) {
        const int c = i / NODES, node = i - c * NODES, o = LPC && c > MAXO ? c - MAXO : c;
        int l = 0;
        while ((2 << l) - 1 <= node) ++l;
        const int p = node - ((1 << l) - 1);
        if (l > pmax || (m >> l) <= o || !candidate(c)) continue;
        const unsigned long long count = (unsigned long long)((m >> l) - (p == 0 ? o : 0));
        unsigned long long best = count + s_sum[c][node][0];
        int kb = 0;
        for (int k = 1; k < NK; ++k) {
            const unsigned long long v = count * (unsigned long long)(k + 1) + s_sum[c][node][k];
            if (v < best) { best = v; kb = k; }                            // strictly: the lowest k of equals stays
        }
        s_bits[c][node] = 4u + (best < NODE_CAP ? (unsigned)best : NODE_CAP);
        s_k[c][node] = (unsigned char)kb;
    }
    __syncthreads();
    if (tid == 0) {
        unsigned best = 0xFFFFFFFFu;
        int bc = 0, bpo = 0;
        for (int c = 0; c <= cmax; ++c) {
            if (!candidate(c)) continue;
            const int o = LPC && c > MAXO ? c - MAXO : c;
            for (int po = 0; po <= pmax; ++po) {
                if ((m >> po) <= o) continue;
                unsigned bits = head_bits(LPC && c > MAXO, o);
                for (int p = 0; p < (1 << po); ++p) bits += s_bits[c][(1 << po) - 1 + p];
                if (bits < best) { best = bits; bc = c; bpo = po; }       // strictly: Fixed before LPC, the lower order, then the lower po of equals stays
            }
        }
        int kind = LPC && bc > MAXO ? KIND_LPC : KIND_FIXED, bo = LPC && bc > MAXO ? bc - MAXO : bc;
        unsigned klo = 0, khi = 0;
        if (!s_differs) { kind = KIND_CONSTANT; best = 24; bo = bpo = 0; }
        else if (8u + 16u * (unsigned)m < best) { kind = KIND_VERBATIM; best = 8u + 16u * (unsigned)m; bo = bpo = 0; }
        else
            for (int p = 0; p < (1 << bpo); ++p) {
                const unsigned k = s_k[bc][(1 << bpo) - 1 + p];
                if (p < 8) klo |= k << (4 * p); else khi |= k << (4 * (p - 8));
            }
        int* q = rec + REC * frame;
        q[0] = header_bytes(m, rate, number) + (int)((best + 7) / 8) + 2;
        q[1] = kind | (bo << 8) | (bpo << 16);
        q[2] = (int)klo;
        q[3] = (int)khi;
        if constexpr (LPC) {
            int* lq = lrec + LREC * frame;
            lq[0] = kind == KIND_LPC ? s_shift[bo - 1] : 0;
            for (int j = 0; j < MAXL; ++j) lq[1 + j] = kind == KIND_LPC && j < bo ? s_q[bo - 1][j] : 0;
        }
    }
}

// the frames' offsets (exclusive sum of their sizes) and info: (R + 1) x 3 {offset of the row's first frame, smallest, largest frame}, row R
// = {total, 0, 0}.  One workgroup: a thread sums a run of frames, thread 0 scans the runs
__global__ __launch_bounds__(NT) void flac_scan_kernel(const long long* __restrict__ fbase, int R, long long n_frames, const int* __restrict__ rec,
                                                       long long* __restrict__ off, long long* __restrict__ info) {
    __shared__ long long s_sum[NT];
    __shared__ long long s_total;
    const int tid = threadIdx.x;
    long long F = fbase[R];
    if (F > n_frames) F = n_frames;
    const long long per = (F + NT - 1) / NT;
    const long long lo = tid * per < F ? tid * per : F, hi = lo + per < F ? lo + per : F;
    long long sum = 0;
    for (long long f = lo; f < hi; ++f) sum += rec[REC * f];
    s_sum[tid] = sum;
    __syncthreads();
    if (tid == 0) {
        long long run = 0;
        for (int t = 0; t < NT; ++t) { const long long v = s_sum[t]; s_sum[t] = run; run += v; }
        s_total = run;
    }
    __syncthreads();
    long long at = s_sum[tid];
    for (long long f = lo; f < hi; ++f) { off[f] = at; at += rec[REC * f]; }
    __syncthreads();                                                       // off[] of the other threads is read below
    for (int r = tid; r <= R; r += NT) {
        long long* q = info + 3 * (long long)r;
        if (r == R) { q[0] = s_total; q[1] = 0; q[2] = 0; continue; }
        long long f0 = fbase[r], f1 = fbase[r + 1];
        if (f1 > F) f1 = F;
        long long lo_b = 0, hi_b = 0;
        for (long long f = f0; f < f1; ++f) {
            const long long b = rec[REC * f];
            if (f == f0 || b < lo_b) lo_b = b;
            if (f == f0 || b > hi_b) hi_b = b;
        }
        q[0] = f0 < F ? off[f0] : s_total;
        q[1] = lo_b;
        q[2] = hi_b;
    }
}

// n <= 32 bits of v, most significant first, at bit position pos of the image; nothing at or past bit ``limit``.  The analysis and this
// pass compute the same lengths, so the limit never bites; if a record and the samples ever disagreed, the dropped bits would give a
// frame that fails its CRC in a decoder, not a write past the LDS image
__device__ __forceinline__ void put_bits(unsigned* img, unsigned limit, unsigned pos, int n, unsigned v) {
    if (pos + (unsigned)n > limit) return;
    const unsigned long long w = (unsigned long long)v << (64 - n - (int)(pos & 31));
    const unsigned hi = (unsigned)(w >> 32), lo = (unsigned)w;
    if (hi) atomicOr(&img[pos >> 5], hi);
    if (lo) atomicOr(&img[(pos >> 5) + 1], lo);
}

__device__ __forceinline__ unsigned image_byte(const unsigned* img, int j) { return (img[j >> 2] >> (24 - 8 * (j & 3))) & 0xFF; }

// a * b mod P in GF(2)[x], P = x^16 + x^15 + x^2 + 1 (CRC-16, polynomial 0x8005)
__device__ __forceinline__ unsigned mulmod16(unsigned a, unsigned b) {
    unsigned r = 0;
    for (int i = 15; i >= 0; --i) {
        r = (r & 0x8000) ? ((r << 1) ^ 0x8005) & 0xFFFF : (r << 1);
        if ((b >> i) & 1) r ^= a;
    }
    return r;
}

constexpr unsigned x_power_mod(int e) {
    unsigned r = 1;
    for (int i = 0; i < e; ++i) r = (r & 0x8000) ? ((r << 1) ^ 0x8005) & 0xFFFF : (r << 1);
    return r;
}
constexpr unsigned X256 = x_power_mod(256);                                // x^(8 * 32) mod P: one 32-byte piece further from the end

template <bool LPC>
__global__ __launch_bounds__(NT) void flac_pack_kernel(const int16_t* __restrict__ x, long long n_x, const long long* __restrict__ rows, int rate,
                                                       const long long* __restrict__ fbase, long long n_frames, const long long* __restrict__ off,
                                                       const int* __restrict__ rec, uint8_t* __restrict__ y, long long n_y,
                                                       const int* __restrict__ lrec) {
    __shared__ int s_x[FB + 2 * MAXO];
    __shared__ unsigned s_img[IMG_WORDS];
    __shared__ unsigned s_scan[NT];
    __shared__ unsigned s_crc;
    long long frame, src, number;
    int m;
    if (!my_frame(rows, fbase, n_x, frame, src, m, number) || frame >= n_frames) return;
    const int tid = threadIdx.x;
    const int* q = rec + REC * frame;
    const int bytes = q[0], kind = q[1] & 0xFF, o = (q[1] >> 8) & 0xFF, po = (q[1] >> 16) & 0xFF;
    const unsigned klo = (unsigned)q[2], khi = (unsigned)q[3];
    const long long at = off[frame];
    const int hb = header_bytes(m, rate, number);
    const bool lpc = LPC && kind == KIND_LPC, coded = kind == KIND_FIXED || lpc;      // coded: warm-up samples and Rice partitions
    if (bytes < hb + 3 || bytes > HDR_MAX + 1 + 2 * m + 2 || at < 0 || at > n_y - bytes || kind > (LPC ? KIND_LPC : KIND_FIXED) ||
        o > (lpc ? MAXL : MAXO) || po > MAXPO || (coded && (o > m - 1 || m % (1 << po) || (m >> po) <= o)))
        return;                                                            // uniform: a record the analysis cannot have written
    int shift = 0, coef[MAXL];
    if constexpr (LPC) {
        const int* lq = lrec + LREC * frame;
        shift = lq[0];
#pragma unroll
        for (int j = 0; j < MAXL; ++j) coef[j] = lq[1 + j];
        if (lpc && (o < 1 || shift < 0 || shift > 15)) return;             // uniform, as above
    }
    const unsigned head = head_bits(lpc, o) - 6;                           // the subframe's bits in front of the partition order
    load_frame(s_x, x, src, m);
    for (int i = tid; i < IMG_WORDS; i += NT) s_img[i] = 0;
    if (tid == 0) s_crc = 0;
    __syncthreads();
    const int* s = s_x + MAXO;
    const unsigned limit = 8u * (unsigned)(bytes - 2), sub = 8u * (unsigned)hb;
    const int i0 = tid * SPT, i1 = i0 + SPT < m ? i0 + SPT : m;
    if (tid == 0) {
        unsigned char h[HDR_MAX + 1];
        const int n = frame_header(h, m, rate, number);
        for (int j = 0; j < n; ++j) put_bits(s_img, limit, 8u * (unsigned)j, 8, h[j]);
        if (kind == KIND_CONSTANT) put_bits(s_img, limit, sub + 8, 16, (unsigned)s[0] & 0xFFFF);          // subframe header 0 000000 0
        else if (kind == KIND_VERBATIM) put_bits(s_img, limit, sub, 8, 0x02);
        else {
            put_bits(s_img, limit, sub, 8, lpc ? (unsigned)(32 | (o - 1)) << 1 : (unsigned)(8 | o) << 1);
            put_bits(s_img, limit, sub + head, 6, (unsigned)po);                                           // coding method 00, partition order
            if constexpr (LPC) {
                if (lpc) {                                                                                 // precision - 1, shift, q1 ... qo
                    put_bits(s_img, limit, sub + 8 + 16u * (unsigned)o, 9, (unsigned)((LPREC - 1) << 5 | shift));
#pragma unroll
                    for (int j = 0; j < MAXL; ++j)
                        if (j < o) put_bits(s_img, limit, sub + 8 + 16u * (unsigned)o + 9 + (unsigned)(LPREC * j), LPREC, (unsigned)coef[j] & ((1u << LPREC) - 1));
                }
            }
        }
    }
    if (kind == KIND_VERBATIM) {
        for (int i = i0; i < i1; ++i) put_bits(s_img, limit, sub + 8 + 16u * (unsigned)i, 16, (unsigned)s[i] & 0xFFFF);
    } else if (coded) {
        const int ps = m >> po;
        unsigned total = 0;
        if (i0 < m) {
            int p = i0 / ps, next = (p + 1) * ps;
            for (int i = i0; i < i1; ++i) {
                if (i == next) { ++p; next += ps; }
                if (i < o) continue;
                const unsigned k = ((p < 8 ? klo >> (4 * p) : khi >> (4 * (p - 8))) & 15u);
                total += ((lpc ? zigzag_lpc(s, i, o, coef, shift) : zigzag_residual(s, i, o)) >> k) + 1 + k + (i == (p == 0 ? o : p * ps) ? 4u : 0u);
            }
        }
        s_scan[tid] = total;
        __syncthreads();
        for (int d = 1; d < NT; d <<= 1) {                                 // inclusive sum over the workgroup
            const unsigned v = tid >= d ? s_scan[tid - d] : 0;
            __syncthreads();
            s_scan[tid] += v;
            __syncthreads();
        }
        if (i0 < m) {
            unsigned pos = sub + head + 6 + s_scan[tid] - total;
            int p = i0 / ps, next = (p + 1) * ps;
            for (int i = i0; i < i1; ++i) {
                if (i == next) { ++p; next += ps; }
                if (i < o) { put_bits(s_img, limit, sub + 8 + 16u * (unsigned)i, 16, (unsigned)s[i] & 0xFFFF); continue; }      // warm-up
                const unsigned k = ((p < 8 ? klo >> (4 * p) : khi >> (4 * (p - 8))) & 15u);
                if (i == (p == 0 ? o : p * ps)) { put_bits(s_img, limit, pos, 4, k); pos += 4; }
                const unsigned u = lpc ? zigzag_lpc(s, i, o, coef, shift) : zigzag_residual(s, i, o), zeros = u >> k;
                put_bits(s_img, limit, pos + zeros, (int)k + 1, (1u << k) | (u & ((1u << k) - 1)));
                pos += zeros + 1 + k;
            }
        }
    }
    __syncthreads();
    const int L = bytes - 2, pieces = (L + 31) / 32;
    unsigned mine = 0;
    for (int t = tid; t < pieces; t += NT) {
        const int hi = L - 32 * t, lo = hi - 32 > 0 ? hi - 32 : 0;
        unsigned c = 0;
        for (int j = lo; j < hi; ++j) {
            c ^= image_byte(s_img, j) << 8;
            for (int b = 0; b < 8; ++b) c = (c & 0x8000) ? ((c << 1) ^ 0x8005) & 0xFFFF : (c << 1);
        }
        unsigned f = 1, base = X256;
        for (int e = t; e; e >>= 1) {
            if (e & 1) f = mulmod16(f, base);
            base = mulmod16(base, base);
        }
        mine ^= mulmod16(c, f);
    }
    if (mine) atomicXor(&s_crc, mine);
    __syncthreads();
    if (tid == 0) put_bits(s_img, 8u * (unsigned)bytes, 8u * (unsigned)L, 16, s_crc);
    __syncthreads();
    for (int j = tid; j < bytes; j += NT) y[at + j] = (uint8_t)image_byte(s_img, j);
}

}  // namespace

// N16: Levinson-Durbin and the quantisation of the coefficients: the one place with floating point in this file.  Plain operators under
// contract(off), so that every written operation is one float64 operation rounded to nearest, as in the mirror's Python floats: the
// __dmul_rn family is written as plain operators in the headers as well and could still be contracted into fused multiply-adds from
// there.  One thread runs it, a few hundred dependent operations.
#pragma clang fp contract(off)
namespace {

__device__ void lpc_quantise(const unsigned long long* R, int lags, int* shift, int (*q)[MAXL]) {
    double Rf[MAXL + 1], a[MAXL + 1], nw[MAXL + 1];
    for (int l = 0; l <= MAXL; ++l) Rf[l] = l <= lags ? (double)(long long)R[l] : 0.0;
    double err = Rf[0];
    for (int p = 1; p <= MAXL; ++p) {
        if (p > lags) break;
        double acc = Rf[p];
        for (int j = 1; j < p; ++j) acc = acc - a[j] * Rf[p - j];
        const double k = acc / err;
        for (int j = 1; j < p; ++j) nw[j] = a[j] - k * a[p - j];
        nw[p] = k;
        for (int j = 1; j <= p; ++j) a[j] = nw[j];
        err = err * (1.0 - k * k);
        if (!(err > 0.0)) break;                                           // this order and the higher ones are no candidates
        double big = 0.0;
        for (int j = 1; j <= p; ++j) big = fmax(big, fabs(a[j]));
        if (big == 0.0) continue;
        int e;
        frexp(big, &e);                                                    // big = f 2^e, 0.5 <= f < 1
        const int sh = LPREC - 1 - e < 15 ? LPREC - 1 - e : 15;
        if (sh < 0) continue;
        double fe = 0.0;
        for (int j = 1; j <= p; ++j) {
            fe = fe + ldexp(a[j], sh);
            double r = floor(fe + 0.5);
            r = r < -(double)(1 << (LPREC - 1)) ? -(double)(1 << (LPREC - 1)) : r > (double)((1 << (LPREC - 1)) - 1) ? (double)((1 << (LPREC - 1)) - 1) : r;
            q[p - 1][j - 1] = (int)r;
            fe = fe - r;
        }
        shift[p - 1] = sh;
    }
}

}  // namespace (floating point)

#ifndef VV_FLAC_HOST_CHECK
unsigned long long vvk_flac_frame_bound(long long m) { return m < 1 || m > FB ? 0ull : (unsigned long long)(HDR_MAX + 1 + 2 * m + 2); }

// scratch: fbase (R + 1) int64 | off total_frames int64 | rec total_frames x REC int32
unsigned long long vvk_pcm_flac_ws_bytes(long long total_frames, int R) {
    const unsigned long long F = (unsigned long long)(total_frames > 0 ? total_frames : 0), r = (unsigned long long)(R > 0 ? R : 0);
    return 8ull * (r + 1) + 8ull * F + 4ull * REC * F;
}

// the same with the LPC record behind it: ... | lrec total_frames x LREC int32
unsigned long long vvk_pcm_flac_lpc_ws_bytes(long long total_frames, int R) {
    return vvk_pcm_flac_ws_bytes(total_frames, R) + 4ull * LREC * (unsigned long long)(total_frames > 0 ? total_frames : 0);
}

// lpc_order 0: N15 (the LPC = false kernels, ws without the LPC record); 1 ... 12: N16
int vvk_pcm_flac(const int16_t* x, long long n_x, const long long* rows, int R, int rate, int lpc_order, long long total_frames, long long max_frames,
                 uint8_t* y, long long n_y, long long* info, void* ws, hipStream_t st, const char** err) {
    if (R < 1 || R > 65535 || n_x < 0 || n_y < 0 || total_frames < 1 || max_frames < 1 || max_frames > total_frames || max_frames >= (1ll << 31)) {
        *err = "pcm_flac: bad sizes (1 <= R <= 65535)";
        return -22;
    }
    if (!x || !rows || !y || !info || !ws) { *err = "pcm_flac: null pointer"; return -22; }
    if (lpc_order < 0 || lpc_order > MAXL) { *err = "pcm_flac: lpc_order 0 ... 12"; return -22; }
    long long* fbase = (long long*)ws;
    long long* off = fbase + (R + 1);
    int* rec = (int*)(off + total_frames);
    const dim3 grid((unsigned)max_frames, (unsigned)R);
    int* lrec = rec + REC * total_frames;
    flac_plan_kernel<<<1, NT, 0, st>>>(rows, R, n_x, fbase);
    if (lpc_order) flac_analyse_kernel<true><<<grid, NT, 0, st>>>(x, n_x, rows, rate, fbase, total_frames, rec, lpc_order, lrec);
    else flac_analyse_kernel<false><<<grid, NT, 0, st>>>(x, n_x, rows, rate, fbase, total_frames, rec, 0, nullptr);
    flac_scan_kernel<<<1, NT, 0, st>>>(fbase, R, total_frames, rec, off, info);
    if (lpc_order) flac_pack_kernel<true><<<grid, NT, 0, st>>>(x, n_x, rows, rate, fbase, total_frames, off, rec, y, n_y, lrec);
    else flac_pack_kernel<false><<<grid, NT, 0, st>>>(x, n_x, rows, rate, fbase, total_frames, off, rec, y, n_y, nullptr);
    hipError_t he = hipGetLastError();
    if (he != hipSuccess) { *err = hipGetErrorString(he); return -5; }
    return 0;
}
#endif
