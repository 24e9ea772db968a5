// N17: FLAC input on the device (RFC 9639) -- 1 ... 8 channels, 8 / 16 / 24 bits, every subframe kind, both residual methods.
// The arithmetic is the specification: core/audio_processor.py (flac_container, _flac_header, _flac_subframe, flac_frame_index,
// flac_decode) runs the same checks in the same order, so the two agree sample for sample on a valid stream and in reason code and byte
// position on a malformed one.  Everything is integer arithmetic.  The frame bytes of R clips lie back to back in ``data`` (each clip
// 4-byte aligned, 8 bytes of padding behind the last); rows R x 8 {byte offset, n_bytes, channels, bits, min block, max block, rate, total}.
//   vv_flac_index
//     scan     : one thread per 4 byte positions.  A position is a CANDIDATE when check_header passes there: sync, reserved codes, the
//                coded number, the optional block-size / rate bytes, CRC-8, agreement with the row.  count per workgroup -> one-workgroup
//                exclusive sum -> write: the candidates' positions in ascending order, the same in every run (no global counter)
//     measure  : one thread per candidate walks the frame without restoring it (subframe headers, partitions, Rice codes), records each
//                subframe's first bit, the frame's end, its block size and a status, and checks the CRC-16 with a table in LDS
//     chain    : one thread per clip walks candidate -> end -> candidate from the clip's first byte, lists the genuine frames with their
//                sample offsets and writes info[r] = {status, byte of the first problem (from the clip's first), frames, samples}
//   vv_flac_decode (after the host has read info and laid out the PCM)
//     restore  : one thread per (genuine frame, channel) from the recorded bit: 64-bit sums, range check, an int32 plane
//     verdict  : one thread per clip: the first frame that failed the range check -> info2[r] = {status, byte}
//     interleave: one thread per sample: stereo decorrelation, width conversion, byte stores into the layout vv_ingest_pcm reads
// HOSTILE BYTES: the bit reader (Bits) never reads at or past its limit = min(clip end, frame start + frame bound): a read across it gives
// zeros and sets ``over``.  Every loop is bounded by a field check_row validated (block size, channels) or by the bits that remain (a
// unary run ends at the limit; every Rice loop leaves when ``over`` is set).  Every index taken from the workspace is range-checked
// before it is used.  No atomics on global memory, nothing depends on the execution order, every output byte is written once.
#ifndef VV_FLAC_HOST_CHECK            // tools/flac_decode_host_check.cpp compiles the kernels below for the host, with its own stand-ins
#include "vv_common.h"
#include "vv_kernels.h"
#endif

namespace {

constexpr int NT = 256;                       // threads of the scan kernels
constexpr int PER = 4;                        // byte positions per scan thread
constexpr int SCAN = NT * PER;                // positions per scan workgroup
constexpr int MT = 64;                        // threads of the per-frame, per-clip and per-sample kernels
constexpr int MAXCH = 8;
constexpr int REC = 4;                        // ints per candidate {end byte, block size, status, assignment | header bytes << 8}
constexpr long long MAX_CLIP = 1ll << 26;     // VV_FLAC_MAX_CLIP
constexpr long long MAX_BYTES = (1ll << 31) - 64;

enum { ST_OK = 0, ST_BAD_HEADER, ST_CRC8, ST_CRC16, ST_RESERVED, ST_PARTITION, ST_RANGE, ST_OVERRUN, ST_CHAIN, ST_TOO_LONG, ST_CLIP_TOO_LONG };

struct Row { long long off, n, total; int ch, bits, minb, maxb, rate; };

// a row the kernels may follow.  The host has checked it; checked all the same
__device__ __forceinline__ bool load_row(const long long* __restrict__ rows, int r, long long n_bytes, Row& q) {
    const long long* p = rows + 8 * (long long)r;
    q.off = p[0]; q.n = p[1]; q.total = p[7];
    if (q.off < 0 || (q.off & 3) || q.n < 0 || q.n > n_bytes - 8 || q.off > n_bytes - 8 - q.n) return false;
    if (p[2] < 1 || p[2] > MAXCH || (p[3] != 8 && p[3] != 16 && p[3] != 24) || p[5] < 16 || p[5] > 65535 || p[4] < 0 || p[4] > p[5] || p[6] < 1 ||
        p[6] > 1048575 || q.total < 0 || q.total > MAX_CLIP)
        return false;
    q.ch = (int)p[2]; q.bits = (int)p[3]; q.minb = (int)p[4]; q.maxb = (int)p[5]; q.rate = (int)p[6];
    return true;
}

// the row that holds byte ``pos`` (rows ascending by offset): -1 = none
__device__ int find_row(const long long* __restrict__ rows, int R, long long n_bytes, long long pos, Row& q) {
    int lo = 0, hi = R;                                                    // the last row with off <= pos
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (rows[8 * (long long)mid] <= pos) lo = mid; else hi = mid;
    }
    if (!load_row(rows, lo, n_bytes, q) || pos < q.off || pos >= q.off + q.n) return -1;
    return lo;
}

__host__ __device__ __forceinline__ long long frame_bound(int bs, int ch, int bits) {
    return 2ll * (16 + (long long)ch * (2 + ((long long)bs * (bits + 1) + 7) / 8) + 2) + 64;
}

struct Head { int status, hlen, bs, assign; };

// the frame header expected at byte p of a clip that ends at ``end``: _flac_header of the mirror, check for check
__device__ Head check_header(const uint8_t* __restrict__ d, long long p, long long end, const Row& q, int blocking) {
    Head h{ST_OK, 0, 0, 0};
    if (p + 4 > end) { h.status = ST_OVERRUN; return h; }
    const unsigned b0 = d[p], b1 = d[p + 1], b2 = d[p + 2], b3 = d[p + 3];
    if (b0 != 0xFF || (b1 & 0xFC) != 0xF8) { h.status = ST_BAD_HEADER; return h; }
    const int bsc = (int)(b2 >> 4), rc = (int)(b2 & 15), cc = (int)(b3 >> 4), dc = (int)((b3 >> 1) & 7);
    if ((b1 & 2) || bsc == 0 || rc == 15 || cc > 10 || dc == 3 || (b3 & 1)) { h.status = ST_RESERVED; return h; }
    long long at = p + 4;
    if (at + 1 > end) { h.status = ST_OVERRUN; return h; }
    const unsigned lead = d[at];
    int n = 0;
    while (n < 8 && (lead & (0x80u >> n))) ++n;
    if (n == 1 || n == 8) { h.status = ST_BAD_HEADER; return h; }
    if (n < 1) n = 1;
    if (at + n > end) { h.status = ST_OVERRUN; return h; }
    for (int i = 1; i < n; ++i)
        if ((d[at + i] & 0xC0) != 0x80) { h.status = ST_BAD_HEADER; return h; }
    at += n;
    int extra = bsc == 6 ? 1 : bsc == 7 ? 2 : 0;
    if (at + extra > end) { h.status = ST_OVERRUN; return h; }
    int v = 0;
    for (int i = 0; i < extra; ++i) v = (v << 8) | d[at + i];
    at += extra;
    if (bsc == 7 && v == 65535) { h.status = ST_RESERVED; return h; }
    const int bs = bsc == 1 ? 192 : bsc <= 5 ? 576 << (bsc - 2) : bsc <= 7 ? v + 1 : 256 << (bsc - 8);
    extra = rc == 12 ? 1 : rc == 13 || rc == 14 ? 2 : 0;
    if (at + extra > end) { h.status = ST_OVERRUN; return h; }
    v = 0;
    for (int i = 0; i < extra; ++i) v = (v << 8) | d[at + i];
    at += extra;
    int rate = q.rate;
    switch (rc) {
        case 1: rate = 88200; break;   case 2: rate = 176400; break;  case 3: rate = 192000; break;  case 4: rate = 8000; break;
        case 5: rate = 16000; break;   case 6: rate = 22050; break;   case 7: rate = 24000; break;   case 8: rate = 32000; break;
        case 9: rate = 44100; break;   case 10: rate = 48000; break;  case 11: rate = 96000; break;  case 12: rate = v * 1000; break;
        case 13: rate = v; break;      case 14: rate = v * 10; break;
    }
    if (at + 1 > end) { h.status = ST_OVERRUN; return h; }
    unsigned c = 0;
    for (long long i = p; i < at; ++i) {                                   // at - p <= 15
        c ^= d[i];
        for (int b = 0; b < 8; ++b) c = (c & 0x80) ? ((c << 1) ^ 0x07) & 0xFF : (c << 1) & 0xFF;
    }
    if (c != d[at]) { h.status = ST_CRC8; return h; }
    const int depth = dc == 1 ? 8 : dc == 2 ? 12 : dc == 4 ? 16 : dc == 5 ? 20 : dc == 6 ? 24 : dc == 7 ? 32 : q.bits;
    if ((cc < 8 ? cc + 1 : 2) != q.ch || depth != q.bits || rate != q.rate || (int)(b1 & 1) != blocking || bs > q.maxb) {
        h.status = ST_BAD_HEADER;
        return h;
    }
    h.hlen = (int)(at + 1 - p); h.bs = bs; h.assign = cc;
    return h;
}

// is byte ``pos`` a candidate?  The cheap test first: two bytes decide for nearly every position
__device__ __forceinline__ bool is_candidate(const uint8_t* __restrict__ d, long long n_bytes, const long long* __restrict__ rows, int R, long long pos) {
    if (pos + 1 >= n_bytes || d[pos] != 0xFF || (d[pos + 1] & 0xFC) != 0xF8) return false;
    Row q;
    if (find_row(rows, R, n_bytes, pos, q) < 0) return false;
    const int blocking = q.n >= 2 ? d[q.off + 1] & 1 : 0;
    return check_header(d, pos, q.off + q.n, q, blocking).status == ST_OK;
}

// candidates of each workgroup's SCAN positions: counts[b]
__global__ __launch_bounds__(NT) void flac_scan_count_kernel(const uint8_t* __restrict__ d, long long n_bytes, const long long* __restrict__ rows, int R,
                                                             int* __restrict__ counts) {
    __shared__ int s_n[NT];
    const int tid = threadIdx.x;
    const long long p0 = (long long)blockIdx.x * SCAN + (long long)tid * PER;
    int n = 0;
    for (int j = 0; j < PER; ++j) n += p0 + j < n_bytes && is_candidate(d, n_bytes, rows, R, p0 + j) ? 1 : 0;
    s_n[tid] = n;
    __syncthreads();
    for (int s = NT / 2; s > 0; s >>= 1) {
        if (tid < s) s_n[tid] += s_n[tid + s];
        __syncthreads();
    }
    if (tid == 0) counts[blockIdx.x] = s_n[0];
}

// counts[0 ... nb) -> their exclusive sum, counts[nb] = the total.  One workgroup: a thread sums a run, thread 0 scans the runs
__global__ __launch_bounds__(NT) void flac_scan_offsets_kernel(int* __restrict__ counts, int nb) {
    __shared__ int s_sum[NT];
    const int tid = threadIdx.x, per = (nb + NT - 1) / NT;
    const int lo = tid * per < nb ? tid * per : nb, hi = lo + per < nb ? lo + per : nb;
    int sum = 0;
    for (int b = lo; b < hi; ++b) sum += counts[b];
    s_sum[tid] = sum;
    __syncthreads();
    if (tid == 0) {
        int run = 0;
        for (int t = 0; t < NT; ++t) { const int v = s_sum[t]; s_sum[t] = run; run += v; }
        counts[nb] = run;
    }
    __syncthreads();
    int at = s_sum[tid];
    for (int b = lo; b < hi; ++b) { const int v = counts[b]; counts[b] = at; at += v; }
}

// the candidates' positions in ascending order: cand[counts[b] + rank inside the workgroup]
__global__ __launch_bounds__(NT) void flac_scan_write_kernel(const uint8_t* __restrict__ d, long long n_bytes, const long long* __restrict__ rows, int R,
                                                             const int* __restrict__ counts, int* __restrict__ cand, long long cap) {
    __shared__ int s_n[NT];
    const int tid = threadIdx.x;
    const long long p0 = (long long)blockIdx.x * SCAN + (long long)tid * PER;
    bool is[PER];
    int n = 0;
    for (int j = 0; j < PER; ++j) { is[j] = p0 + j < n_bytes && is_candidate(d, n_bytes, rows, R, p0 + j); n += is[j] ? 1 : 0; }
    s_n[tid] = n;
    __syncthreads();
    for (int s = 1; s < NT; s <<= 1) {                                     // inclusive sum over the workgroup
        const int v = tid >= s ? s_n[tid - s] : 0;
        __syncthreads();
        s_n[tid] += v;
        __syncthreads();
    }
    long long at = (long long)counts[blockIdx.x] + s_n[tid] - n;
    for (int j = 0; j < PER; ++j)
        if (is[j]) {
            if (at >= 0 && at < cap) cand[at] = (int)(p0 + j);
            ++at;
        }
}

// ---- the bit reader both sides share: nothing at or past ``limit`` (in bits from the start of ``d``) is read
struct Bits {
    const uint8_t* d;
    unsigned long long pos, limit;
    bool over;
};

// the next 32 bits (pos < limit), those at or past the limit as zeros.  Two aligned 4-byte reads: the second one ends < 8 bytes behind
// the byte that holds ``pos``, inside the padding the rows guarantee
__device__ __forceinline__ unsigned peek32(const Bits& b) {
    const unsigned* w = (const unsigned*)b.d + (b.pos >> 5);
    const unsigned long long v = ((unsigned long long)__builtin_bswap32(w[0]) << 32) | __builtin_bswap32(w[1]);
    unsigned r = (unsigned)((v << (b.pos & 31)) >> 32);
    const unsigned long long avail = b.limit - b.pos;
    if (avail < 32) r &= ~0u << (32 - (int)avail);
    return r;
}

__device__ __forceinline__ unsigned take(Bits& b, int n) {                // n <= 32
    const unsigned long long pos = b.pos;
    b.pos = pos + (unsigned)n;
    if (pos + (unsigned)n > b.limit) { b.over = true; return 0; }
    if (n == 0) return 0;
    Bits at = b;
    at.pos = pos;
    return peek32(at) >> (32 - n);
}

__device__ __forceinline__ long long take_signed(Bits& b, int n) {
    const unsigned v = take(b, n);
    return n == 0 ? 0 : (long long)((int)(v << (32 - n)) >> (32 - n));
}

__device__ __forceinline__ void skip(Bits& b, unsigned long long n) {
    b.pos += n;
    if (b.pos > b.limit) b.over = true;
}

// zeros in front of the next one bit; at most (limit - pos) / 32 + 1 rounds
__device__ __forceinline__ unsigned long long unary(Bits& b) {
    unsigned long long n = 0;
    while (true) {
        if (b.pos >= b.limit) { b.over = true; return n; }
        const unsigned long long left = b.limit - b.pos;
        const int avail = left < 32 ? (int)left : 32;
        const unsigned v = peek32(b);
        if (v) {
            const int lz = __builtin_clz(v);                               // < avail: the bits past the limit are zeros
            b.pos += (unsigned)lz + 1;
            return n + (unsigned)lz;
        }
        n += (unsigned)avail;
        b.pos += (unsigned)avail;
    }
}

__device__ __forceinline__ int depth_of(int bits, int assign, int c) {
    return bits + (((assign == 8 && c == 1) || (assign == 9 && c == 0) || (assign == 10 && c == 1)) ? 1 : 0);
}

// one subframe at the reader's position: _flac_subframe of the mirror, check for check.  RESTORE = false walks it; true restores it
// into out[0 ... bs) (the samples before the wasted bits come back are kept there for the predictor; shifted at the end)
template <bool RESTORE>
__device__ int subframe(Bits& r, int bs, int depth, int* out) {
    const unsigned h = take(r, 8);
    if (r.over) return ST_OVERRUN;
    if (h & 0x80) return ST_RESERVED;
    const int t = (int)((h >> 1) & 63);
    long long w = 0;
    if (h & 1) {
        w = (long long)unary(r) + 1;
        if (r.over) return ST_OVERRUN;
    }
    if (w >= depth) return ST_RESERVED;
    const int de = depth - (int)w;
    const long long lo = -(1ll << (de - 1)), hi = (1ll << (de - 1)) - 1;
    if (t == 0) {
        if (RESTORE) {
            const int v = (int)take_signed(r, de);
            for (int i = 0; i < bs; ++i) out[i] = v;
        } else skip(r, (unsigned)de);
    } else if (t == 1) {
        if (RESTORE) {
            for (int i = 0; i < bs; ++i) out[i] = (int)take_signed(r, de);
        } else skip(r, (unsigned long long)de * (unsigned)bs);
    } else if ((t >= 8 && t <= 12) || t >= 32) {
        const bool lpc = t >= 32;
        const int o = lpc ? (t & 31) + 1 : t - 8;
        if (o > bs) return ST_PARTITION;
        if (RESTORE) {
            for (int i = 0; i < o; ++i) out[i] = (int)take_signed(r, de);
        } else skip(r, (unsigned long long)o * (unsigned)de);
        if (r.over) return ST_OVERRUN;
        int coef[32], shift = 0;
        if (lpc) {
            const unsigned pq = take(r, 9);
            if (r.over) return ST_OVERRUN;
            const int prec = (int)(pq >> 5) + 1;
            shift = (int)(pq & 15);
            if (prec == 16 || (pq & 16)) return ST_RESERVED;
            if (RESTORE) {
                for (int j = 0; j < o; ++j) coef[j] = (int)take_signed(r, prec);
            } else skip(r, (unsigned long long)o * (unsigned)prec);
            if (r.over) return ST_OVERRUN;
        } else if (RESTORE) {
            const int fixed[5][4] = {{0, 0, 0, 0}, {1, 0, 0, 0}, {2, -1, 0, 0}, {3, -3, 1, 0}, {4, -6, 4, -1}};
            for (int j = 0; j < o; ++j) coef[j] = fixed[o][j];
        }
        const unsigned m = take(r, 6);
        if (r.over) return ST_OVERRUN;
        const int method = (int)(m >> 4), po = (int)(m & 15);
        if (method > 1) return ST_RESERVED;
        if ((bs & ((1 << po) - 1)) || (bs >> po) < o) return ST_PARTITION;
        const int pb = 4 + method;
        int i = o;
        for (int part = 0; part < (1 << po); ++part) {                     // 2^po <= bs: bs is a multiple of it
            int n = (bs >> po) - (part == 0 ? o : 0);
            const int k = (int)take(r, pb);
            if (r.over) return ST_OVERRUN;
            int raw = -1;
            if (k == (1 << pb) - 1) {
                raw = (int)take(r, 5);
                if (r.over) return ST_OVERRUN;
                if (!RESTORE) { skip(r, (unsigned long long)n * (unsigned)raw); n = 0; }
            }
            for (int s = 0; s < n; ++s) {
                long long res = 0;
                if (raw >= 0) res = take_signed(r, raw);
                else {
                    unsigned long long u = unary(r);
                    if (RESTORE) {
                        u = (u << k) | take(r, k);                         // u < 2^26 (the frame bound) and k <= 30: no overflow
                        res = (long long)(u >> 1) ^ -(long long)(u & 1);
                    } else skip(r, (unsigned)k);
                }
                if (r.over) return ST_OVERRUN;
                if (RESTORE) {
                    long long pred = 0;
                    for (int j = 0; j < o; ++j) pred += (long long)coef[j] * out[i - 1 - j];
                    const long long v = (pred >> shift) + res;
                    if (v < lo || v > hi) return ST_RANGE;
                    out[i++] = (int)v;
                }
            }
            if (r.over) return ST_OVERRUN;
        }
    } else return ST_RESERVED;
    if (r.over) return ST_OVERRUN;
    if (RESTORE && w)
        for (int i = 0; i < bs; ++i) out[i] = (int)((unsigned)out[i] << w);
    return ST_OK;
}

// one thread per candidate: rec[i] = {end, block size, status, assignment | header bytes << 8}, sub[i][c] = the subframes' first bits
__global__ __launch_bounds__(MT) void flac_measure_kernel(const uint8_t* __restrict__ d, long long n_bytes, const long long* __restrict__ rows, int R,
                                                          const int* __restrict__ counts, int nb, const int* __restrict__ cand, long long cap,
                                                          int* __restrict__ rec, unsigned* __restrict__ sub) {
    __shared__ unsigned short s_crc[256];
    for (int v = threadIdx.x; v < 256; v += MT) {
        unsigned c = (unsigned)v << 8;
        for (int b = 0; b < 8; ++b) c = (c & 0x8000) ? ((c << 1) ^ 0x8005) & 0xFFFF : (c << 1) & 0xFFFF;
        s_crc[v] = (unsigned short)c;
    }
    __syncthreads();
    const long long i = (long long)blockIdx.x * MT + threadIdx.x;
    long long total = counts[nb];
    if (total > cap) total = cap;
    if (i >= total) return;
    int* q = rec + REC * i;
    q[0] = 0; q[1] = 0; q[2] = ST_BAD_HEADER; q[3] = 0;
    const long long p = cand[i];
    Row row;
    if (p < 0 || p >= n_bytes || find_row(rows, R, n_bytes, p, row) < 0) return;
    const long long end = row.off + row.n;
    const Head h = check_header(d, p, end, row, row.n >= 2 ? d[row.off + 1] & 1 : 0);
    if (h.status) { q[2] = h.status; return; }
    q[1] = h.bs;
    q[3] = h.assign | (h.hlen << 8);
    const long long bound = p + frame_bound(h.bs, row.ch, row.bits);
    const int over = bound <= end ? ST_TOO_LONG : ST_OVERRUN;
    Bits r{d, 8ull * (unsigned long long)(p + h.hlen), 8ull * (unsigned long long)(bound < end ? bound : end), false};
    for (int c = 0; c < row.ch; ++c) {
        sub[MAXCH * i + c] = (unsigned)(r.pos - 8ull * (unsigned long long)p);
        const int st = subframe<false>(r, h.bs, depth_of(row.bits, h.assign, c), nullptr);
        if (st) { q[2] = st == ST_OVERRUN ? over : st; return; }
    }
    const unsigned pad = take(r, (int)((8 - (r.pos & 7)) & 7));
    if (r.over) { q[2] = over; return; }
    if (pad) { q[2] = ST_RESERVED; return; }
    const unsigned crc = take(r, 16);
    if (r.over) { q[2] = over; return; }
    const long long e = (long long)(r.pos >> 3);
    unsigned c = 0;
    for (long long j = p; j < e - 2; ++j) c = ((c << 8) & 0xFFFF) ^ s_crc[(c >> 8) ^ d[j]];
    q[0] = (int)e;
    q[2] = c == crc ? ST_OK : ST_CRC16;
}

__device__ __forceinline__ int lower_bound(const int* __restrict__ a, int n, long long v) {
    int lo = 0, hi = n;
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (a[mid] < v) lo = mid + 1; else hi = mid;
    }
    return lo;
}

// one thread per clip: the chain rule.  gen[lo + f] = the candidate that is the clip's frame f, s0[candidate] = its first sample,
// clip[r] = {lo, frames}, info[r] = {status, byte of the first problem from the clip's first byte, frames, samples}
__global__ __launch_bounds__(MT) void flac_chain_kernel(const uint8_t* __restrict__ d, long long n_bytes, const long long* __restrict__ rows, int R,
                                                        const int* __restrict__ counts, int nb, const int* __restrict__ cand, long long cap,
                                                        const int* __restrict__ rec, int* __restrict__ gen, int* __restrict__ s0,
                                                        int* __restrict__ clip, long long* __restrict__ info) {
    const int r = blockIdx.x * MT + threadIdx.x;
    if (r >= R) return;
    long long* out = info + 4 * (long long)r;
    clip[2 * r] = 0; clip[2 * r + 1] = 0;
    Row q;
    if (!load_row(rows, r, n_bytes, q)) { out[0] = ST_BAD_HEADER; out[1] = 0; out[2] = 0; out[3] = 0; return; }
    long long total = counts[nb];
    if (total > cap) total = cap;
    const long long end = q.off + q.n;
    const int lo = lower_bound(cand, (int)total, q.off), hi = lower_bound(cand, (int)total, end);
    const int blocking = q.n >= 2 ? d[q.off + 1] & 1 : 0;
    long long p = q.off, samples = 0;
    int frames = 0, status = ST_OK, i = lo;
    while (!(q.total && samples == q.total)) {                             // every round moves p forward: at most n rounds
        if (p == end) {
            if (q.total) status = ST_CHAIN;
            break;
        }
        while (i < hi && cand[i] < p) ++i;
        if (i >= hi || cand[i] != p) {
            status = check_header(d, p, end, q, blocking).status;
            if (!status) status = ST_BAD_HEADER;
            break;
        }
        const int* f = rec + REC * (long long)i;
        if (f[2]) { status = f[2]; break; }
        const int bs = f[1];
        if (f[0] <= p || f[0] > end || bs < 1 || bs > 65535) { status = ST_BAD_HEADER; break; }
        if (samples + bs > MAX_CLIP) { status = ST_CLIP_TOO_LONG; break; }
        if (q.total && samples + bs > q.total) { status = ST_CHAIN; break; }
        gen[lo + frames] = i;
        s0[i] = (int)samples;
        ++frames;
        samples += bs;
        p = f[0];
    }
    clip[2 * r] = lo; clip[2 * r + 1] = frames;
    out[0] = status; out[1] = status ? p - q.off : 0; out[2] = frames; out[3] = samples;
}

// ---- vv_flac_decode.  lay R x 6 {pcm byte offset, frames, samples, frames in front, plane samples in front, samples in front}
struct Clip { Row q; long long pcm, frames, samples, fbase, pbase, sbase; int lo; };

__device__ bool load_clip(const long long* __restrict__ rows, const long long* __restrict__ lay, int r, long long n_bytes, const int* __restrict__ clip,
                          long long total, long long n_plane, long long n_pcm, Clip& c) {
    if (!load_row(rows, r, n_bytes, c.q)) return false;
    const long long* l = lay + 6 * (long long)r;
    c.pcm = l[0]; c.frames = l[1]; c.samples = l[2]; c.fbase = l[3]; c.pbase = l[4]; c.sbase = l[5];
    c.lo = clip[2 * r];
    const long long width = c.q.bits == 24 ? 4 : c.q.bits / 8;
    if (c.frames < 0 || c.frames != clip[2 * r + 1] || c.lo < 0 || c.lo > total - c.frames || c.samples < 0 || c.samples > MAX_CLIP) return false;
    if (c.fbase < 0 || c.sbase < 0 || c.pbase < 0 || c.pbase > n_plane - c.samples * c.q.ch) return false;
    if (c.pcm < 0 || c.pcm > n_pcm - c.samples * c.q.ch * width) return false;
    return true;
}

// the last row whose field ``col`` of lay is <= v (lay's prefix sums ascend)
__device__ int clip_of(const long long* __restrict__ lay, int R, int col, long long v) {
    int lo = 0, hi = R;
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (lay[6 * (long long)mid + col] <= v) lo = mid; else hi = mid;
    }
    return lo;
}

// the clip's frame f as a candidate: -1 when the workspace does not hold a frame the kernels may follow
__device__ int frame_of(const Clip& c, long long f, const int* __restrict__ gen, const int* __restrict__ cand, const int* __restrict__ rec,
                        const int* __restrict__ s0, long long total) {
    const int i = gen[c.lo + f];
    if (i < 0 || i >= total) return -1;
    const int* q = rec + REC * (long long)i;
    const long long p = cand[i];
    if (q[2] != ST_OK || p < c.q.off || q[0] <= p || q[0] > c.q.off + c.q.n || q[1] < 1 || q[1] > 65535 || s0[i] < 0 || s0[i] > c.samples - q[1]) return -1;
    return i;
}

// one thread per (genuine frame, channel): plane[pbase + s0 ch + c bs + 0 ... bs), fst[8 frame + c] = its status
__global__ __launch_bounds__(MT) void flac_restore_kernel(const uint8_t* __restrict__ d, long long n_bytes, const long long* __restrict__ rows, int R,
                                                          const long long* __restrict__ lay, long long F, int maxch, const int* __restrict__ counts,
                                                          int nb, const int* __restrict__ cand, long long cap, const int* __restrict__ rec,
                                                          const unsigned* __restrict__ sub, const int* __restrict__ gen, const int* __restrict__ s0,
                                                          const int* __restrict__ clip, int* plane, long long n_plane, long long n_pcm,
                                                          int* __restrict__ fst) {
    const long long t = (long long)blockIdx.x * MT + threadIdx.x;
    const long long g = t / maxch;
    const int c = (int)(t - g * maxch);
    if (g >= F) return;
    fst[MAXCH * g + c] = ST_OK;
    long long total = counts[nb];
    if (total > cap) total = cap;
    const int r = clip_of(lay, R, 3, g);
    Clip k;
    if (!load_clip(rows, lay, r, n_bytes, clip, total, n_plane, n_pcm, k) || g < k.fbase || g - k.fbase >= k.frames || c >= k.q.ch) return;
    const int i = frame_of(k, g - k.fbase, gen, cand, rec, s0, total);
    if (i < 0) { fst[MAXCH * g + c] = ST_BAD_HEADER; return; }
    const int* q = rec + REC * (long long)i;
    const int bs = q[1], assign = q[3] & 0xFF;
    const unsigned long long first = 8ull * (unsigned long long)cand[i] + sub[MAXCH * (long long)i + c];
    Bits b{d, first, 8ull * (unsigned long long)q[0], false};
    if (first >= b.limit) { fst[MAXCH * g + c] = ST_BAD_HEADER; return; }
    fst[MAXCH * g + c] = subframe<true>(b, bs, depth_of(k.q.bits, assign, c), plane + k.pbase + (long long)s0[i] * k.q.ch + (long long)c * bs);
}

// one thread per clip: the first frame (then channel) that failed -> info2[r] = {status, its byte from the clip's first byte}
__global__ __launch_bounds__(MT) void flac_verdict_kernel(const long long* __restrict__ rows, int R, long long n_bytes, const long long* __restrict__ lay,
                                                          long long F, const int* __restrict__ counts, int nb, const int* __restrict__ cand,
                                                          long long cap, const int* __restrict__ gen, const int* __restrict__ clip,
                                                          long long n_plane, long long n_pcm, const int* __restrict__ fst, long long* __restrict__ info2) {
    const int r = blockIdx.x * MT + threadIdx.x;
    if (r >= R) return;
    long long* out = info2 + 2 * (long long)r;
    out[0] = ST_OK; out[1] = 0;
    long long total = counts[nb];
    if (total > cap) total = cap;
    Clip k;
    if (!load_clip(rows, lay, r, n_bytes, clip, total, n_plane, n_pcm, k) || k.fbase > F - k.frames) { out[0] = ST_BAD_HEADER; return; }
    for (long long f = 0; f < k.frames; ++f)
        for (int c = 0; c < k.q.ch; ++c) {
            const int st = fst[MAXCH * (k.fbase + f) + c];
            if (st) {
                const int i = gen[k.lo + f];
                out[0] = st;
                out[1] = i >= 0 && i < total ? cand[i] - k.q.off : 0;
                return;
            }
        }
}

// one thread per sample of every clip: channels out of the planes, decorrelation, the width's little-endian bytes
__global__ __launch_bounds__(MT) void flac_interleave_kernel(const long long* __restrict__ rows, int R, long long n_bytes, const long long* __restrict__ lay,
                                                             long long S, const int* __restrict__ counts, int nb, const int* __restrict__ cand,
                                                             long long cap, const int* __restrict__ rec, const int* __restrict__ gen,
                                                             const int* __restrict__ s0, const int* __restrict__ clip, const int* __restrict__ plane,
                                                             long long n_plane, uint8_t* __restrict__ pcm, long long n_pcm) {
    const long long t = (long long)blockIdx.x * MT + threadIdx.x;
    if (t >= S) return;
    long long total = counts[nb];
    if (total > cap) total = cap;
    const int r = clip_of(lay, R, 5, t);
    Clip k;
    if (!load_clip(rows, lay, r, n_bytes, clip, total, n_plane, n_pcm, k)) return;
    const long long s = t - k.sbase;
    if (s < 0 || s >= k.samples || k.frames < 1) return;
    long long lo = 0, hi = k.frames;                                       // the last frame whose first sample is <= s
    while (hi - lo > 1) {
        const long long mid = (lo + hi) >> 1;
        const int im = gen[k.lo + mid];
        if (im >= 0 && im < total && s0[im] <= s) lo = mid; else hi = mid;
    }
    const int i = frame_of(k, lo, gen, cand, rec, s0, total);
    if (i < 0) return;
    const int bs = rec[REC * (long long)i + 1], assign = rec[REC * (long long)i + 3] & 0xFF;
    const long long j = s - s0[i];
    if (j < 0 || j >= bs) return;
    const int* src = plane + k.pbase + (long long)s0[i] * k.q.ch + j;
    int v[MAXCH];
    for (int c = 0; c < MAXCH; ++c) v[c] = c < k.q.ch ? src[(long long)c * bs] : 0;
    if (assign == 8) v[1] = v[0] - v[1];
    else if (assign == 9) v[0] = v[0] + v[1];
    else if (assign == 10) {
        const int mid = (int)(((unsigned)v[0] << 1) | ((unsigned)v[1] & 1u)), side = v[1];
        v[0] = (mid + side) >> 1;
        v[1] = (mid - side) >> 1;
    }
    const int width = k.q.bits == 24 ? 4 : k.q.bits / 8;
    uint8_t* dst = pcm + k.pcm + s * k.q.ch * width;
    for (int c = 0; c < MAXCH; ++c) {
        if (c >= k.q.ch) break;
        const unsigned u = (unsigned)v[c];
        if (width == 1) dst[c] = (uint8_t)u;
        else if (width == 2) { dst[2 * c] = (uint8_t)u; dst[2 * c + 1] = (uint8_t)(u >> 8); }
        else {                                                             // 24 bits: the sign pad first, then the sample's three bytes
            dst[4 * c] = (u & 0x800000u) ? 0xFF : 0x00;
            dst[4 * c + 1] = (uint8_t)u; dst[4 * c + 2] = (uint8_t)(u >> 8); dst[4 * c + 3] = (uint8_t)(u >> 16);
        }
    }
}

// the workspace of vv_flac_index, which vv_flac_decode reads: counts nb + 1 | cand C | rec C x REC | sub C x 8 | gen C | s0 C | clip R x 2
// (all int32).  C = n_bytes / 2 + 1: two candidates are at least two bytes apart (0xFF, then 0xF8 ... 0xFB)
struct Ws { int nb; long long cap; int *counts, *cand, *rec, *gen, *s0, *clip; unsigned* sub; unsigned long long bytes; };

inline Ws ws_layout(void* ws, long long n_bytes, int R) {
    Ws w;
    w.nb = (int)((n_bytes + SCAN - 1) / SCAN);
    w.cap = n_bytes / 2 + 1;
    const unsigned long long C = (unsigned long long)w.cap, o_cand = ((unsigned long long)w.nb + 2) / 2 * 2, o_rec = o_cand + C, o_sub = o_rec + REC * C,
                             o_gen = o_sub + MAXCH * C, o_s0 = o_gen + C, o_clip = o_s0 + C, o_end = o_clip + 2ull * (unsigned long long)R;
    w.bytes = (4 * o_end + 7) / 8 * 8;
    int* p = (int*)ws;
    w.counts = p;
    w.cand = p ? p + o_cand : nullptr;
    w.rec = p ? p + o_rec : nullptr;
    w.sub = p ? (unsigned*)(p + o_sub) : nullptr;
    w.gen = p ? p + o_gen : nullptr;
    w.s0 = p ? p + o_s0 : nullptr;
    w.clip = p ? p + o_clip : nullptr;
    return w;
}

}  // namespace

#ifndef VV_FLAC_HOST_CHECK
unsigned long long vvk_flac_decode_frame_bound(int block, int channels, int bits) {
    return block < 1 || block > 65535 || channels < 1 || channels > MAXCH ? 0ull : (unsigned long long)frame_bound(block, channels, bits);
}

unsigned long long vvk_flac_index_ws_bytes(long long n_bytes, int R) {
    if (n_bytes < 8 || n_bytes > MAX_BYTES || R < 1 || R > 65535) return 0;
    return ws_layout(nullptr, n_bytes, R).bytes;
}

// plane int32 n_plane | fst int32 total_frames x 8
unsigned long long vvk_flac_decode_ws_bytes(long long n_plane, long long total_frames) {
    if (n_plane < 0 || total_frames < 0) return 0;
    return 4ull * (unsigned long long)n_plane + 4ull * MAXCH * (unsigned long long)total_frames + 8;
}

int vvk_flac_index(const uint8_t* data, long long n_bytes, const long long* rows, int R, long long* info, void* ws, hipStream_t st, const char** err) {
    if (R < 1 || R > 65535 || n_bytes < 8 || n_bytes > MAX_BYTES) { *err = "flac_index: bad sizes (1 <= R <= 65535, 8 <= n_bytes < 2^31 - 64)"; return -22; }
    if (!data || !rows || !info || !ws) { *err = "flac_index: null pointer"; return -22; }
    const Ws w = ws_layout(ws, n_bytes, R);
    flac_scan_count_kernel<<<w.nb, NT, 0, st>>>(data, n_bytes, rows, R, w.counts);
    flac_scan_offsets_kernel<<<1, NT, 0, st>>>(w.counts, w.nb);
    flac_scan_write_kernel<<<w.nb, NT, 0, st>>>(data, n_bytes, rows, R, w.counts, w.cand, w.cap);
    flac_measure_kernel<<<(unsigned)((w.cap + MT - 1) / MT), MT, 0, st>>>(data, n_bytes, rows, R, w.counts, w.nb, w.cand, w.cap, w.rec, w.sub);
    flac_chain_kernel<<<(R + MT - 1) / MT, MT, 0, st>>>(data, n_bytes, rows, R, w.counts, w.nb, w.cand, w.cap, w.rec, w.gen, w.s0, w.clip, info);
    hipError_t he = hipGetLastError();
    if (he != hipSuccess) { *err = hipGetErrorString(he); return -5; }
    return 0;
}

int vvk_flac_decode(const uint8_t* data, long long n_bytes, const long long* rows, int R, const long long* lay, long long total_frames,
                    long long total_samples, long long n_plane, int max_channels, void* ws, uint8_t* pcm, long long n_pcm, long long* info2, void* ws2,
                    hipStream_t st, const char** err) {
    if (R < 1 || R > 65535 || n_bytes < 8 || n_bytes > MAX_BYTES || total_frames < 0 || total_samples < 0 || n_plane < 0 || n_pcm < 0 ||
        max_channels < 1 || max_channels > MAXCH || total_frames > MAX_BYTES || total_samples >= (1ll << 37)) {
        *err = "flac_decode: bad sizes";
        return -22;
    }
    if (!data || !rows || !lay || !ws || !pcm || !info2 || !ws2) { *err = "flac_decode: null pointer"; return -22; }
    const Ws w = ws_layout(ws, n_bytes, R);
    int* plane = (int*)ws2;
    int* fst = plane + n_plane;
    if (total_frames)
        flac_restore_kernel<<<(unsigned)((total_frames * max_channels + MT - 1) / MT), MT, 0, st>>>(
            data, n_bytes, rows, R, lay, total_frames, max_channels, w.counts, w.nb, w.cand, w.cap, w.rec, w.sub, w.gen, w.s0, w.clip, plane, n_plane,
            n_pcm, fst);
    flac_verdict_kernel<<<(R + MT - 1) / MT, MT, 0, st>>>(rows, R, n_bytes, lay, total_frames, w.counts, w.nb, w.cand, w.cap, w.gen, w.clip, n_plane, n_pcm,
                                                         fst, info2);
    if (total_samples)
        flac_interleave_kernel<<<(unsigned)((total_samples + MT - 1) / MT), MT, 0, st>>>(rows, R, n_bytes, lay, total_samples, w.counts, w.nb, w.cand, w.cap,
                                                                                       w.rec, w.gen, w.s0, w.clip, plane, n_plane, pcm, n_pcm);
    hipError_t he = hipGetLastError();
    if (he != hipSuccess) { *err = hipGetErrorString(he); return -5; }
    return 0;
}
#endif
