// N25: IMA ADPCM output on the device, and IMA ADPCM / G.711 reference clips decoded on the device (WAVE format tags 0x11, 7, 6).
// The arithmetic is the specification: core/audio_processor.py (adpcm_encode_blocks, adpcm_decode_frames, ulaw2lin, alaw2lin) restates the
// quantiser and predictor of CPython's Modules/audioop.c (lin2adpcm / adpcm2lin, the Intel/DVI coder of the IMA recommendation of 1992), and
// the kernels below make the same choices and pack the same bytes.  Everything is integer arithmetic; there is no float in this file.
//     encode  : one workgroup per block of spb samples (spb = 8 k + 1; block = 4 header bytes + (spb - 1) / 2).  The block's samples are staged
//               once in LDS (the padding of a signal's last block repeats its last real sample), the 89 step sizes too.  Lane c < 89 runs the
//               quantiser over the block from the header state (x[0], c): every lane reads the same sample (an LDS broadcast) and its own
//               step; the three compares are selects, so the lanes stay converged.  Its error, the sum of (x - p)^2 over the REAL samples
//               in int64 (p = what a decoder reconstructs), goes to LDS; every thread walks the 89 errors in index order and keeps the first
//               smallest (fixed order: the smallest index of equals).  Thread 0 then runs the block once more from the winner and packs the
//               codes, low nibble first, into an LDS image of the block; all threads copy the image out with 4-byte stores.
//               (The other way, 89 lanes parking their codes in LDS, needs 89 x (spb - 1) / 2 bytes -- 45 KB at 24 kHz, 91 KB at 48 kHz --
//               and so one workgroup per CU; the second pass costs one lane's time, 1 / 89 of the search: profiles/adpcm/notes.md.)
//     check   : one workgroup per clip: the step index of every block header of an ADPCM clip; the FIRST one above 88 in file order (a
//               minimum over the lanes, reduced in LDS) is the clip's status {reason, byte}.  A clip is its own workgroup's alone.
//     decode  : ADPCM: one lane per (block, channel), the block's codes in sequence, 4 bytes (8 samples) at a time; int16 stores into the
//               interleaved frames vv_ingest_pcm reads.  A block with a bad header writes nothing.  G.711: elementwise, 8 codes (one 8-byte
//               load) to 8 samples (one 16-byte store) per lane and trip, a scalar tail.
// No atomics, no dependence on the execution order; every output byte is written by one thread, once.  Every read is bounded by the
// row's own sizes, which the kernels check again (the host has refused such a row before anything is launched).
#ifndef VV_ADPCM_HOST_CHECK           // tools/adpcm_host_check.cpp compiles the kernels below for the host, on tools/hip_host_shim.h
#include "vv_common.h"
#include "vv_kernels.h"
#endif

namespace {

constexpr int NCAND = 89;                     // step indices 0 ... 88
constexpr int ENC_NT = 128;                   // threads of the encoder: 89 candidates in two waves
constexpr int DEC_NT = 256;                   // threads of the check and decode kernels
constexpr int MAX_BA = 4096;                  // VV_ADPCM_MAX_BLOCK_ALIGN: bytes of the largest block the encoder writes
constexpr int MAX_SPB = (MAX_BA - 4) * 2 + 1; // 8185 samples
constexpr int TAG_ALAW = 6, TAG_ULAW = 7, TAG_ADPCM = 0x11;
constexpr int ST_STEP_INDEX = 1, ST_BLOCK_ALIGN = 2;      // VV_WAV_STEP_INDEX, VV_WAV_BLOCK_ALIGN
constexpr int WROW = 8;                       // int64 per clip row of the decoder

__device__ const int kSteps[NCAND] = {
    7, 8, 9, 10, 11, 12, 13, 14, 16, 17, 19, 21, 23, 25, 28, 31, 34, 37, 41, 45, 50, 55, 60, 66, 73, 80, 88, 97, 107, 118, 130, 143,
    157, 173, 190, 209, 230, 253, 279, 307, 337, 371, 408, 449, 494, 544, 598, 658, 724, 796, 876, 963, 1060, 1166, 1282, 1411,
    1552, 1707, 1878, 2066, 2272, 2499, 2749, 3024, 3327, 3660, 4026, 4428, 4871, 5358, 5894, 6484, 7132, 7845, 8630, 9493,
    10442, 11487, 12635, 13899, 15289, 16818, 18500, 20350, 22385, 24623, 27086, 29794, 32767};

__device__ __forceinline__ int clamp16(int v) { return v > 32767 ? 32767 : v < -32768 ? -32768 : v; }

// indexTable of audioop.c: -1 for the codes 0 ... 3 (and 8 ... 11), 2, 4, 6, 8 for 4 ... 7 (and 12 ... 15)
__device__ __forceinline__ int next_index(int index, int code) {
    index += (code & 4) ? ((code & 3) + 1) * 2 : -1;
    return index < 0 ? 0 : index > 88 ? 88 : index;
}

// one sample of lin2adpcm: the code; pred and index move on.  Selects only: lanes with different steps stay converged
__device__ __forceinline__ int quantise(int x, int& pred, int& index, const int* __restrict__ steps) {
    const int step = steps[index], s1 = step >> 1, s2 = step >> 2;
    int d = x - pred;
    const int sign = d < 0 ? 8 : 0;
    d = d < 0 ? -d : d;
    const int b2 = d >= step ? 1 : 0;
    d -= b2 ? step : 0;
    const int b1 = d >= s1 ? 1 : 0;
    d -= b1 ? s1 : 0;
    const int b0 = d >= s2 ? 1 : 0;
    const int vp = (step >> 3) + (b2 ? step : 0) + (b1 ? s1 : 0) + (b0 ? s2 : 0);
    pred = clamp16(sign ? pred - vp : pred + vp);
    const int code = sign | (b2 << 2) | (b1 << 1) | b0;
    index = next_index(index, code);
    return code;
}

// one sample of adpcm2lin
__device__ __forceinline__ int expand(int code, int& pred, int& index, const int* __restrict__ steps) {
    const int step = steps[index];
    const int vp = (step >> 3) + ((code & 4) ? step : 0) + ((code & 2) ? step >> 1 : 0) + ((code & 1) ? step >> 2 : 0);
    pred = clamp16((code & 8) ? pred - vp : pred + vp);
    index = next_index(index, code);
    return pred;
}

// rows (3 int64): {src_off, n, dst_off in bytes}: x[src_off, +n) becomes ceil(n / spb) blocks at y + dst_off.  grid (blocks, R)
__global__ __launch_bounds__(ENC_NT) void adpcm_encode_kernel(const int16_t* __restrict__ x, long long n_x, const long long* __restrict__ rows, int spb,
                                                              uint8_t* __restrict__ y, long long n_y) {
    __shared__ short s[MAX_SPB + 1];
    __shared__ int steps[NCAND];
    __shared__ long long err[NCAND];
    __shared__ unsigned image[MAX_BA / 4];
    const long long* r = rows + 3 * (long long)blockIdx.y;
    const long long so = r[0], n = r[1], dof = r[2];
    const int tid = (int)threadIdx.x;
    if (spb < 9 || spb > MAX_SPB || (spb - 1) % 8) return;
    const int ba = (spb - 1) / 2 + 4;
    if (so < 0 || n < 1 || n > n_x || so > n_x - n || dof < 0 || dof % 4) return;
    const long long nblk = (n + spb - 1) / spb;
    if (nblk > (n_y - dof) / ba) return;
    if (tid < NCAND) steps[tid] = kSteps[tid];
    for (long long b = blockIdx.x; b < nblk; b += gridDim.x) {
        const long long first = b * spb;
        const int real = n - first < spb ? (int)(n - first) : spb;               // 1 ... spb samples of the signal; the rest repeats the last
        for (int t = tid; t < spb; t += ENC_NT) s[t] = x[so + first + (t < real ? t : real - 1)];
        __syncthreads();
        if (tid < NCAND) {
            int pred = s[0], index = tid;
            long long e = 0;
            for (int t = 1; t < real; ++t) {
                const int v = s[t];
                quantise(v, pred, index, steps);
                const long long d = v - pred;
                e += d * d;
            }
            err[tid] = e;
        }
        __syncthreads();
        int best = 0;
        long long lo = err[0];
        for (int c = 1; c < NCAND; ++c) {
            const long long e = err[c];
            if (e < lo) { lo = e; best = c; }
        }
        if (tid == 0) {
            int pred = s[0], index = best;
            image[0] = ((unsigned)pred & 0xffffu) | ((unsigned)best << 16);
            for (int k = 0; k < (spb - 1) / 8; ++k) {
                unsigned w = 0;
#pragma unroll
                for (int j = 0; j < 8; ++j) w |= (unsigned)quantise(s[1 + 8 * k + j], pred, index, steps) << (4 * j);      // low nibble first
                image[1 + k] = w;
            }
        }
        __syncthreads();
        unsigned* out = (unsigned*)(y + dof + b * ba);
        for (int w = tid; w < ba / 4; w += ENC_NT) out[w] = image[w];
        __syncthreads();
    }
}

// a clip row {data byte offset, n_bytes, tag, channels, block align, frames, pcm byte offset, 0} that the kernels may follow
__device__ __forceinline__ bool wav_row_ok(const long long* __restrict__ r, long long n_data, long long n_pcm) {
    const long long off = r[0], nb = r[1], tag = r[2], ch = r[3], ba = r[4], frames = r[5], po = r[6];
    if (off < 0 || off % 16 || nb < 0 || nb > n_data || off > n_data - nb || ch < 1 || ch > 65535 || frames < 0 || po < 0 || po % 16) return false;
    if (frames > (n_pcm - po) / (2 * ch)) return false;
    if (tag == TAG_ADPCM) {
        if (ch > 2 || ba < 8 * ch || ba % (4 * ch) || ba > 65535) return false;
        const long long full = nb / ba, rem = nb % ba;
        long long part = 0;
        if (rem >= 4 * ch) {
            const long long q = (rem - 4 * ch) / (4 * ch), m = (rem - 4 * ch) % (4 * ch) - 4 * (ch - 1);
            part = 1 + 8 * q + 2 * (m > 0 ? m : 0);
        }
        return frames <= full * ((ba / ch - 4) * 2 + 1) + part;
    }
    return (tag == TAG_ALAW || tag == TAG_ULAW) && frames <= nb / ch;
}

// status (2 int64 per clip) = {0, 0}, or {reason, byte offset inside the clip's data}.  grid R
__global__ __launch_bounds__(DEC_NT) void wav_check_kernel(const uint8_t* __restrict__ data, long long n_data, const long long* __restrict__ rows,
                                                           long long n_pcm, long long* __restrict__ status) {
    __shared__ long long first[DEC_NT];
    const long long* r = rows + WROW * (long long)blockIdx.x;
    const int tid = (int)threadIdx.x;
    if (!wav_row_ok(r, n_data, n_pcm)) {
        if (tid == 0) { status[2 * blockIdx.x] = ST_BLOCK_ALIGN; status[2 * blockIdx.x + 1] = 0; }
        return;
    }
    const long long off = r[0], nb = r[1], ch = r[3], ba = r[4];
    long long at = -1;
    if (r[2] == TAG_ADPCM) {
        const long long heads = (nb / ba + (nb % ba >= 4 * ch ? 1 : 0)) * ch;     // the (block, channel) headers that are whole
        for (long long i = tid; i < heads; i += DEC_NT) {
            const long long pos = (i / ch) * ba + 4 * (i % ch) + 2;
            if (data[off + pos] > 88 && (at < 0 || pos < at)) at = pos;
        }
    }
    first[tid] = at;
    __syncthreads();
    for (int h = DEC_NT / 2; h > 0; h >>= 1) {
        if (tid < h) {
            const long long a = first[tid], b = first[tid + h];
            first[tid] = a < 0 ? b : b < 0 ? a : a < b ? a : b;
        }
        __syncthreads();
    }
    if (tid == 0) {
        status[2 * blockIdx.x] = first[0] >= 0 ? ST_STEP_INDEX : 0;
        status[2 * blockIdx.x + 1] = first[0] >= 0 ? first[0] : 0;
    }
}

// one lane per (block, channel) of the ADPCM clips.  grid (bx, R)
__global__ __launch_bounds__(DEC_NT) void adpcm_decode_kernel(const uint8_t* __restrict__ data, long long n_data, const long long* __restrict__ rows,
                                                              uint8_t* __restrict__ pcm, long long n_pcm) {
    __shared__ int steps[NCAND];
    const long long* r = rows + WROW * (long long)blockIdx.y;
    if (r[2] != TAG_ADPCM || !wav_row_ok(r, n_data, n_pcm)) return;
    const int tid = (int)threadIdx.x;
    if (tid < NCAND) steps[tid] = kSteps[tid];
    __syncthreads();
    const long long off = r[0], nb = r[1], ch = r[3], ba = r[4], frames = r[5];
    const long long spb = (ba / ch - 4) * 2 + 1;
    const long long heads = (nb / ba + (nb % ba >= 4 * ch ? 1 : 0)) * ch;
    int16_t* out = (int16_t*)(pcm + r[6]);
    for (long long i = (long long)blockIdx.x * DEC_NT + tid; i < heads; i += (long long)gridDim.x * DEC_NT) {
        const long long b = i / ch, c = i % ch, f0 = b * spb;
        const long long lim = frames - f0 < spb ? frames - f0 : spb;              // frames of this block that are written
        if (lim <= 0) continue;
        const uint8_t* p = data + off + b * ba;
        const long long left = nb - b * ba;                                        // bytes of this block inside the clip: >= 4 ch
        int pred = (int)(int16_t)(p[4 * c] | (p[4 * c + 1] << 8)), index = p[4 * c + 2];
        if (index > 88) continue;                                                  // the clip is refused (wav_check_kernel): nothing of this block
        out[f0 * ch + c] = (int16_t)pred;
        for (long long g = 0; 1 + 8 * g < lim; ++g) {
            const long long at = 4 * ch + g * 4 * ch + 4 * c;                      // this channel's 4 bytes of round g
            unsigned w = 0;
            if (at + 4 <= left) w = *(const unsigned*)(p + at);
            else for (int k = 0; k < 4; ++k) w |= at + k < left ? (unsigned)p[at + k] << (8 * k) : 0u;
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                const int v = expand((int)((w >> (4 * j)) & 15u), pred, index, steps);
                const long long t = 1 + 8 * g + j;
                if (t < lim) out[(f0 + t) * ch + c] = (int16_t)v;
            }
        }
    }
}

__device__ __forceinline__ int ulaw2lin(unsigned code) {
    const int u = (int)(~code & 0xffu);
    const int t = (((u & 0x0f) << 3) + 0x84) << ((u & 0x70) >> 4);
    return (u & 0x80) ? 0x84 - t : t - 0x84;
}

__device__ __forceinline__ int alaw2lin(unsigned code) {
    const int a = (int)((code ^ 0x55u) & 0xffu), seg = (a & 0x70) >> 4;
    int t = ((a & 0x0f) << 4) + (seg == 0 ? 8 : 0x108);
    t = seg > 1 ? t << (seg - 1) : t;
    return (a & 0x80) ? t : -t;
}

// the codes in bits sh ... sh + 7 and sh + 8 ... sh + 15 of w -> two int16 in one word
__device__ __forceinline__ unsigned g711_pair(unsigned w, int sh, bool ulaw) {
    const int a = ulaw ? ulaw2lin((w >> sh) & 0xffu) : alaw2lin((w >> sh) & 0xffu);
    const int b = ulaw ? ulaw2lin((w >> (sh + 8)) & 0xffu) : alaw2lin((w >> (sh + 8)) & 0xffu);
    return ((unsigned)a & 0xffffu) | ((unsigned)b << 16);
}

// the G.711 clips: frames * channels codes -> as many int16.  grid (bx, R)
__global__ __launch_bounds__(DEC_NT) void g711_decode_kernel(const uint8_t* __restrict__ data, long long n_data, const long long* __restrict__ rows,
                                                             uint8_t* __restrict__ pcm, long long n_pcm) {
    const long long* r = rows + WROW * (long long)blockIdx.y;
    if ((r[2] != TAG_ALAW && r[2] != TAG_ULAW) || !wav_row_ok(r, n_data, n_pcm)) return;
    const bool ulaw = r[2] == TAG_ULAW;
    const long long n = r[5] * r[3];
    const uint8_t* src = data + r[0];
    int16_t* out = (int16_t*)(pcm + r[6]);
    for (long long q = (long long)blockIdx.x * DEC_NT + threadIdx.x; q * 8 < n; q += (long long)gridDim.x * DEC_NT) {
        const long long j0 = q * 8;
        if (j0 + 8 <= n) {
            const uint2 u = *(const uint2*)(src + j0);
            uint4 o;
            o.x = g711_pair(u.x, 0, ulaw); o.y = g711_pair(u.x, 16, ulaw); o.z = g711_pair(u.y, 0, ulaw); o.w = g711_pair(u.y, 16, ulaw);
            *(uint4*)(out + j0) = o;
        } else {
            for (long long j = j0; j < n; ++j) out[j] = (int16_t)(ulaw ? ulaw2lin(src[j]) : alaw2lin(src[j]));
        }
    }
}

#ifndef VV_ADPCM_HOST_CHECK
inline int launched(const char** err) {
    hipError_t he = hipGetLastError();
    if (he != hipSuccess) { *err = hipGetErrorString(he); return -5; }
    return 0;
}
#endif

}  // namespace

#ifndef VV_ADPCM_HOST_CHECK
int vvk_pcm_adpcm(const int16_t* x, long long n_x, const long long* rows, int R, int spb, long long max_blocks, uint8_t* y, long long n_y,
                  hipStream_t st, const char** err) {
    if (R < 1 || R > 65535 || n_x < 0 || n_y < 0 || max_blocks < 0) { *err = "pcm_adpcm: bad sizes"; return -22; }
    if (spb < 9 || spb > MAX_SPB || (spb - 1) % 8) { *err = "pcm_adpcm: samples_per_block is 8 k + 1 in 9 ... 8185"; return -22; }
    if (!x || !rows || !y || (uintptr_t)y % 8 || (uintptr_t)rows % 8) { *err = "pcm_adpcm: null or misaligned pointer (y 8 bytes)"; return -22; }
    if (max_blocks == 0) return 0;
    const dim3 grid((unsigned)(max_blocks > 65535 ? 65535 : max_blocks), R);
    adpcm_encode_kernel<<<grid, ENC_NT, 0, st>>>(x, n_x, rows, spb, y, n_y);
    return launched(err);
}

int vvk_wav_decode(const uint8_t* data, long long n_data, const long long* rows, int R, long long max_heads, long long max_codes, uint8_t* pcm,
                   long long n_pcm, long long* status, hipStream_t st, const char** err) {
    if (R < 1 || R > 65535 || n_data < 0 || n_pcm < 0 || max_heads < 0 || max_codes < 0) { *err = "wav_decode: bad sizes"; return -22; }
    if (!data || !rows || !pcm || !status || (uintptr_t)data % 16 || (uintptr_t)pcm % 16 || (uintptr_t)rows % 8 || (uintptr_t)status % 8) {
        *err = "wav_decode: null or misaligned pointer (data, pcm 16 bytes)";
        return -22;
    }
    wav_check_kernel<<<R, DEC_NT, 0, st>>>(data, n_data, rows, n_pcm, status);
    if (int e = launched(err)) return e;
    if (max_heads > 0) {
        long long bx = (max_heads + DEC_NT - 1) / DEC_NT;
        adpcm_decode_kernel<<<dim3((unsigned)(bx > 4096 ? 4096 : bx), R), DEC_NT, 0, st>>>(data, n_data, rows, pcm, n_pcm);
        if (int e = launched(err)) return e;
    }
    if (max_codes > 0) {
        long long bx = (max_codes / 8 + DEC_NT) / DEC_NT;
        g711_decode_kernel<<<dim3((unsigned)(bx > 4096 ? 4096 : bx), R), DEC_NT, 0, st>>>(data, n_data, rows, pcm, n_pcm);
        if (int e = launched(err)) return e;
    }
    return 0;
}
#endif
