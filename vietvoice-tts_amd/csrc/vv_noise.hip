// N9 start noise of the flow ODE, generated on the device: x[b][t][m] is a pure function of (seed, stream, t, m).
// Philox4x32-10 (Salmon, Moraes, Dror, Shaw, SC'11): key = the 64-bit seed, counter = (q, 0, stream_lo, stream_hi) where element
// e = t * n_mel + m of an item lies in group q = e >> 2 and takes output word e & 3.  n_mel % 4 == 0, so a group never crosses a frame:
// one thread owns one group and stores it once, as one float4.  Rows t >= clamp(seq_len[b], 0, N) are +0.0f.  No LDS, no atomics.
//   uniform : u(w) = ((w >> 9) + 0.5f) * 2^-23   -- exact in fp32, never 0, never 1
//   normal  : Box-Muller on the word pairs (0, 1) and (2, 3): r = sqrtf(-2 logf(u0)), z0 = r cospif(2 u1), z1 = r sinpif(2 u1)
//             (2 u is exact: no rounded 2 pi enters).  Precise libm forms only, as in the Vocos spectrum kernel: this file is built
//             without fast-math and uses no __-prefixed intrinsic.
#ifndef VV_NOISE_HOST_CHECK           // tools/noise_host_check.cpp compiles the kernel below for the host, on tools/hip_host_shim.h
#include "vv_common.h"
#include "vv_kernels.h"
#endif

namespace {

constexpr uint32_t PHILOX_M0 = 0xD2511F53u, PHILOX_M1 = 0xCD9E8D57u, PHILOX_W0 = 0x9E3779B9u, PHILOX_W1 = 0xBB67AE85u;

// host + device: the same text can be checked against the Random123 known answers by a host program
__host__ __device__ __forceinline__ uint4 philox4x32_10(uint4 c, uint32_t k0, uint32_t k1) {
#pragma unroll
    for (int r = 0; r < 10; ++r) {
        const uint64_t p0 = (uint64_t)PHILOX_M0 * c.x, p1 = (uint64_t)PHILOX_M1 * c.z;      // v_mul_hi_u32 + v_mul_lo_u32 each
        c = make_uint4((uint32_t)(p1 >> 32) ^ c.y ^ k0, (uint32_t)p1, (uint32_t)(p0 >> 32) ^ c.w ^ k1, (uint32_t)p0);
        k0 += PHILOX_W0;
        k1 += PHILOX_W1;
    }
    return c;
}

__host__ __device__ __forceinline__ float philox_uniform(uint32_t w) { return ((float)(w >> 9) + 0.5f) * 0x1p-23f; }

// x [B][N][n_mel], keys [B][2] = {seed, stream}.  per_item = N * n_mel / 4 groups per item (<= 2^32: the counter word q), total = B * per_item.
template <int KIND>
__global__ __launch_bounds__(256) void noise_fill_kernel(float* __restrict__ x, const int* __restrict__ seq_len,
                                                         const unsigned long long* __restrict__ keys, int N, int n_mel,
                                                         unsigned long long per_item, unsigned long long total) {
    for (unsigned long long i = (unsigned long long)blockIdx.x * 256 + threadIdx.x; i < total; i += (unsigned long long)gridDim.x * 256) {
        const unsigned long long b = i / per_item, q = i - b * per_item;
        const int t = (int)(q * 4 / (unsigned)n_mel);
        const int len = min(max(seq_len[b], 0), N);
        float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
        if (t < len) {
            const unsigned long long seed = keys[2 * b], stream = keys[2 * b + 1];
            const uint4 w = philox4x32_10(make_uint4((uint32_t)q, 0u, (uint32_t)stream, (uint32_t)(stream >> 32)), (uint32_t)seed,
                                          (uint32_t)(seed >> 32));
            const float u0 = philox_uniform(w.x), u1 = philox_uniform(w.y), u2 = philox_uniform(w.z), u3 = philox_uniform(w.w);
            if (KIND == 1) {
                v = make_float4(u0, u1, u2, u3);
            } else {
                const float ra = sqrtf(-2.0f * logf(u0)), rb = sqrtf(-2.0f * logf(u2));
                v = make_float4(ra * cospif(2.0f * u1), ra * sinpif(2.0f * u1), rb * cospif(2.0f * u3), rb * sinpif(2.0f * u3));
            }
        }
        *(float4*)(x + i * 4) = v;
    }
}

}  // namespace

#ifndef VV_NOISE_HOST_CHECK
int vvk_noise_fill(float* x, const int* seq_len, const unsigned long long* keys, int B, int N, int n_mel, int kind, hipStream_t st,
                   const char** err) {
    if (B < 1 || N < 1 || n_mel < 4 || n_mel % 4) { *err = "noise_fill: B, N >= 1 and n_mel a positive multiple of 4"; return -22; }
    if (kind != 0 && kind != 1) { *err = "noise_fill: kind is 0 (normal) or 1 (uniform)"; return -22; }
    if (!x || !seq_len || !keys || (uintptr_t)x % 16 || (uintptr_t)keys % 8) { *err = "noise_fill: null or misaligned buffer"; return -22; }
    const unsigned long long per_item = (unsigned long long)N * (unsigned)n_mel / 4;
    if (per_item > (1ull << 32)) { *err = "noise_fill: an item has more than 2^32 groups of four elements"; return -22; }
    const unsigned long long total = per_item * (unsigned)B;
    const int grid = (int)std::min<unsigned long long>((total + 255) / 256, 256 * 8);
    if (kind == 1) noise_fill_kernel<1><<<grid, 256, 0, st>>>(x, seq_len, keys, N, n_mel, per_item, total);
    else noise_fill_kernel<0><<<grid, 256, 0, st>>>(x, seq_len, keys, N, n_mel, per_item, total);
    hipError_t he = hipGetLastError();
    if (he != hipSuccess) { *err = hipGetErrorString(he); return -5; }
    return 0;
}
#endif
