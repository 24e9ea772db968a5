// numpy's float32 summation order, shared by the clip ingest (np.mean of a clip, vv_ingest.hip) and the output stage (the RMS of a
// junction, vv_output.hip): add.reduce walks the array in buffers of 8192 elements, sums each buffer pairwise (leaves of <= 128
// elements on 8 interleaved accumulators, split at (n / 2) & ~7) and accumulates the buffer sums in order.  ONE implementation of
// that order: a workgroup of 256 threads sums one buffer, 8 lanes per leaf = numpy's 8 accumulators, the tree combined through LDS.
#pragma once
#ifndef VV_HIP_HOST_SHIM               // tools/hip_host_shim.h: the host checks bring their own stand-ins
#include <hip/hip_runtime.h>
#endif

constexpr int NP_BUF = 8192;          // np.getbufsize(): add.reduce hands the inner loop one buffer at a time
constexpr int NP_LEAF = 128;          // PW_BLOCKSIZE of numpy's pairwise sum
constexpr int PW_DEPTH = 7;           // a buffer's tree is at most 7 deep: right child <= n / 2 + 8  ->  8192 / 128 + 16 <= 128

// node (k, p) of the pairwise tree over L elements: its length (0 = does not exist: an ancestor already is a leaf) and start
__device__ __forceinline__ int pw_node(int L, int k, int p, int& start) {
    int len = L;
    start = 0;
    for (int j = 0; j < k; ++j) {
        if (len <= NP_LEAF) return 0;
        const int n2 = (len >> 1) & ~7;
        if ((p >> (k - 1 - j)) & 1) { start += n2; len -= n2; } else len = n2;
    }
    return len;
}

// The pairwise sum of one buffer x(0) ... x(L - 1), 0 <= L <= 8192, exactly as numpy's FLOAT_pairwise_sum orders it.  Called by ALL 256
// threads of the workgroup with the same L; v = 128 floats of LDS; every thread returns the sum.  x(i) must be a pure read (no fma can
// form across the call: the additions below are plain float adds of loaded values).
template <typename Load>
__device__ __forceinline__ float np_buffer_sum(Load x, int L, float* v) {
    const int lane = threadIdx.x & 7;
    for (int it = 0; it < 4; ++it) {
        const int slot = it * 32 + (threadIdx.x >> 3);                           // 7 path bits, most significant first
        int len = L, start = 0, k = 0;
        for (; k < PW_DEPTH && len > NP_LEAF; ++k) {
            const int n2 = (len >> 1) & ~7;
            if ((slot >> (PW_DEPTH - 1 - k)) & 1) { start += n2; len -= n2; } else len = n2;
        }
        const bool owner = (slot & ((1 << (PW_DEPTH - k)) - 1)) == 0;            // a leaf at depth k belongs to the slot with zero low bits
        if (!owner) len = 0;
        float r = 0.f;
        const int body = len - (len & 7);
        if (len >= 8) {                                                          // r[lane] = a[lane] + a[8 + lane] + ...
            r = x(start + lane);
            for (int i = 8; i < body; i += 8) r += x(start + i + lane);
        }
        r += __shfl_xor(r, 1);                                                   // (r0 + r1), (r2 + r3), ...
        r += __shfl_xor(r, 2);                                                   // ((r0 + r1) + (r2 + r3)), ...
        r += __shfl_xor(r, 4);
        if (lane == 0) {
            for (int i = (len >= 8 ? body : 0); i < len; ++i) r += x(start + i);    // the tail (or a whole leaf of < 8) in order
            v[slot] = r;
        }
    }
    __syncthreads();
    for (int k = PW_DEPTH - 1; k >= 0; --k) {                                    // node = left child + right child, bottom up
        const int p = threadIdx.x;
        if (p < (1 << k)) {
            int st;
            if (pw_node(L, k, p, st) > NP_LEAF) v[p << (PW_DEPTH - k)] += v[(p << (PW_DEPTH - k)) + (1 << (PW_DEPTH - 1 - k))];
        }
        __syncthreads();
    }
    const float s = v[0];
    __syncthreads();                                                             // v may be overwritten by the next call
    return s;
}
