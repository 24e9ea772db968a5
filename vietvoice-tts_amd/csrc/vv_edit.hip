// N5 speech editing: regenerate chosen time spans of an existing clip.  Synthesis conditions on a PREFIX (the
// reference clip's frames, then zeros); editing conditions on a FRAME MASK.  Two kernels here, the masked conditioning build is
// build_cat_kernel<true> (vv_elementwise.hip):
//   splice  : [B][ld_out] int16 clips assembled from source clips in HBM by descriptor rows {item, src_off, dst_off, n}:
//             copied where a row covers a sample, 0 elsewhere (the spans to regenerate, and everything past the clip)
//   restore : after the last Euler step, x[b][t] = cat[b][t][0:n_mel] wherever keep[b][t] (the known frames, bit for bit)
#ifndef VV_EDIT_HOST_CHECK            // tools/edit_host_check.cpp compiles the kernels below for the host, on tools/hip_host_shim.h
#include "vv_common.h"
#include "vv_kernels.h"
#endif

namespace {

constexpr int SPLICE_ROWS = 256;      // descriptor rows staged in LDS per pass (8 KB)

// One thread owns 4 consecutive output samples of one item (grid.y = item) and stores them once, as one 8-byte store: every
// output sample is written exactly once, no atomics.  The rows were validated by the caller (in range of both buffers, rows of
// one item disjoint on the output); the source index is also clamped here, so no row can make the kernel read outside src.
__global__ __launch_bounds__(256) void edit_splice_kernel(const int16_t* __restrict__ src, long long n_src,
                                                          const long long* __restrict__ desc, int n_rows, int16_t* __restrict__ out,
                                                          int ld_out) {
    __shared__ long long rows[SPLICE_ROWS][4];
    const int b = blockIdx.y;
    const long long j0 = ((long long)blockIdx.x * 256 + threadIdx.x) * 4;
    int v[4] = {0, 0, 0, 0};
    for (int r0 = 0; r0 < n_rows; r0 += SPLICE_ROWS) {
        const int nr = min(SPLICE_ROWS, n_rows - r0);
        __syncthreads();
        for (int i = threadIdx.x; i < nr * 4; i += 256) rows[i >> 2][i & 3] = desc[(size_t)r0 * 4 + i];
        __syncthreads();
        for (int r = 0; r < nr; ++r) {
            if (rows[r][0] != b) continue;
            const long long so = rows[r][1], d0 = rows[r][2], n = rows[r][3];
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const long long j = j0 + k, s = so + (j - d0);
                if (j >= d0 && j < d0 + n && s >= 0 && s < n_src) v[k] = src[s];
            }
        }
    }
    if (j0 < ld_out) {      // ld_out % 4 == 0: the 4 samples are all inside the row
        uint2 w;
        w.x = (uint32_t)(uint16_t)v[0] | ((uint32_t)(uint16_t)v[1] << 16);
        w.y = (uint32_t)(uint16_t)v[2] | ((uint32_t)(uint16_t)v[3] << 16);
        *(uint2*)(out + (size_t)b * ld_out + j0) = w;
    }
}

// x [B][N][n_mel], cat [B][N][cd]: float4 copies of the mel columns of the kept frames inside each item's length.
__global__ __launch_bounds__(256) void edit_restore_kernel(float* __restrict__ x, const float* __restrict__ cat,
                                                           const uint8_t* __restrict__ keep, int ld_keep, const int* __restrict__ seq_len,
                                                           int B, int N, int n_mel, int cd) {
    const int m4 = n_mel >> 2;
    const size_t total = (size_t)B * N * m4;
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (size_t)gridDim.x * 256) {
        const int c = (int)(i % m4) * 4;
        const size_t row = i / m4;
        const int t = (int)(row % N);
        const int b = (int)(row / N);
        if (t < seq_len[b] && keep[(size_t)b * ld_keep + t]) *(float4*)(x + row * n_mel + c) = *(const float4*)(cat + row * cd + c);
    }
}

}  // namespace

#ifndef VV_EDIT_HOST_CHECK
int vvk_edit_splice(const int16_t* src, long long n_src, const long long* desc, int n_rows, int B, int16_t* out, int ld_out,
                    hipStream_t st, const char** err) {
    if (B < 1 || B > 65535 || n_rows < 0 || ld_out < 4 || ld_out % 4 || n_src < 0) { *err = "edit_splice: bad sizes"; return -22; }
    if (!out || (n_rows > 0 && (!desc || !src)) || (uintptr_t)out % 8) { *err = "edit_splice: null or misaligned buffer"; return -22; }
    const unsigned bx = (unsigned)((ld_out / 4 + 255) / 256);
    edit_splice_kernel<<<dim3(bx, B), 256, 0, st>>>(src, n_src, desc, n_rows, out, ld_out);
    hipError_t he = hipGetLastError();
    if (he != hipSuccess) { *err = hipGetErrorString(he); return -5; }
    return 0;
}

int vvk_edit_restore(float* x, const float* cat, const uint8_t* keep, int ld_keep, const int* seq_len, int B, int N, int n_mel, int cd,
                     hipStream_t st, const char** err) {
    if (B < 1 || N < 1 || ld_keep < N || n_mel % 4 || cd % 4 || cd < n_mel) { *err = "edit_restore: bad sizes"; return -22; }
    if (!x || !cat || !keep || !seq_len || (uintptr_t)x % 16 || (uintptr_t)cat % 16) { *err = "edit_restore: null or misaligned buffer"; return -22; }
    const size_t total = (size_t)B * N * (n_mel / 4);
    const int grid = (int)std::min<size_t>((total + 255) / 256, 256 * 8);
    edit_restore_kernel<<<grid, 256, 0, st>>>(x, cat, keep, ld_keep, seq_len, B, N, n_mel, cd);
    hipError_t he = hipGetLastError();
    if (he != hipSuccess) { *err = hipGetErrorString(he); return -5; }
    return 0;
}
#endif
