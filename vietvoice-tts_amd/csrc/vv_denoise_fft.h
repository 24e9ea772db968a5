// The 1024-point float64 transform of the PCM stage, shared by vv_denoise.hip and vv_watermark.hip: radix-2 decimation in
// time behind a bit reversal, in LDS, by a workgroup of 256 threads.  The arithmetic is core/audio_processor.py's denoise_fft, operation by
// operation; the including file sets "#pragma clang fp contract(off)" in front of the include.  Internal: everything is in an unnamed namespace.
#pragma once
#ifndef VV_HIP_HOST_SHIM               // tools/hip_host_shim.h: the host checks bring their own stand-ins
#include "vv_common.h"
#endif

namespace {

constexpr int DN = 1024;                      // VV_DENOISE_N
constexpr int DH = 256;                       // VV_DENOISE_H
constexpr int DLDS = DN + DN / 4;             // doubles of one padded plane
static_assert(DN == 1024 && DH == 256 && DN == 4 * DH, "the index arithmetic below assumes these");

__device__ __forceinline__ int pad(int i) { return i + (i >> 2); }
__device__ __forceinline__ int rev10(int i) { return (int)(__brev((unsigned)i) >> 22); }

// stages S and S + 1 on the four points base + {0, h, 2 h, 3 h}, h = 2^S, of thread t: (0, 1) and (2, 3) meet in stage S, (0, 2) and (1, 3)
// in stage S + 1.  s_tw = cos | -sin, N / 2 each
template <int S>
__device__ __forceinline__ void two_stages(double* __restrict__ s_re, double* __restrict__ s_im, const double* __restrict__ s_tw, int t, bool inverse) {
    constexpr int h = 1 << S;
    const int j = t & (h - 1), base = ((t >> S) << (S + 2)) + j;
    double ar[4], ai[4];
    int at[4];
#pragma unroll
    for (int m = 0; m < 4; ++m) {
        at[m] = pad(base + m * h);
        ar[m] = s_re[at[m]];
        ai[m] = s_im[at[m]];
    }
    auto bfly = [&](int a, int b, int k) {
        const double c = s_tw[k], s = inverse ? -s_tw[DN / 2 + k] : s_tw[DN / 2 + k];
        const double tr = ar[b] * c - ai[b] * s;
        const double ti = ar[b] * s + ai[b] * c;
        const double xr = ar[a], xi = ai[a];
        ar[a] = xr + tr;
        ai[a] = xi + ti;
        ar[b] = xr - tr;
        ai[b] = xi - ti;
    };
    bfly(0, 1, j * (DN / 2 >> S));
    bfly(2, 3, j * (DN / 2 >> S));
    bfly(0, 2, j * (DN / 4 >> S));
    bfly(1, 3, (j + h) * (DN / 4 >> S));
#pragma unroll
    for (int m = 0; m < 4; ++m) {
        s_re[at[m]] = ar[m];
        s_im[at[m]] = ai[m];
    }
}

// the ten stages over the bit-reversed frame in LDS; on return every thread sees the result
__device__ __forceinline__ void transform(double* __restrict__ s_re, double* __restrict__ s_im, const double* __restrict__ s_tw, int t, bool inverse) {
    two_stages<0>(s_re, s_im, s_tw, t, inverse);
    __syncthreads();
    two_stages<2>(s_re, s_im, s_tw, t, inverse);
    __syncthreads();
    two_stages<4>(s_re, s_im, s_tw, t, inverse);
    __syncthreads();
    two_stages<6>(s_re, s_im, s_tw, t, inverse);
    __syncthreads();
    two_stages<8>(s_re, s_im, s_tw, t, inverse);
    __syncthreads();
}

// w[k] x[start + k], zero outside [0, n), bit-reversed into LDS
__device__ __forceinline__ void load_frame(const int16_t* __restrict__ x, long long n, long long start, const double* __restrict__ window,
                                           double* __restrict__ s_re, double* __restrict__ s_im, int t) {
#pragma unroll
    for (int m = 0; m < 4; ++m) {
        const int p = t + 256 * m, k = rev10(p);
        const long long i = start + k;
        const double u = i >= 0 && i < n ? (double)x[i] : 0.0;
        s_re[pad(p)] = window[k] * u;
        s_im[pad(p)] = 0.0;
    }
}

}  // namespace
