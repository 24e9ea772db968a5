// HBM-bound kernels of the acoustic path: K4 LayerNorm/AdaLN-modulate, K2 conditioning pack,
// K9 CFG+Euler, text-side embedding gather / depthwise conv / GRN, and the tiny time-grid helpers.
// All are wave64-native: 16-byte vector loads, wave shuffles for row reductions, no LDS unless a
// cross-wave reduction is needed.
#ifndef VV_ELEMENTWISE_HOST_CHECK     // tools/elementwise_host_check.cpp compiles the kernels below for the host, on tools/hip_host_shim.h
#include "vv_common.h"
#include "vv_kernels.h"
#endif
#include <type_traits>

namespace {

// fp32 -> T -> fp32, element-wise (round to nearest even: what store4<T> / the GEMM epilogue's v_cvt_pk_bf16_f32 do)
template <typename T> __device__ __forceinline__ float4 round4_as(float4 a) {
    if constexpr (sizeof(T) == 2) {
        typedef __attribute__((ext_vector_type(4))) float f4v;
        const f4v r = __builtin_convertvector(__builtin_convertvector((f4v){a.x, a.y, a.z, a.w}, bf16x4), f4v);
        return make_float4(r[0], r[1], r[2], r[3]);
    } else {
        return a;
    }
}

// ---------------------------------------------------------------- K4: [x += delta;] y = LN(x) * (w [+1]) + b
// One wave per row, the row cached in registers (D <= 1024): one HBM read, one write.  When a
// delta is given (the gated branch output of the previous GEMM) the residual add is fused here:
// the fp32 stream is read once, updated, written back and normalised in the same pass.
template <typename To, typename Td>
__global__ __launch_bounds__(256) void ln_mod_kernel(float* __restrict__ x, int ldx, To* __restrict__ y, int ldy,
                                                     int R, int D, const float* __restrict__ w,
                                                     const float* __restrict__ b, int add_one, float eps,
                                                     const Td* __restrict__ delta, int ldd, const Td* __restrict__ delta2,
                                                     int keep_x, int tail_row0, int tp1, const float* __restrict__ dt1, int tp2,
                                                     const float* __restrict__ dt2) {
    const int lane = threadIdx.x & 63;
    const int row = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= R) return;
    const int n4 = D >> 2;
    float* xr = x + (size_t)row * ldx;
    float4 v[4];
    float s = 0.f;
    if (delta) {
        // all loads of the row first (x, delta, delta2: up to 12 independent 16-byte loads in flight), then the adds
        float4 d[4], d2[4];
        // rows of a split-K tail (wave-uniform, a few per cent of the rows): the GEMM left the row's K parts in fp32 and did NOT
        // write the row of the delta itself; the parts are summed here in part order and the SUM is rounded to the delta's dtype
        // once -- the rounding a row outside the tail got in the GEMM epilogue -- so the stream sees the same kind of delta on
        // every row, whatever the row's position in the launch.
        const bool tl1 = tp1 > 0 && row >= tail_row0, tl2 = tp2 > 0 && row >= tail_row0;
        const float4 z4 = make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int c = lane + i * 64;
            if (c < n4) {
                v[i] = load4_nt<float>(xr + c * 4);             // the fp32 stream is far larger than the caches: stream it
                d[i] = tl1 ? z4 : load4_nt<Td>(delta + (size_t)row * ldd + c * 4);      // read once: keep it out of the caches
                d2[i] = (delta2 && !tl2) ? load4_nt<Td>(delta2 + (size_t)row * ldd + c * 4) : z4;
            } else {
                v[i] = d[i] = d2[i] = z4;
            }
        }
        if (row >= tail_row0) {
            const size_t tr = (size_t)(R - tail_row0), r = (size_t)(row - tail_row0);
            if (tl1) {
                for (int p = 0; p < tp1; ++p)
#pragma unroll
                    for (int i = 0; i < 4; ++i) {
                        const int c = lane + i * 64;
                        if (c < n4) {
                            const float4 t = load4_nt<float>(dt1 + (p * tr + r) * ldd + c * 4);
                            d[i].x += t.x; d[i].y += t.y; d[i].z += t.z; d[i].w += t.w;
                        }
                    }
#pragma unroll
                for (int i = 0; i < 4; ++i) d[i] = round4_as<Td>(d[i]);
            }
            if (tl2) {
                for (int p = 0; p < tp2; ++p)
#pragma unroll
                    for (int i = 0; i < 4; ++i) {
                        const int c = lane + i * 64;
                        if (c < n4) {
                            const float4 t = load4_nt<float>(dt2 + (p * tr + r) * ldd + c * 4);
                            d2[i].x += t.x; d2[i].y += t.y; d2[i].z += t.z; d2[i].w += t.w;
                        }
                    }
#pragma unroll
                for (int i = 0; i < 4; ++i) d2[i] = round4_as<Td>(d2[i]);
            }
        }
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int c = lane + i * 64;
            if (c < n4) {
                v[i].x += d[i].x; v[i].y += d[i].y; v[i].z += d[i].z; v[i].w += d[i].w;
                if (delta2) {                                // (x + delta) + delta2: the order the one-delta-at-a-time protocol adds in
                    v[i].x += d2[i].x; v[i].y += d2[i].y; v[i].z += d2[i].z; v[i].w += d2[i].w;
                }
                if (!keep_x) {
                    typedef __attribute__((ext_vector_type(4))) float f4;
                    const f4 w4 = {v[i].x, v[i].y, v[i].z, v[i].w};
                    __builtin_nontemporal_store(w4, (f4*)(xr + c * 4));
                }
                s += (v[i].x + v[i].y) + (v[i].z + v[i].w);
            }
        }
    } else {
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int c = lane + i * 64;
            if (c < n4) {
                v[i] = load4_nt<float>(xr + c * 4);
                s += (v[i].x + v[i].y) + (v[i].z + v[i].w);
            } else {
                v[i] = make_float4(0.f, 0.f, 0.f, 0.f);
            }
        }
    }
    const float mean = wave_sum(s) / (float)D;
    float q = 0.f;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int c = lane + i * 64;
        if (c < n4) {
            const float a = v[i].x - mean, bb = v[i].y - mean, cc = v[i].z - mean, dd = v[i].w - mean;
            q += (a * a + bb * bb) + (cc * cc + dd * dd);
        }
    }
    const float rstd = rsqrtf(wave_sum(q) / (float)D + eps);
    const float one = add_one ? 1.0f : 0.0f;
    To* yr = y + (size_t)row * ldy;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int c = lane + i * 64;
        if (c < n4) {
            float4 ww = w ? *(const float4*)(w + c * 4) : make_float4(1.f - one, 1.f - one, 1.f - one, 1.f - one);
            float4 bv = b ? *(const float4*)(b + c * 4) : make_float4(0.f, 0.f, 0.f, 0.f);
            store4<To>(yr + c * 4, (v[i].x - mean) * rstd * (ww.x + one) + bv.x, (v[i].y - mean) * rstd * (ww.y + one) + bv.y,
                       (v[i].z - mean) * rstd * (ww.z + one) + bv.z, (v[i].w - mean) * rstd * (ww.w + one) + bv.w);
        }
    }
}

// ---------------------------------------------------------------- K2: pack [x | cond | text | 0-pad] rows
// Rows are [branch][b][t]; branch 0 reads cat, branch 1 reads cat_drop.  only_x rewrites just the
// n_mel state columns (the per-step part); the conditioning columns are written once per call.
template <typename T>
__global__ __launch_bounds__(256) void pack_cat_kernel(const float* __restrict__ x, const float* __restrict__ cat,
                                                       const float* __restrict__ cat_drop, T* __restrict__ out, int ldo,
                                                       int BN, int n_mel, int cond_dim, int only_x,
                                                       const int* __restrict__ row_src) {
    const int cols4 = (only_x ? n_mel : ldo) >> 2;
    const size_t total = (size_t)2 * BN * cols4;
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (size_t)gridDim.x * 256) {
        const int c = (int)(i % cols4) * 4;
        const size_t row = i / cols4;
        size_t bt = row >= (size_t)BN ? row - BN : row;
        if (row_src) bt = (size_t)row_src[bt];               // packed rows: bt indexes the padded [B][N] inputs
        float4 v;
        if (c < n_mel) v = *(const float4*)(x + bt * n_mel + c);
        else if (c < n_mel + cond_dim) v = *(const float4*)((row >= (size_t)BN ? cat_drop : cat) + bt * cond_dim + (c - n_mel));
        else v = make_float4(0.f, 0.f, 0.f, 0.f);
        store4<T>(out + row * ldo + c, v.x, v.y, v.z, v.w);
    }
}

// N8: the same pack for a guided SUBSET, rows [row0, row0 + n_rows) of the packed buffer.  Conditional rows [0, Rc) read cat through
// row_src; unconditional row Rc + u exists only for a guided item and gathers cat_drop through u_src[u] (its padded [B][N] row).
// x_packed: x is the stage state [Rc][n_mel] (packed conditional rows): row r reads x[r], unconditional row u reads x[u_crow[u]].
template <typename T>
__global__ __launch_bounds__(256) void pack_cat_guided_kernel(const float* __restrict__ x, const float* __restrict__ cat,
                                                              const float* __restrict__ cat_drop, T* __restrict__ out, int ldo, int Rc,
                                                              int row0, int n_rows, int n_mel, int cond_dim, int only_x, int x_packed,
                                                              const int* __restrict__ row_src, const int* __restrict__ u_src,
                                                              const int* __restrict__ u_crow) {
    const int cols4 = (only_x ? n_mel : ldo) >> 2;
    const size_t total = (size_t)n_rows * cols4;
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (size_t)gridDim.x * 256) {
        const int c = (int)(i % cols4) * 4;
        const size_t row = (size_t)row0 + i / cols4;
        const bool unc = row >= (size_t)Rc;
        const size_t bt = unc ? (size_t)u_src[row - Rc] : (size_t)row_src[row];
        float4 v;
        if (c < n_mel) v = *(const float4*)(x + (x_packed ? (unc ? (size_t)u_crow[row - Rc] : row) : bt) * n_mel + c);
        else if (c < n_mel + cond_dim) v = *(const float4*)((unc ? cat_drop : cat) + bt * cond_dim + (c - n_mel));
        else v = make_float4(0.f, 0.f, 0.f, 0.f);
        store4<T>(out + row * ldo + c, v.x, v.y, v.z, v.w);
    }
}

// ---------------------------------------------------------------- K9: x += dt * (pc + cfg (pc - pu))
__global__ __launch_bounds__(256) void cfg_euler_kernel(float* __restrict__ x, const float* __restrict__ pred, int ldp,
                                                        int BN, int n_mel, float cfg, float dt, const int* __restrict__ row_src) {
    const int c4 = n_mel >> 2;
    const size_t total = (size_t)BN * c4;
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (size_t)gridDim.x * 256) {
        const int c = (int)(i % c4) * 4;
        const size_t row = i / c4;
        const float4 pc = *(const float4*)(pred + row * ldp + c);
        const float4 pu = *(const float4*)(pred + (row + BN) * ldp + c);
        const size_t xr = row_src ? (size_t)row_src[row] : row;
        float4 xv = *(float4*)(x + xr * n_mel + c);
        xv.x += dt * (pc.x + (pc.x - pu.x) * cfg);
        xv.y += dt * (pc.y + (pc.y - pu.y) * cfg);
        xv.z += dt * (pc.z + (pc.z - pu.z) * cfg);
        xv.w += dt * (pc.w + (pc.w - pu.w) * cfg);
        *(float4*)(x + xr * n_mel + c) = xv;
    }
}

// ---------------------------------------------------------------- N7: one stage of an explicit Runge-Kutta step
// k_i = pc + (pc - pu) g (the combine of cfg_euler_kernel, g per item through g_item[row_src[row] / seq_n] when given), stored to
// k_out when a later stage or the final sum reads it; then acc = x + sum_j c_j k_j over the earlier slopes (j ascending, k_prev[j]
// NULL = zero coefficient, skipped) and the fresh one (c_new, skipped when 0).  x_out != NULL: acc is the next stage's state (packed
// rows); x_out == NULL (last stage): x is updated in place through row_src.  The coefficients arrive multiplied by h.
// GUIDED (N8): the unconditional row of packed row r is pred row u_row[r] (an absolute row of pred, inside [BN, BN + Ru)); u_row[r] < 0:
// the item is not guided at this evaluation, it has no unconditional row and k_i = pc.  One body, so a mapped row runs the very
// arithmetic of the plain kernel.
// APG (N11): the item's strength is coef[b][0] = A_b in place of g (the combine is written exactly as the plain one), and where
// coef[b][1] = C_b != 0 the slope also takes C_b d, d = fmaf(1 - t_e, pc, x_e) the conditional data estimate at the state x_e the DiT was
// evaluated at (x through row_src, or the packed stage state when xe_packed) -- never the buffer x_out of the same launch.
// REUSE (N21, on top of GUIDED, never with APG): the guidance difference D = pc - pu of an item is kept in d_buf ([BN][n_mel] fp32, packed
// rows) between evaluations.  The mode of a row is its ITEM's (row_src[row] / seq_n, as g_item's), two bits that travel as kernel arguments
// (two GuideFlags; no table on the device): bit `load` -- the item has no unconditional row at this evaluation (u_row < 0) and
// k_i = pc + D g with D read from d_buf; bit `store` -- the item's D, formed from pred, is also written to d_buf because a later evaluation
// of the call reads it.  A row with u_row >= 0 is computed whatever `load` says; a row with u_row < 0 and no `load` bit is not guided, k_i =
// pc.  One body and one combine expression, so a computed row runs the very arithmetic of ode_stage_kernel<true, false>.
// NORM (N24, on top of GUIDED, never with APG or REUSE): coef[b] = {s, f} of cfg_norm_coef_kernel arrives where APG's coefficients do; a
// guided row's slope is k = f (pc + (pc - s pu) g) -- the plain combine with s pu in place of pu, then one multiplication.  s = 1 and f = 1
// are exact multiplications, fused or not: such an item runs the arithmetic of ode_stage_kernel<true, false>.  A row with u_row < 0 has
// k = pc and reads no coefficient.
struct OdeStagePrev { const float* k[3]; float c[3]; };
struct GuideFlags { unsigned w[VVK_GUIDE_MAX_ITEMS / 32]; };     // one bit per item of a launch, a kernel argument (N8; N21)
struct OdeStageReuse { float* d_buf; GuideFlags load, store; };
struct OdeStageNoReuse {};
template <bool GUIDED, bool APG, bool REUSE = false, bool NORM = false>
__global__ __launch_bounds__(256) void ode_stage_kernel(float* x, const float* __restrict__ pred, int ldp, int BN, int n_mel, float g,
                                                        const float* __restrict__ g_item, int seq_n, const int* __restrict__ row_src,
                                                        OdeStagePrev pv, float c_new, float* k_out, float* __restrict__ x_out,
                                                        const int* __restrict__ u_row, const float* __restrict__ apg_coef,
                                                        const float* x_e, int xe_packed, float omt,
                                                        std::conditional_t<REUSE, OdeStageReuse, OdeStageNoReuse> ru) {
    static_assert(!REUSE || (GUIDED && !APG), "the reuse form sits on the guided kernel and is never combined with APG");
    static_assert(!NORM || (GUIDED && !APG && !REUSE), "the CFG-Zero* / rescale form sits on the guided kernel and is never combined with APG or reuse");
    const int c4 = n_mel >> 2;
    const size_t total = (size_t)BN * c4;
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (size_t)gridDim.x * 256) {
        const int c = (int)(i % c4) * 4;
        const size_t row = i / c4;
        const float4 pc = *(const float4*)(pred + row * ldp + c);
        const size_t xr = row_src ? (size_t)row_src[row] : row;
        float cfg, apg_c = 0.f;
        if (APG) {
            const float2 ac = *(const float2*)(apg_coef + 2 * (xr / (size_t)seq_n));
            cfg = ac.x; apg_c = ac.y;
        } else {
            cfg = g_item ? g_item[xr / (size_t)seq_n] : g;
        }
        const int ur = GUIDED ? u_row[row] : 0;
        bool ru_load = false, ru_store = false;
        if constexpr (REUSE) {
            const unsigned item = (unsigned)(xr / (size_t)seq_n) & (VVK_GUIDE_MAX_ITEMS - 1);
            ru_load = ur < 0 && ((ru.load.w[item >> 5] >> (item & 31)) & 1u);
            ru_store = ur >= 0 && ((ru.store.w[item >> 5] >> (item & 31)) & 1u);
        }
        float4 k = pc;
        if (!GUIDED || ur >= 0 || ru_load) {
            float4 D;
            if constexpr (REUSE) {
                if (ru_load) D = *(const float4*)(ru.d_buf + row * n_mel + c);
            }
            float2 sf = {1.f, 1.f};
            if constexpr (NORM) sf = *(const float2*)(apg_coef + 2 * (xr / (size_t)seq_n));
            if (!ru_load) {
                const float4 pu = *(const float4*)(pred + (GUIDED ? (size_t)ur : row + BN) * ldp + c);
                if constexpr (NORM) {
                    D.x = pc.x - sf.x * pu.x; D.y = pc.y - sf.x * pu.y; D.z = pc.z - sf.x * pu.z; D.w = pc.w - sf.x * pu.w;
                } else {
                    D.x = pc.x - pu.x; D.y = pc.y - pu.y; D.z = pc.z - pu.z; D.w = pc.w - pu.w;
                }
            }
            k.x = pc.x + D.x * cfg;
            k.y = pc.y + D.y * cfg;
            k.z = pc.z + D.z * cfg;
            k.w = pc.w + D.w * cfg;
            if constexpr (NORM) { k.x *= sf.y; k.y *= sf.y; k.z *= sf.y; k.w *= sf.y; }
            if constexpr (REUSE) {
                if (ru_store) *(float4*)(ru.d_buf + row * n_mel + c) = D;
            }
            if (APG && apg_c != 0.f) {
                const float4 xe = *(const float4*)(x_e + (xe_packed ? row : xr) * n_mel + c);
                k.x = fmaf(apg_c, fmaf(omt, pc.x, xe.x), k.x);
                k.y = fmaf(apg_c, fmaf(omt, pc.y, xe.y), k.y);
                k.z = fmaf(apg_c, fmaf(omt, pc.z, xe.z), k.z);
                k.w = fmaf(apg_c, fmaf(omt, pc.w, xe.w), k.w);
            }
        }
        float4 xv = *(const float4*)(x + xr * n_mel + c);
#pragma unroll
        for (int j = 0; j < 3; ++j)
            if (pv.k[j]) {
                const float4 kj = *(const float4*)(pv.k[j] + row * n_mel + c);
                xv.x += pv.c[j] * kj.x; xv.y += pv.c[j] * kj.y; xv.z += pv.c[j] * kj.z; xv.w += pv.c[j] * kj.w;
            }
        // stored behind the loads of the earlier slopes: under a multistep plan (N20) k_out is the ring slot of the oldest slope this
        // launch reads, and each element is read and written by this thread alone
        if (k_out) *(float4*)(k_out + row * n_mel + c) = k;
        if (c_new != 0.f) {
            xv.x += c_new * k.x; xv.y += c_new * k.y; xv.z += c_new * k.z; xv.w += c_new * k.w;
        }
        *(float4*)(x_out ? x_out + row * n_mel + c : x + xr * n_mel + c) = xv;
    }
}

// ---------------------------------------------------------------- N11: projected guidance (APG), the per-item reduction
// Partial sums of one (frame tile, item): S1 = sum D d, S2 = sum d d, S3 = sum D D over the tile's valid frames and the n_mel columns,
// D = pc - pu, d = x_e + (1 - t_e) pc, formed and accumulated in float64 from the fp32 inputs.  Tiles are VV_APG_TILE frames counted from
// the ITEM's frame 0, and float4 q of the tile (frame q / c4, columns 4 (q % c4)) always goes to thread q % 256, its four elements in
// order, the threads' sums through one fixed LDS tree: an item's partials are a function of its own rows alone, whatever its place in
// the batch, its neighbours, N, the lanes or the guided subset.  A row whose u_row is < 0 contributes nothing (the coefficient kernel
// zeroes such an item).  grid (n_tiles, B); a tile past the item's length writes nothing and is never read.
__global__ __launch_bounds__(256) void apg_reduce_kernel(const float* __restrict__ pred, int ldp, int Rc, int n_mel,
                                                         const int* __restrict__ u_row, const float* __restrict__ x_e,
                                                         const int* __restrict__ row_src, const int* __restrict__ row_start,
                                                         const int* __restrict__ len, int n_tiles, double omt, double* __restrict__ partials) {
    __shared__ double red[3][256];
    const int b = blockIdx.y, tile = blockIdx.x;
    const int r0 = min(max(row_start[b], 0), Rc);
    const int n = min(min(max(len[b], 0), Rc - r0), n_tiles * VV_APG_TILE);   // inside the Rc conditional rows and the item's n_tiles partials, whatever the tables say
    const int f0 = tile * VV_APG_TILE;
    if (f0 >= n) return;
    const int c4 = n_mel >> 2;
    const int total = min(VV_APG_TILE, n - f0) * c4;
    double s1 = 0.0, s2 = 0.0, s3 = 0.0;
    for (int q = threadIdx.x; q < total; q += 256) {
        const int c = (q % c4) * 4;
        const size_t row = (size_t)r0 + f0 + q / c4;
        const int ur = u_row ? u_row[row] : (int)row + Rc;
        if (ur < 0) continue;
        const float4 pc = *(const float4*)(pred + row * ldp + c);
        const float4 pu = *(const float4*)(pred + (size_t)ur * ldp + c);
        const float4 xe = *(const float4*)(x_e + (row_src ? (size_t)row_src[row] : row) * n_mel + c);
        const float pcv[4] = {pc.x, pc.y, pc.z, pc.w}, puv[4] = {pu.x, pu.y, pu.z, pu.w}, xev[4] = {xe.x, xe.y, xe.z, xe.w};
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const double D = (double)pcv[j] - (double)puv[j];
            const double d = fma(omt, (double)pcv[j], (double)xev[j]);
            s1 = fma(D, d, s1); s2 = fma(d, d, s2); s3 = fma(D, D, s3);
        }
    }
    red[0][threadIdx.x] = s1; red[1][threadIdx.x] = s2; red[2][threadIdx.x] = s3;
    __syncthreads();
    for (int w = 128; w > 0; w >>= 1) {
        if ((int)threadIdx.x < w) {
            red[0][threadIdx.x] += red[0][threadIdx.x + w];
            red[1][threadIdx.x] += red[1][threadIdx.x + w];
            red[2][threadIdx.x] += red[2][threadIdx.x + w];
        }
        __syncthreads();
    }
    if (threadIdx.x < 3) partials[((size_t)b * n_tiles + tile) * 3 + threadIdx.x] = red[threadIdx.x][0];
}

// One wave per item: lane j < 3 adds the item's partials S_{j+1} in ascending tile order, lane 0 turns them into coef[b] = {A, C} (float64,
// one fp32 rounding each):  s = r / ((1 - t_e) sqrt(S3 / n)) where r > 0 and that RMS exceeds it, else 1;  A = g s;
// C = g s (eta - 1) S1 / S2, 0 when S2 == 0.  {0, 0} for an item without rows or whose first row is not guided (u_row < 0).
__global__ __launch_bounds__(64) void apg_coef_kernel(const double* __restrict__ partials, int n_tiles, int Rc, int n_mel,
                                                      const int* __restrict__ u_row, const int* __restrict__ row_start,
                                                      const int* __restrict__ len, double omt, float g, const float* __restrict__ g_item,
                                                      const float* __restrict__ eta, const float* __restrict__ norm_rms,
                                                      float* __restrict__ coef) {
    const int b = blockIdx.x, lane = threadIdx.x;
    const int r0 = min(max(row_start[b], 0), Rc);
    const int n = min(min(max(len[b], 0), Rc - r0), n_tiles * VV_APG_TILE);
    const bool guided = n > 0 && (!u_row || u_row[r0] >= 0);
    double s = 0.0;
    if (guided && lane < 3) {
        const int nt = (n + VV_APG_TILE - 1) / VV_APG_TILE;
        for (int t = 0; t < nt; ++t) s += partials[((size_t)b * n_tiles + t) * 3 + lane];
    }
    const double S1 = __shfl(s, 0), S2 = __shfl(s, 1), S3 = __shfl(s, 2);
    if (lane != 0) return;
    float A = 0.f, Cc = 0.f;
    if (guided) {
        const double gb = (double)(g_item ? g_item[b] : g), e = eta ? (double)eta[b] : 1.0, r = norm_rms ? (double)norm_rms[b] : 0.0;
        const double rms = omt * sqrt(S3 / ((double)n * (double)n_mel));
        const double sc = (r > 0.0 && rms > r) ? r / rms : 1.0;
        A = (float)(gb * sc);
        Cc = (e == 1.0 || S2 == 0.0) ? 0.f : (float)(gb * sc * (e - 1.0) * S1 / S2);
    }
    coef[2 * b] = A; coef[2 * b + 1] = Cc;
}

// ---------------------------------------------------------------- N24: CFG-Zero* and guidance rescale, the per-item Gram sums
// Partial sums of one (frame tile, item) over the tile's valid frames and the n_mel columns of the fp32 predictions, in this order:
// S_cu = sum pc pu, S_uu = sum pu pu, S_cc = sum pc pc, S_c = sum pc, S_u = sum pu.  Products and sums in float64 and NOT contracted (a
// product, then an add: what a host mirror does with numpy alone).  apg_reduce_kernel's determinism contract: tiles of VV_APG_TILE frames
// counted from the ITEM's frame 0, float4 q of the tile to thread q % 256 with its four elements in order, one fixed LDS tree -- an item's
// partials are a function of its own rows alone.  A row whose u_row is < 0 contributes nothing (the coefficient kernel writes {1, 1} for
// such an item); columns >= n_mel of an ldp-wide row are never read.  grid (n_tiles, B); a tile past the item's length writes nothing.
__global__ __launch_bounds__(256) void cfg_gram_reduce_kernel(const float* __restrict__ pred, int ldp, int Rc, int n_mel,
                                                              const int* __restrict__ u_row, const int* __restrict__ row_start,
                                                              const int* __restrict__ len, int n_tiles, double* __restrict__ partials) {
#pragma clang fp contract(off)
    __shared__ double red[5][256];
    const int b = blockIdx.y, tile = blockIdx.x;
    const int r0 = min(max(row_start[b], 0), Rc);
    const int n = min(min(max(len[b], 0), Rc - r0), n_tiles * VV_APG_TILE);   // inside the Rc conditional rows and the item's n_tiles partials, whatever the tables say
    const int f0 = tile * VV_APG_TILE;
    if (f0 >= n) return;
    const int c4 = n_mel >> 2;
    const int total = min(VV_APG_TILE, n - f0) * c4;
    double s[5] = {0.0, 0.0, 0.0, 0.0, 0.0};
    for (int q = threadIdx.x; q < total; q += 256) {
        const int c = (q % c4) * 4;
        const size_t row = (size_t)r0 + f0 + q / c4;
        const int ur = u_row ? u_row[row] : (int)row + Rc;
        if (ur < 0) continue;
        const float4 pc = *(const float4*)(pred + row * ldp + c);
        const float4 pu = *(const float4*)(pred + (size_t)ur * ldp + c);
        const float pcv[4] = {pc.x, pc.y, pc.z, pc.w}, puv[4] = {pu.x, pu.y, pu.z, pu.w};
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const double vc = (double)pcv[j], vu = (double)puv[j];
            const double cu = vc * vu, uu = vu * vu, cc = vc * vc;
            s[0] = s[0] + cu; s[1] = s[1] + uu; s[2] = s[2] + cc; s[3] = s[3] + vc; s[4] = s[4] + vu;
        }
    }
#pragma unroll
    for (int j = 0; j < 5; ++j) red[j][threadIdx.x] = s[j];
    __syncthreads();
    for (int w = 128; w > 0; w >>= 1) {
        if ((int)threadIdx.x < w) {
#pragma unroll
            for (int j = 0; j < 5; ++j) red[j][threadIdx.x] += red[j][threadIdx.x + w];
        }
        __syncthreads();
    }
    if (threadIdx.x < 5) partials[((size_t)b * n_tiles + tile) * 5 + threadIdx.x] = red[threadIdx.x][0];
}

// One wave per item: lane j < 5 adds the item's partials in ascending tile order from 0.0, lane 0 turns them into coef[b] = {s, f} (float64,
// not contracted, one fp32 rounding each):  s = S_cu / S_uu where star[b] != 0 and S_uu != 0, else 1;  with a = 1 + g, c = -g s (s the fp32
// value), V_xy = S_xy / n - (S_x / n)(S_y / n), var_k = a a V_cc + 2 a c V_cu + c c V_uu:  rho = sqrt(V_cc / var_k), 1 unless both are
// > 0;  f = phi rho + (1 - phi), exactly 1 where phi = rescale[b] is 0.  {1, 1} for an item without rows or whose first row is not guided
// (u_row < 0).  report (optional): the same pair once more, the caller's [B][2] row of this evaluation.
__global__ __launch_bounds__(64) void cfg_norm_coef_kernel(const double* __restrict__ partials, int n_tiles, int Rc, int n_mel,
                                                           const int* __restrict__ u_row, const int* __restrict__ row_start,
                                                           const int* __restrict__ len, float g, const float* __restrict__ g_item,
                                                           const float* __restrict__ star, const float* __restrict__ rescale,
                                                           float* __restrict__ coef, float* __restrict__ report) {
#pragma clang fp contract(off)
    const int b = blockIdx.x, lane = threadIdx.x;
    const int r0 = min(max(row_start[b], 0), Rc);
    const int n = min(min(max(len[b], 0), Rc - r0), n_tiles * VV_APG_TILE);
    const bool guided = n > 0 && (!u_row || u_row[r0] >= 0);
    double acc = 0.0;
    if (guided && lane < 5) {
        const int nt = (n + VV_APG_TILE - 1) / VV_APG_TILE;
        for (int t = 0; t < nt; ++t) acc += partials[((size_t)b * n_tiles + t) * 5 + lane];
    }
    const double Scu = __shfl(acc, 0), Suu = __shfl(acc, 1), Scc = __shfl(acc, 2), Sc = __shfl(acc, 3), Su = __shfl(acc, 4);
    if (lane != 0) return;
    float s = 1.f, f = 1.f;
    if (guided) {
        if (star && star[b] != 0.f && Suu != 0.0) s = (float)(Scu / Suu);
        const double phi = rescale ? (double)rescale[b] : 0.0;
        if (phi != 0.0) {
            const double gb = (double)(g_item ? g_item[b] : g), a = 1.0 + gb, c = -gb * (double)s;
            const double cnt = (double)n * (double)n_mel, mc = Sc / cnt, mu = Su / cnt;
            const double Vcc = Scc / cnt - mc * mc, Vcu = Scu / cnt - mc * mu, Vuu = Suu / cnt - mu * mu;
            const double var_k = (a * a) * Vcc + (2.0 * a * c) * Vcu + (c * c) * Vuu;
            const double rho = (var_k > 0.0 && Vcc > 0.0) ? sqrt(Vcc / var_k) : 1.0;
            f = (float)(phi * rho + (1.0 - phi));
        }
    }
    coef[2 * b] = s; coef[2 * b + 1] = f;
    if (report) { report[2 * b] = s; report[2 * b + 1] = f; }
}

// ---------------------------------------------------------------- N20: the step report of a multistep plan, the per-item reduction
// Partial sums of one (frame tile, item): D2 = sum (f - f_prev)^2 and F2 = sum f^2 over the tile's valid frames and the n_mel columns of
// the packed slopes f and f_prev ([Rc][n_mel] fp32), every difference, square and sum in float64 and NOT contracted (a product, then an
// add: what a host mirror does with numpy alone).  f_prev NULL (step 0): D2 = 0.  apg_reduce_kernel's determinism contract: tiles of
// VV_APG_TILE frames counted from the ITEM's frame 0, float4 q of the tile to thread q % 256 with its four elements in order, one fixed
// LDS tree -- an item's partials are a function of its own rows alone.  grid (n_tiles, B); a tile past the item's length writes nothing.
__global__ __launch_bounds__(256) void ode_diff_reduce_kernel(const float* __restrict__ f, const float* __restrict__ f_prev, int Rc, int n_mel,
                                                              const int* __restrict__ row_start, const int* __restrict__ len, int n_tiles,
                                                              double* __restrict__ partials) {
#pragma clang fp contract(off)
    __shared__ double red[2][256];
    const int b = blockIdx.y, tile = blockIdx.x;
    const int r0 = min(max(row_start[b], 0), Rc);
    const int n = min(min(max(len[b], 0), Rc - r0), n_tiles * VV_APG_TILE);   // inside the Rc rows and the item's n_tiles partials, whatever the tables say
    const int f0 = tile * VV_APG_TILE;
    if (f0 >= n) return;
    const int c4 = n_mel >> 2;
    const int total = min(VV_APG_TILE, n - f0) * c4;
    double s1 = 0.0, s2 = 0.0;
    for (int q = threadIdx.x; q < total; q += 256) {
        const size_t at = ((size_t)r0 + f0 + q / c4) * n_mel + (q % c4) * 4;
        const float4 a = *(const float4*)(f + at);
        const float av[4] = {a.x, a.y, a.z, a.w};
        float pv[4] = {0.f, 0.f, 0.f, 0.f};
        if (f_prev) {
            const float4 p = *(const float4*)(f_prev + at);
            pv[0] = p.x; pv[1] = p.y; pv[2] = p.z; pv[3] = p.w;
        }
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const double v = (double)av[j];
            if (f_prev) {
                const double d = v - (double)pv[j];
                const double dd = d * d;
                s1 = s1 + dd;
            }
            const double vv = v * v;
            s2 = s2 + vv;
        }
    }
    red[0][threadIdx.x] = s1; red[1][threadIdx.x] = s2;
    __syncthreads();
    for (int w = 128; w > 0; w >>= 1) {
        if ((int)threadIdx.x < w) {
            red[0][threadIdx.x] += red[0][threadIdx.x + w];
            red[1][threadIdx.x] += red[1][threadIdx.x + w];
        }
        __syncthreads();
    }
    if (threadIdx.x < 2) partials[((size_t)b * n_tiles + tile) * 2 + threadIdx.x] = red[threadIdx.x][0];
}

// One wave per item: lane j < 2 adds the item's partials in ascending tile order from 0.0 and stores report[b] = {D2, F2}; {0, 0} for an
// item without rows.
__global__ __launch_bounds__(64) void ode_diff_finish_kernel(const double* __restrict__ partials, int n_tiles, int Rc,
                                                             const int* __restrict__ row_start, const int* __restrict__ len,
                                                             double* __restrict__ report) {
    const int b = blockIdx.x, lane = threadIdx.x;
    if (lane >= 2) return;
    const int r0 = min(max(row_start[b], 0), Rc);
    const int n = min(min(max(len[b], 0), Rc - r0), n_tiles * VV_APG_TILE);
    const int nt = (n + VV_APG_TILE - 1) / VV_APG_TILE;
    double s = 0.0;
    for (int t = 0; t < nt; ++t) s += partials[((size_t)b * n_tiles + t) * 2 + lane];
    report[2 * b + lane] = s;
}

// ---------------------------------------------------------------- N21: the drift report of guidance reuse, the per-item reduction
// Partial sums of one (frame tile, item): E2 = sum (D_new - D_old)^2 and N2 = sum D_new^2 over the tile's valid frames and the n_mel columns,
// D_new = pc - pu the fp32 difference the stage kernel forms from pred through u_row (one fp32 subtraction: the value it stores), D_old the
// row of d_buf.  Differences of the two, squares and sums in float64 and NOT contracted (a product, then an add).  A row whose u_row is < 0
// (its item reuses or is not guided here) contributes nothing, so such an item's sums are {0, 0}; an item whose bit of `has_old` is clear
// (no difference stored yet in this call) does not read d_buf and E2 = 0.  ode_diff_reduce_kernel's determinism contract: tiles of
// VV_APG_TILE frames counted from the ITEM's frame 0, float4 q of the tile to thread q % 256 with its four elements in order, one fixed LDS
// tree -- an item's partials are a function of its own rows alone.  grid (n_tiles, B); a tile past the item's length writes nothing.  It
// runs BEFORE the stage launch that overwrites d_buf.  The item sums are ode_diff_finish_kernel's.
__global__ __launch_bounds__(256) void cfg_drift_reduce_kernel(const float* __restrict__ pred, int ldp, int Rc, int n_mel,
                                                               const int* __restrict__ u_row, const float* __restrict__ d_buf, GuideFlags has_old,
                                                               const int* __restrict__ row_start, const int* __restrict__ len, int n_tiles,
                                                               double* __restrict__ partials) {
#pragma clang fp contract(off)
    __shared__ double red[2][256];
    const int b = blockIdx.y, tile = blockIdx.x;
    const int r0 = min(max(row_start[b], 0), Rc);
    const int n = min(min(max(len[b], 0), Rc - r0), n_tiles * VV_APG_TILE);   // inside the Rc rows and the item's n_tiles partials, whatever the tables say
    const int f0 = tile * VV_APG_TILE;
    if (f0 >= n) return;
    const bool old = (has_old.w[b >> 5] >> (b & 31)) & 1u;
    const int c4 = n_mel >> 2;
    const int total = min(VV_APG_TILE, n - f0) * c4;
    double s1 = 0.0, s2 = 0.0;
    for (int q = threadIdx.x; q < total; q += 256) {
        const int c = (q % c4) * 4;
        const size_t row = (size_t)r0 + f0 + q / c4;
        const int ur = u_row[row];
        if (ur < 0) continue;
        const float4 pc = *(const float4*)(pred + row * ldp + c);
        const float4 pu = *(const float4*)(pred + (size_t)ur * ldp + c);
        const float dn[4] = {pc.x - pu.x, pc.y - pu.y, pc.z - pu.z, pc.w - pu.w};
        float dv[4] = {0.f, 0.f, 0.f, 0.f};
        if (old) {
            const float4 p = *(const float4*)(d_buf + row * n_mel + c);
            dv[0] = p.x; dv[1] = p.y; dv[2] = p.z; dv[3] = p.w;
        }
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const double v = (double)dn[j];
            if (old) {
                const double d = v - (double)dv[j];
                const double dd = d * d;
                s1 = s1 + dd;
            }
            const double vv = v * v;
            s2 = s2 + vv;
        }
    }
    red[0][threadIdx.x] = s1; red[1][threadIdx.x] = s2;
    __syncthreads();
    for (int w = 128; w > 0; w >>= 1) {
        if ((int)threadIdx.x < w) {
            red[0][threadIdx.x] += red[0][threadIdx.x + w];
            red[1][threadIdx.x] += red[1][threadIdx.x + w];
        }
        __syncthreads();
    }
    if (threadIdx.x < 2) partials[((size_t)b * n_tiles + tile) * 2 + threadIdx.x] = red[threadIdx.x][0];
}

// ---------------------------------------------------------------- N23: block caching, the span kernels
// X = the fp32 residual stream at a block boundary, formed per element as ln_mod_kernel forms it: (x + (float)d1) + (float)d2 with the two
// pending deltas of the block in front (fp32 adds, in this order), or plain x when nothing is pending (d1 NULL).  Over n4 float4s of the
// contiguous [R][D] planes:
//   MARK   buf = X                (x and the deltas are read only)
//   DIFF   buf = X - buf          (one fp32 subtraction: the span's contribution, X at its end less X at its start)
//   APPLY  x   = X + buf          (one fp32 add: the stored contribution in place of the span's blocks; buf is read only)
// Flat, float4, grid-stride with size_t indices: every element is read and written by one thread.  The planes are far larger than the
// caches and each is touched once per evaluation: non-temporal loads and stores, as ln_mod_kernel's.  No LDS, no atomics.
template <typename Td, int MODE>
__global__ __launch_bounds__(256) void block_span_kernel(float* x, const Td* __restrict__ d1, const Td* __restrict__ d2, float* buf, size_t n4) {
    const size_t stride = (size_t)gridDim.x * 256;
    for (size_t q = (size_t)blockIdx.x * 256 + threadIdx.x; q < n4; q += stride) {
        float4 v = load4_nt<float>(x + q * 4);
        if (d1) {
            const float4 a = load4_nt<Td>(d1 + q * 4);
            v.x += a.x; v.y += a.y; v.z += a.z; v.w += a.w;
            if (d2) {
                const float4 b = load4_nt<Td>(d2 + q * 4);
                v.x += b.x; v.y += b.y; v.z += b.z; v.w += b.w;
            }
        }
        if (MODE == VV_SPAN_MARK) {
            store4_nt<float>(buf + q * 4, v.x, v.y, v.z, v.w);
        } else {
            const float4 s = load4_nt<float>(buf + q * 4);
            if (MODE == VV_SPAN_DIFF) store4_nt<float>(buf + q * 4, v.x - s.x, v.y - s.y, v.z - s.z, v.w - s.w);
            else store4_nt<float>(x + q * 4, v.x + s.x, v.y + s.y, v.z + s.z, v.w + s.w);
        }
    }
}

// ---------------------------------------------------------------- N23: the drift report of block caching, the per-sequence reduction
// Partial sums of one (frame tile, sequence): E2 = sum (d_new - d_prev)^2 and N2 = sum d_new^2 over the tile's valid frames and the D columns
// of two stored contributions ([R][D] fp32).  Sequence s owns the rows [row_start[s], + len[s]) -- one CFG branch of one item.  d_prev NULL
// (the first store of a call): E2 = 0.  Differences, squares and sums in float64 and NOT contracted.  cfg_drift_reduce_kernel's determinism
// contract: tiles of VV_APG_TILE frames counted from the SEQUENCE's frame 0, float4 q of the tile to thread q % 256 with its four elements in
// order, one fixed LDS tree -- a sequence's partials are a function of its own rows alone.  grid (n_tiles, n_seq); a tile past the length
// writes nothing.
__global__ __launch_bounds__(256) void block_drift_reduce_kernel(const float* __restrict__ d_new, const float* __restrict__ d_prev, int R, int D,
                                                                 const int* __restrict__ row_start, const int* __restrict__ len, int n_tiles,
                                                                 double* __restrict__ partials) {
#pragma clang fp contract(off)
    __shared__ double red[2][256];
    const int s = blockIdx.y, tile = blockIdx.x;
    const int r0 = min(max(row_start[s], 0), R);
    const int n = min(min(max(len[s], 0), R - r0), n_tiles * VV_APG_TILE);    // inside the R rows and the sequence's n_tiles partials, whatever the tables say
    const int f0 = tile * VV_APG_TILE;
    if (f0 >= n) return;
    const int c4 = D >> 2;
    const int total = min(VV_APG_TILE, n - f0) * c4;
    double s1 = 0.0, s2 = 0.0;
    for (int q = threadIdx.x; q < total; q += 256) {
        const size_t at = ((size_t)r0 + f0 + q / c4) * D + (q % c4) * 4;
        const float4 a = load4_nt<float>(d_new + at);
        const float av[4] = {a.x, a.y, a.z, a.w};
        float pv[4] = {0.f, 0.f, 0.f, 0.f};
        if (d_prev) {
            const float4 p = load4_nt<float>(d_prev + at);
            pv[0] = p.x; pv[1] = p.y; pv[2] = p.z; pv[3] = p.w;
        }
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const double v = (double)av[j];
            if (d_prev) {
                const double d = v - (double)pv[j];
                const double dd = d * d;
                s1 = s1 + dd;
            }
            const double vv = v * v;
            s2 = s2 + vv;
        }
    }
    red[0][threadIdx.x] = s1; red[1][threadIdx.x] = s2;
    __syncthreads();
    for (int w = 128; w > 0; w >>= 1) {
        if ((int)threadIdx.x < w) {
            red[0][threadIdx.x] += red[0][threadIdx.x + w];
            red[1][threadIdx.x] += red[1][threadIdx.x + w];
        }
        __syncthreads();
    }
    if (threadIdx.x < 2) partials[((size_t)s * n_tiles + tile) * 2 + threadIdx.x] = red[threadIdx.x][0];
}

// One wave per sequence: lane j < 2 adds the sequence's partials in ascending tile order from 0.0 and stores them at the report's
// [item][branch][2] place: item = s % n_items, branch = branch0 + s / n_items.  {0, 0} for a sequence without rows, and for every sequence
// when n_tiles is 0 (an evaluation that stores nothing: the partials are not read).
__global__ __launch_bounds__(64) void block_drift_finish_kernel(const double* __restrict__ partials, int n_tiles, int R,
                                                                const int* __restrict__ row_start, const int* __restrict__ len, int n_items,
                                                                int branch0, double* __restrict__ report) {
    const int s = blockIdx.x, lane = threadIdx.x;
    if (lane >= 2) return;
    const int r0 = min(max(row_start[s], 0), R);
    const int n = min(min(max(len[s], 0), R - r0), n_tiles * VV_APG_TILE);
    const int nt = (n + VV_APG_TILE - 1) / VV_APG_TILE;
    double sum = 0.0;
    for (int t = 0; t < nt; ++t) sum += partials[((size_t)s * n_tiles + t) * 2 + lane];
    report[((size_t)(s % n_items) * 2 + (branch0 + s / n_items)) * 2 + lane] = sum;
}

// ---------------------------------------------------------------- text: embed gather + position table
// Sequence s in [0, 2B): b = s % B, drop branch when s >= B (all filler ids).  Token t of the
// text is id+1; beyond the text (or the sequence) the filler id 0.
__global__ __launch_bounds__(256) void text_embed_kernel(const int* __restrict__ ids, int ld_ids,
                                                         const int* __restrict__ text_len, const float* __restrict__ emb,
                                                         const float* __restrict__ pos, float* __restrict__ out, int B,
                                                         int N, int Dt, int vocab_rows) {
    const int c4 = Dt >> 2;
    const size_t total = (size_t)2 * B * N * c4;
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (size_t)gridDim.x * 256) {
        const int c = (int)(i % c4) * 4;
        const size_t row = i / c4;
        const int t = (int)(row % N);
        const int s = (int)(row / N);
        const int b = s % B;
        int id = 0;
        if (s < B && t < text_len[b] && t < ld_ids) id = ids[(size_t)b * ld_ids + t] + 1;
        id = min(max(id, 0), vocab_rows - 1);
        const float4 e = *(const float4*)(emb + (size_t)id * Dt + c);
        const float4 p = *(const float4*)(pos + (size_t)t * Dt + c);
        *(float4*)(out + row * Dt + c) = make_float4(e.x + p.x, e.y + p.y, e.z + p.z, e.w + p.w);
    }
}

// depthwise conv k=KW along tokens, token-major [seq][t][c]; zero beyond [0, len)
__global__ __launch_bounds__(256) void dwconv_kernel(const float* __restrict__ in, float* __restrict__ out,
                                                     const float* __restrict__ w /*[C][KW]*/, const float* __restrict__ bias,
                                                     const int* __restrict__ seq_len, int B, int n_seq, int N, int C, int KW) {
    const int c4 = C >> 2;
    const size_t total = (size_t)n_seq * N * c4;
    const int pad = KW / 2;
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (size_t)gridDim.x * 256) {
        const int c = (int)(i % c4) * 4;
        const size_t row = i / c4;
        const int t = (int)(row % N);
        const int s = (int)(row / N);
        const int len = seq_len ? min(seq_len[s % B], N) : N;
        float4 acc = *(const float4*)(bias + c);
        for (int k = 0; k < KW; ++k) {
            const int tt = t + k - pad;
            if (tt < 0 || tt >= len) continue;
            const float4 v = *(const float4*)(in + ((size_t)s * N + tt) * C + c);
            acc.x += w[(c + 0) * KW + k] * v.x;
            acc.y += w[(c + 1) * KW + k] * v.y;
            acc.z += w[(c + 2) * KW + k] * v.z;
            acc.w += w[(c + 3) * KW + k] * v.w;
        }
        *(float4*)(out + row * C + c) = acc;
    }
}

// GRN statistics: sumsq[s][c] over valid tokens.  grid (C/64, n_seq), block 256 = 4 token phases x 64 channels
template <typename T>
__global__ __launch_bounds__(256) void grn_stats_kernel(const T* __restrict__ x, float* __restrict__ sumsq,
                                                        const int* __restrict__ seq_len, int B, int N, int C) {
    __shared__ float red[256];
    const int s = blockIdx.y;
    const int c = blockIdx.x * 64 + (threadIdx.x & 63);
    const int ph = threadIdx.x >> 6;
    const int len = seq_len ? min(seq_len[s % B], N) : N;
    float acc = 0.f;
    for (int t = ph; t < len; t += 4) {
        const float v = to_f32<T>(x[((size_t)s * N + t) * C + c]);
        acc += v * v;
    }
    red[threadIdx.x] = acc;
    __syncthreads();
    if (ph == 0) sumsq[(size_t)s * C + c] = (red[threadIdx.x] + red[threadIdx.x + 64]) + (red[threadIdx.x + 128] + red[threadIdx.x + 192]);
}

// GRN apply: y = gamma * (x * nx) + beta + x, nx = g / (mean_c g + 1e-6), g = sqrt(sumsq).  In place.
template <typename T>
__global__ __launch_bounds__(256) void grn_apply_kernel(T* __restrict__ x, const float* __restrict__ sumsq,
                                                        const float* __restrict__ gamma, const float* __restrict__ beta,
                                                        int N, int C, int rows_per_block) {
#ifndef VV_ELEMENTWISE_HOST_CHECK
    extern __shared__ float sc[];      // [C] scale = gamma*nx + 1
#else
    float* sc = (float*)vv_host::dynamic_lds();
#endif
    __shared__ float red[4];
    const int s = blockIdx.y;
    float part = 0.f;
    for (int c = threadIdx.x; c < C; c += 256) part += sqrtf(sumsq[(size_t)s * C + c]);
    part = wave_sum(part);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = part;
    __syncthreads();
    const float mean = ((red[0] + red[1]) + (red[2] + red[3])) / (float)C;
    for (int c = threadIdx.x; c < C; c += 256) sc[c] = gamma[c] * (sqrtf(sumsq[(size_t)s * C + c]) / (mean + 1e-6f)) + 1.0f;
    __syncthreads();
    const int t0 = blockIdx.x * rows_per_block;
    const int c4 = C >> 2;
    for (int i = threadIdx.x; i < rows_per_block * c4; i += 256) {
        const int t = t0 + i / c4;
        if (t >= N) break;
        const int c = (i % c4) * 4;
        T* p = x + ((size_t)s * N + t) * C + c;
        const float4 v = load4<T>(p);
        const float4 bb = *(const float4*)(beta + c);
        store4<T>(p, v.x * sc[c] + bb.x, v.y * sc[c + 1] + bb.y, v.z * sc[c + 2] + bb.z, v.w * sc[c + 3] + bb.w);
    }
}

// conditioning: cat[b][t] = [mel (t < ref_len) | text(b)], cat_drop[b][t] = [0 | text(B+b)]
// MASKED (speech editing, vv_edit.hip): the mel only where keep[b][t] as well -- a frame mask in place of the prefix
template <bool MASKED>
__global__ __launch_bounds__(256) void build_cat_kernel(const float* __restrict__ mel, int F_max,
                                                        const int* __restrict__ ref_len, const float* __restrict__ text,
                                                        float* __restrict__ cat, float* __restrict__ cat_drop, int B, int N,
                                                        int n_mel, int Dt, const uint8_t* __restrict__ keep, int ld_keep) {
    const int cd = n_mel + Dt;
    const int c4 = cd >> 2;
    const size_t total = (size_t)B * N * c4;
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (size_t)gridDim.x * 256) {
        const int c = (int)(i % c4) * 4;
        const size_t row = i / c4;
        const int t = (int)(row % N);
        const int b = (int)(row / N);
        float4 v, vd;
        if (c < n_mel) {
            v = (t < ref_len[b] && t < F_max && (!MASKED || keep[(size_t)b * ld_keep + t])) ? *(const float4*)(mel + ((size_t)b * F_max + t) * n_mel + c)
                                               : make_float4(0.f, 0.f, 0.f, 0.f);
            vd = make_float4(0.f, 0.f, 0.f, 0.f);
        } else {
            v = *(const float4*)(text + row * Dt + (c - n_mel));
            vd = *(const float4*)(text + ((size_t)B * N + row) * Dt + (c - n_mel));
        }
        *(float4*)(cat + row * cd + c) = v;
        *(float4*)(cat_drop + row * cd + c) = vd;
    }
}

// small integer helpers (lengths live on the device so that batches need no host round trip)
__global__ void ref_len_kernel(const int* __restrict__ audio_len, int* __restrict__ ref_len, int B, int hop) {
    const int b = blockIdx.x * 64 + threadIdx.x;
    if (b < B) ref_len[b] = audio_len[b] / hop + 1;      // reference core/tts_engine.py:55
}
__global__ void decode_len_kernel(const int* __restrict__ seq_len, const int* __restrict__ ref_len, int* __restrict__ lens,
                                  int B, int n_levels, const int* __restrict__ mult, int N, int T_max) {
    // lens[level][b] = tg * mult[level], tg = the frames mel_slice_kernel hands to the first level: the slice [ref_len, seq_len) with
    // both ends clamped into the item's N rows, and at most the T_max columns of the level-0 plane.  The last level is pcm_len: a
    // device length that disagrees with the host's (stale tensor) never describes more samples than a pcm row holds.
    const int b = blockIdx.x * 64 + threadIdx.x;
    if (b >= B) return;
    const int sl = max(min(seq_len[b], N), 0);
    const int tg = min(sl - min(max(ref_len[b], 0), sl), T_max);
    for (int l = 0; l < n_levels; ++l) lens[l * B + b] = tg * mult[l];
}

// Packed-row tables of one vv_transformer_steps call, built on the device from the per-item lengths (one workgroup per item):
//   row_start[2B] (conditional branch first), row_src[Rc] = b * N + t, row_pos[2 Rc] = t.
//   kv_len[2B]: the lengths attention and posconv run on, both branches -- the SAME clamped lengths the tables are built from.
__global__ __launch_bounds__(256) void row_tables_kernel(const int* __restrict__ seq_len, int B, int N, int Rc, int* __restrict__ row_start,
                                                         int* __restrict__ row_src, int* __restrict__ row_pos, int* __restrict__ kv_len) {
    // The table sizes (Rc, 2 Rc) and every launch shape come from the HOST copy of the lengths; the device copy is clamped to
    // [0, N] and to the Rc rows that exist, so a device array that disagrees with the host one (stale tensor, wrong batch) cannot
    // write past the tables -- it produces wrong audio for that call, never a stray store.  When the device lengths sum to MORE
    // rows than Rc, the items past the Rc-th row get a shorter or a zero length (kv_len carries the clamped value, so every row
    // [row_start, +kv_len) the block kernels address lies below Rc in its branch; a zero-length item owns no row).  When they sum to FEWER
    // rows than the host's Rc, the last workgroup maps the rows nobody owns onto the PADDING rows of the last item (the rows of
    // x / cat right after its device length, clamped to N - 1), so the gathers and the read-modify-write of cfg_euler through
    // row_src never see an unwritten index and never touch a valid row of any item.
    const int b = blockIdx.x;
    int r0 = 0;
    for (int i = 0; i < b; ++i) r0 += min(max(seq_len[i], 0), N);   // B is at most a few hundred: a serial prefix per workgroup is cheaper than a scan
    r0 = min(r0, Rc);
    const int len = min(min(max(seq_len[b], 0), N), Rc - r0);
    if (threadIdx.x == 0) { row_start[b] = r0; row_start[B + b] = Rc + r0; kv_len[b] = len; kv_len[B + b] = len; }
    for (int t = threadIdx.x; t < len; t += 256) {
        row_src[r0 + t] = b * N + t;
        row_pos[r0 + t] = t;
        row_pos[Rc + r0 + t] = t;
    }
    if (b == B - 1)
        for (int t = r0 + len + (int)threadIdx.x; t < Rc; t += 256) {
            const int p = min(len + (t - (r0 + len)), N - 1);
            row_src[t] = b * N + p;
            row_pos[t] = p;
            row_pos[Rc + t] = p;
        }
}

// N8: the tables of one evaluation whose unconditional half covers only the GUIDED items (bit b of `flags`), one workgroup per item.
// Conditional entries are row_tables_kernel's; the unconditional rows of the guided items are compacted to [Rc, Rc + Ru) in item order
// and their sequences to entries [B, B + Bu):
//   row_start[B + j] = Rc + u0, rs_rel[j] = u0 (the same, relative to the unconditional half), kv_len[B + j], row_pos[Rc + u],
//   u_src[Ru]: unconditional row -> padded [B][N] row, u_crow[Ru]: -> its conditional packed row,
//   u_row[Rc]: conditional packed row -> its unconditional packed row Rc + u, or -1.
// Rc and Ru come from the HOST lengths and flags; the device lengths are clamped as in row_tables_kernel and once more to the Ru rows
// that exist, so device lengths that disagree with the host's never index past a table: a guided item past the Ru-th row gets a shorter
// or empty unconditional sequence (its remaining rows are unguided, u_row -1), and rows of either half that nobody owns map onto the
// padding rows of the last item.
__global__ __launch_bounds__(256) void guided_tables_kernel(const int* __restrict__ seq_len, GuideFlags flags, int B, int N, int Rc, int Ru,
                                                            int* __restrict__ row_start, int* __restrict__ rs_rel, int* __restrict__ kv_len,
                                                            int* __restrict__ row_pos, int* __restrict__ u_src, int* __restrict__ u_crow,
                                                            int* __restrict__ u_row) {
    const int b = blockIdx.x;
    int r0 = 0, u0 = 0, j = 0;
    for (int i = 0; i < b; ++i) {
        const int li = min(min(max(seq_len[i], 0), N), Rc - r0);
        r0 += li;
        if ((flags.w[i >> 5] >> (i & 31)) & 1u) { u0 += min(li, Ru - u0); ++j; }
    }
    const int len = min(min(max(seq_len[b], 0), N), Rc - r0);
    const bool guided = (flags.w[b >> 5] >> (b & 31)) & 1u;
    const int ulen = guided ? min(len, Ru - u0) : 0;
    if (threadIdx.x == 0) {
        row_start[b] = r0; kv_len[b] = len;
        if (guided) { row_start[B + j] = Rc + u0; rs_rel[j] = u0; kv_len[B + j] = ulen; }
    }
    for (int t = threadIdx.x; t < len; t += 256) {
        row_pos[r0 + t] = t;
        u_row[r0 + t] = t < ulen ? Rc + u0 + t : -1;
    }
    for (int t = threadIdx.x; t < ulen; t += 256) {
        row_pos[Rc + u0 + t] = t;
        u_src[u0 + t] = b * N + t;
        u_crow[u0 + t] = r0 + t;
    }
    if (b == B - 1) {
        for (int t = r0 + len + (int)threadIdx.x; t < Rc; t += 256) {
            row_pos[t] = min(len + (t - (r0 + len)), N - 1);
            u_row[t] = -1;
        }
        for (int t = u0 + ulen + (int)threadIdx.x; t < Ru; t += 256) {
            const int p = min(len + (t - (u0 + ulen)), N - 1);
            row_pos[Rc + t] = p;
            u_src[t] = b * N + p;
            u_crow[t] = Rc - 1;
        }
    }
}

// ---------------------------------------------------------------- K5: GroupNorm over channel-major slabs [B][C][T]
// One workgroup per (group, batch item) slab of (C / G) x T contiguous floats, which stays in the caches: 3 reads + 1 write per element.
// (1) m0 = sum x / n; (2) the sums of (x - m0) and (x - m0)^2: the corrected two-pass variance, mean = m0 + d, var = q / n - d^2 with
// d = sum (x - m0) / n, a few roundings of m0 -- accurate whatever single elements hold (a shift by the slab's first element, the earlier
// form, lost five digits when that element was an outlier: profiles/norm_parity/notes.md); (3) normalise with the per-channel affine and
// the optional fused activation.  16-byte loads and stores, wave-shuffle + LDS reductions; a slab that is not 16-byte aligned or whose T
// is not a multiple of 4 takes scalar accesses.
__global__ __launch_bounds__(256) void groupnorm_kernel(const float* __restrict__ x, float* __restrict__ y,
                                                        const float* __restrict__ gamma, const float* __restrict__ beta,
                                                        int C, int T, int G, float eps, int act) {
    __shared__ float red[3][4];
    const int b = blockIdx.y, g = blockIdx.x;
    const int cpg = C / G;
    const size_t n = (size_t)cpg * T;
    const float* xs = x + ((size_t)b * C + (size_t)g * cpg) * T;
    float* ys = y + ((size_t)b * C + (size_t)g * cpg) * T;
    const bool vec = (T & 3) == 0 && (((uintptr_t)xs | (uintptr_t)ys) & 15) == 0;
    const size_t n4 = n >> 2;
    float s0 = 0.f;
    if (vec) {
        for (size_t i = threadIdx.x; i < n4; i += 256) {
            const float4 v = *(const float4*)(xs + i * 4);
            s0 += (v.x + v.y) + (v.z + v.w);
        }
    } else {
        for (size_t i = threadIdx.x; i < n; i += 256) s0 += xs[i];
    }
    s0 = wave_sum(s0);
    if ((threadIdx.x & 63) == 0) red[0][threadIdx.x >> 6] = s0;
    __syncthreads();
    const float m0 = ((red[0][0] + red[0][1]) + (red[0][2] + red[0][3])) / (float)n;
    float s = 0.f, q = 0.f;
    if (vec) {
        for (size_t i = threadIdx.x; i < n4; i += 256) {
            const float4 v = *(const float4*)(xs + i * 4);
            const float a0 = v.x - m0, a1 = v.y - m0, a2 = v.z - m0, a3 = v.w - m0;
            s += (a0 + a1) + (a2 + a3);
            q += (a0 * a0 + a1 * a1) + (a2 * a2 + a3 * a3);
        }
    } else {
        for (size_t i = threadIdx.x; i < n; i += 256) { const float d = xs[i] - m0; s += d; q += d * d; }
    }
    s = wave_sum(s); q = wave_sum(q);
    if ((threadIdx.x & 63) == 0) { red[1][threadIdx.x >> 6] = s; red[2][threadIdx.x >> 6] = q; }
    __syncthreads();
    const float sd = ((red[1][0] + red[1][1]) + (red[1][2] + red[1][3])) / (float)n;      // mean of x - m0: the rounding m0 carries
    const float var = fmaxf(((red[2][0] + red[2][1]) + (red[2][2] + red[2][3])) / (float)n - sd * sd, 0.f);
    const float mean = m0 + sd, rstd = rsqrtf(var + eps);
    if (vec) {
        const int t4 = T >> 2;
        for (size_t i = threadIdx.x; i < n4; i += 256) {
            const int c = g * cpg + (int)(i / t4);
            const float ga = (gamma ? gamma[c] : 1.f) * rstd, be = beta ? beta[c] : 0.f;
            const float4 v = *(const float4*)(xs + i * 4);
            float4 o;
            o.x = act_apply((v.x - mean) * ga + be, act); o.y = act_apply((v.y - mean) * ga + be, act);
            o.z = act_apply((v.z - mean) * ga + be, act); o.w = act_apply((v.w - mean) * ga + be, act);
            *(float4*)(ys + i * 4) = o;
        }
    } else {
        for (size_t i = threadIdx.x; i < n; i += 256) {
            const int c = g * cpg + (int)(i / T);
            ys[i] = act_apply((xs[i] - mean) * ((gamma ? gamma[c] : 1.f) * rstd) + (beta ? beta[c] : 0.f), act);
        }
    }
}

__global__ __launch_bounds__(256) void rope_compact_kernel(const float* __restrict__ c, const float* __restrict__ s, float* __restrict__ out, int n) {
    const int i = blockIdx.x * 256 + threadIdx.x;      // one (pos, pair)
    if (i >= n * 32) return;
    const int pos = i >> 5, pr = i & 31;
    out[(size_t)pos * 64 + 2 * pr] = c[(size_t)pos * 64 + 2 * pr];
    out[(size_t)pos * 64 + 2 * pr + 1] = s[(size_t)pos * 64 + 2 * pr];
}

__global__ __launch_bounds__(256) void rope_rows_kernel(const float* __restrict__ cs, const int* __restrict__ pos, float* __restrict__ out, int rows) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;      // one float4 of one row
    if (i >= (size_t)rows * 16) return;
    const size_t r = i >> 4;
    const int q = (int)(i & 15);
    *(float4*)(out + r * 64 + q * 4) = *(const float4*)(cs + (size_t)pos[r] * 64 + q * 4);
}

#ifndef VV_ELEMENTWISE_HOST_CHECK
inline int grid_for(size_t total) { return (int)std::min<size_t>((total + 255) / 256, 256 * 8); }
#endif

}  // namespace

#ifndef VV_ELEMENTWISE_HOST_CHECK
#define VVK_CHECK_LAUNCH()                                               \
    do {                                                                 \
        hipError_t he__ = hipGetLastError();                             \
        if (he__ != hipSuccess) { *err = hipGetErrorString(he__); return -5; } \
    } while (0)

int vvk_ln_mod(const vv_ln_args* a, hipStream_t st, const char** err) {
    if (a->R <= 0) { *err = "ln: empty"; return -22; }
    if (a->D < 4 || a->D % 4 || a->D > 1024 || a->ldx % 4 || a->ldy % 4) { *err = "ln: D must be a multiple of 4 within [4, 1024]"; return -22; }
    if (a->ldx < a->D || a->ldy < a->D) { *err = "ln: ldx and ldy must be at least D"; return -22; }
    if (a->delta && (a->ld_delta % 4 || a->ld_delta < a->D)) { *err = "ln: bad delta leading dimension"; return -22; }
    if (a->delta2 && !a->delta) { *err = "ln: delta2 without delta"; return -22; }
    const int grid = (a->R + 3) / 4;
    float* x = const_cast<float*>(a->x);
    const bool ob = a->out_dtype == VV_BF16, db = a->delta_dtype == VV_BF16;
    const int tp1 = a->delta && a->delta_tail_parts > 1 ? a->delta_tail_parts : 0, tp2 = a->delta2 && a->delta2_tail_parts > 1 ? a->delta2_tail_parts : 0;
    if ((tp1 || tp2) && (((uintptr_t)a->delta_tail | (uintptr_t)a->delta2_tail) % 16)) { *err = "ln: split-K tail buffers must be 16-byte aligned"; return -22; }
    if ((a->delta_tail_parts > 1 && !a->delta) || (a->delta2_tail_parts > 1 && !a->delta2)) { *err = "ln: a delta tail without its delta"; return -22; }
    if ((tp1 || tp2) && (a->tail_row0 < 0 || a->tail_row0 >= a->R || (tp1 && !a->delta_tail) || (tp2 && !a->delta2_tail) || tp1 > 8 || tp2 > 8)) {
        *err = "ln: bad split-K tail (row0 within [0, R), buffers given, at most 8 parts)"; return -22;
    }
    const int tail_row0 = (tp1 || tp2) ? a->tail_row0 : a->R;
#define LN_GO(To, Td) ln_mod_kernel<To, Td><<<grid, 256, 0, st>>>(x, a->ldx, (To*)a->y, a->ldy, a->R, a->D, a->w, a->b, a->add_one, a->eps, (const Td*)a->delta, a->ld_delta, (const Td*)a->delta2, a->keep_x, tail_row0, tp1, (const float*)a->delta_tail, tp2, (const float*)a->delta2_tail)
    if (ob && db) LN_GO(bf16, bf16);
    else if (ob) LN_GO(bf16, float);
    else if (db) LN_GO(float, bf16);
    else LN_GO(float, float);
#undef LN_GO
    VVK_CHECK_LAUNCH();
    return 0;
}

int vvk_pack_cat(int dtype, const float* x, const float* cat, const float* cat_drop, void* out, int ldo, int BN, int n_mel,
                 int cond_dim, int only_x, const int* row_src, hipStream_t st, const char** err) {
    if (n_mel % 4 || cond_dim % 4 || ldo % 4 || ldo < n_mel + cond_dim) { *err = "pack_cat: bad widths"; return -22; }
    if (BN < 1 || n_mel < 4 || cond_dim < 0) { *err = "pack_cat: BN >= 1, n_mel >= 4, cond_dim >= 0"; return -22; }
    if (!x || !out || (!only_x && cond_dim > 0 && (!cat || !cat_drop))) { *err = "pack_cat: x, out and (unless only_x) cat and cat_drop are required"; return -22; }
    // both kernels move 4 elements at a time: float4 loads, a float4 or 4 x bf16 store
    if (((uintptr_t)x | (uintptr_t)cat | (uintptr_t)cat_drop) % 16 || (uintptr_t)out % (dtype == VV_BF16 ? 8 : 16)) {
        *err = "pack_cat: x, cat and cat_drop must be 16-byte aligned, out 16-byte (f32) or 8-byte (bf16)"; return -22;
    }
    const size_t total = (size_t)2 * BN * ((only_x ? n_mel : ldo) / 4);
    if (dtype == VV_BF16)
        pack_cat_kernel<bf16><<<grid_for(total), 256, 0, st>>>(x, cat, cat_drop, (bf16*)out, ldo, BN, n_mel, cond_dim, only_x, row_src);
    else
        pack_cat_kernel<float><<<grid_for(total), 256, 0, st>>>(x, cat, cat_drop, (float*)out, ldo, BN, n_mel, cond_dim, only_x, row_src);
    VVK_CHECK_LAUNCH();
    return 0;
}

int vvk_cfg_euler(float* x, const float* pred, int ldp, int BN, int n_mel, float cfg, float dt, const int* row_src, hipStream_t st,
                  const char** err) {
    if (n_mel % 4 || ldp % 4) { *err = "cfg_euler: widths must be multiples of 4"; return -22; }
    if (BN < 1 || n_mel < 4 || ldp < n_mel) { *err = "cfg_euler: BN >= 1, n_mel >= 4, ldp >= n_mel"; return -22; }
    if (!x || !pred) { *err = "cfg_euler: x and pred are required"; return -22; }
    if (((uintptr_t)x | (uintptr_t)pred) % 16) { *err = "cfg_euler: x and pred must be 16-byte aligned"; return -22; }
    cfg_euler_kernel<<<grid_for((size_t)BN * n_mel / 4), 256, 0, st>>>(x, pred, ldp, BN, n_mel, cfg, dt, row_src);
    VVK_CHECK_LAUNCH();
    return 0;
}

int vvk_ode_stage(const vv_ode_stage_args* a, const int* u_row, const vv_apg_stage_args* apg, hipStream_t st, const char** err, int k_out_ring,
                  const vv_reuse_stage_args* reuse, const float* norm_coef) {
    if (a->n_mel < 4 || a->n_mel % 4 || a->ldp % 4 || a->ldp < a->n_mel || a->Rc < 1) { *err = "ode_stage: widths must be multiples of 4, ldp >= n_mel, Rc >= 1"; return -22; }
    if (!a->x || !a->pred || a->n_prev < 0 || a->n_prev > 3) { *err = "ode_stage: x, pred and 0..3 earlier slopes"; return -22; }
    if (a->g_item && a->seq_n < 1) { *err = "ode_stage: g_item needs the padded sequence length seq_n"; return -22; }
    uintptr_t al = (uintptr_t)a->x | (uintptr_t)a->pred | (uintptr_t)a->k_out | (uintptr_t)a->x_out;
    OdeStagePrev pv{};
    for (int j = 0; j < a->n_prev; ++j) {
        if (!(a->coef[j] == a->coef[j]) || !(a->coef[a->n_prev] == a->coef[a->n_prev])) { *err = "ode_stage: NaN coefficient"; return -22; }
        if (a->coef[j] == 0.f) continue;
        if (!a->k_prev[j]) { *err = "ode_stage: a non-zero coefficient without its slope buffer"; return -22; }
        pv.k[j] = a->k_prev[j]; pv.c[j] = a->coef[j];
        al |= (uintptr_t)a->k_prev[j];
        // k_out_ring (N20, the steps driver alone): k_out may BE one of the earlier slopes' buffers -- the kernel stores k behind its loads of them
        if ((a->k_prev[j] == a->k_out && !k_out_ring) || a->k_prev[j] == a->x_out) { *err = "ode_stage: an output aliases an earlier slope"; return -22; }
    }
    if (al % 16) { *err = "ode_stage: buffers must be 16-byte aligned"; return -22; }
    if (a->x_out && (a->x_out == a->x || a->x_out == a->k_out)) { *err = "ode_stage: x_out must be a buffer of its own"; return -22; }
    if (apg) {
        if (!apg->coef || !apg->x_e || a->seq_n < 1) { *err = "ode_stage: APG needs coef, x_e and the padded sequence length seq_n"; return -22; }
        if (((uintptr_t)apg->coef % 8) || ((uintptr_t)apg->x_e % 16)) { *err = "ode_stage: APG coef must be 8-byte and x_e 16-byte aligned"; return -22; }
        if (apg->x_e == a->x_out || apg->x_e == a->k_out) { *err = "ode_stage: APG x_e aliases an output of the launch"; return -22; }
        if (!(apg->t_e == apg->t_e)) { *err = "ode_stage: NaN evaluation time"; return -22; }
    }
    const int grid = grid_for((size_t)a->Rc * a->n_mel / 4);
    const float omt = apg ? 1.0f - apg->t_e : 0.f;
    if (norm_coef) {                                     // N24
        if (apg || reuse || !u_row) { *err = "ode_stage: the CFG-Zero* / rescale form needs u_row and is not combined with APG or reuse"; return -22; }
        if ((uintptr_t)norm_coef % 8 || a->seq_n < 1) { *err = "ode_stage: the CFG-Zero* / rescale form needs 8-byte aligned coefficients and the padded sequence length seq_n"; return -22; }
        ode_stage_kernel<true, false, false, true><<<grid, 256, 0, st>>>(a->x, a->pred, a->ldp, a->Rc, a->n_mel, a->g, a->g_item, a->seq_n, a->row_src, pv,
                                                                          a->coef[a->n_prev], a->k_out, a->x_out, u_row, norm_coef, nullptr, 0, omt, OdeStageNoReuse{});
        VVK_CHECK_LAUNCH();
        return 0;
    }
    if (reuse) {                                         // N21
        if (apg || !u_row) { *err = "ode_stage: the reuse form needs u_row and is not combined with APG"; return -22; }
        if (!reuse->d_buf || (uintptr_t)reuse->d_buf % 16 || !reuse->item_mode_host) { *err = "ode_stage: d_buf (16-byte aligned) and the item modes are required"; return -22; }
        if (a->seq_n < 1 || reuse->n_items < 1 || reuse->n_items > VVK_GUIDE_MAX_ITEMS) { *err = "ode_stage: the reuse form needs seq_n and 1..1024 item modes"; return -22; }
        if (reuse->d_buf == a->k_out || reuse->d_buf == a->x_out || reuse->d_buf == a->x) { *err = "ode_stage: d_buf must be a buffer of its own"; return -22; }
        for (int j = 0; j < 3; ++j)
            if (pv.k[j] == reuse->d_buf) { *err = "ode_stage: d_buf must be a buffer of its own"; return -22; }
        OdeStageReuse ru{};
        ru.d_buf = reuse->d_buf;
        for (int b = 0; b < reuse->n_items; ++b) {
            if (reuse->item_mode_host[b] & ~3u) { *err = "ode_stage: an item mode is VV_REUSE_LOAD | VV_REUSE_STORE at the most"; return -22; }
            if (reuse->item_mode_host[b] & VV_REUSE_LOAD) ru.load.w[b >> 5] |= 1u << (b & 31);
            if (reuse->item_mode_host[b] & VV_REUSE_STORE) ru.store.w[b >> 5] |= 1u << (b & 31);
        }
        ode_stage_kernel<true, false, true><<<grid, 256, 0, st>>>(a->x, a->pred, a->ldp, a->Rc, a->n_mel, a->g, a->g_item, a->seq_n, a->row_src, pv,
                                                                   a->coef[a->n_prev], a->k_out, a->x_out, u_row, nullptr, nullptr, 0, omt, ru);
        VVK_CHECK_LAUNCH();
        return 0;
    }
#define STAGE_GO(G, A) ode_stage_kernel<G, A><<<grid, 256, 0, st>>>(a->x, a->pred, a->ldp, a->Rc, a->n_mel, a->g, a->g_item, a->seq_n, a->row_src, pv, \
        a->coef[a->n_prev], a->k_out, a->x_out, u_row, apg ? apg->coef : nullptr, apg ? apg->x_e : nullptr, apg ? apg->x_e_packed : 0, omt, OdeStageNoReuse{})
    if (apg) { if (u_row) STAGE_GO(true, true); else STAGE_GO(false, true); }
    else if (u_row) STAGE_GO(true, false);
    else STAGE_GO(false, false);
#undef STAGE_GO
    VVK_CHECK_LAUNCH();
    return 0;
}

// N11: the two kernels behind vv_apg_coef.  which & 1: the reduction, which & 2: the coefficients.
int vvk_apg_coef(const vv_apg_coef_args* a, int which, hipStream_t st, const char** err) {
    if (a->n_mel < 4 || a->n_mel % 4 || a->ldp % 4 || a->ldp < a->n_mel || a->Rc < 1) { *err = "apg_coef: widths must be multiples of 4, ldp >= n_mel, Rc >= 1"; return -22; }
    if (!a->pred || !a->x_e || !a->row_start || !a->len || !a->partials || !a->coef) { *err = "apg_coef: pred, x_e, row_start, len, partials and coef are required"; return -22; }
    if (a->B < 1 || a->B > VVK_GUIDE_MAX_ITEMS || a->n_tiles < 1) { *err = "apg_coef: 1..1024 items, n_tiles >= 1"; return -22; }
    if (((uintptr_t)a->pred | (uintptr_t)a->x_e) % 16 || (uintptr_t)a->partials % 8 || (uintptr_t)a->coef % 8) { *err = "apg_coef: pred and x_e 16-byte, partials and coef 8-byte aligned"; return -22; }
    if (!(a->t_e == a->t_e)) { *err = "apg_coef: NaN evaluation time"; return -22; }
    const double omt = 1.0 - (double)a->t_e;
    if (which & 1) {
        apg_reduce_kernel<<<dim3(a->n_tiles, a->B), 256, 0, st>>>(a->pred, a->ldp, a->Rc, a->n_mel, a->u_row, a->x_e, a->row_src, a->row_start,
                                                                   a->len, a->n_tiles, omt, a->partials);
        VVK_CHECK_LAUNCH();
    }
    if (which & 2) {
        apg_coef_kernel<<<a->B, 64, 0, st>>>(a->partials, a->n_tiles, a->Rc, a->n_mel, a->u_row, a->row_start, a->len, omt, a->g, a->g_item,
                                             a->eta, a->norm_rms, a->coef);
        VVK_CHECK_LAUNCH();
    }
    return 0;
}

// N24: the two kernels behind vv_cfg_norm_coef.  which & 1: the Gram sums, which & 2: the coefficients.
int vvk_cfg_norm_coef(const vv_cfg_norm_coef_args* a, int which, hipStream_t st, const char** err) {
    if (a->n_mel < 4 || a->n_mel % 4 || a->ldp % 4 || a->ldp < a->n_mel || a->Rc < 1) { *err = "cfg_norm_coef: widths must be multiples of 4, ldp >= n_mel, Rc >= 1"; return -22; }
    if (!a->pred || !a->row_start || !a->len || !a->partials || !a->coef) { *err = "cfg_norm_coef: pred, row_start, len, partials and coef are required"; return -22; }
    if (a->B < 1 || a->B > VVK_GUIDE_MAX_ITEMS || a->n_tiles < 1) { *err = "cfg_norm_coef: 1..1024 items, n_tiles >= 1"; return -22; }
    if ((uintptr_t)a->pred % 16 || (uintptr_t)a->partials % 8 || (uintptr_t)a->coef % 8 || (uintptr_t)a->report % 8) { *err = "cfg_norm_coef: pred 16-byte, partials, coef and report 8-byte aligned"; return -22; }
    if (!(a->g == a->g)) { *err = "cfg_norm_coef: NaN strength"; return -22; }
    if (which & 1) {
        cfg_gram_reduce_kernel<<<dim3(a->n_tiles, a->B), 256, 0, st>>>(a->pred, a->ldp, a->Rc, a->n_mel, a->u_row, a->row_start, a->len, a->n_tiles, a->partials);
        VVK_CHECK_LAUNCH();
    }
    if (which & 2) {
        cfg_norm_coef_kernel<<<a->B, 64, 0, st>>>(a->partials, a->n_tiles, a->Rc, a->n_mel, a->u_row, a->row_start, a->len, a->g, a->g_item, a->star, a->rescale,
                                                  a->coef, a->report);
        VVK_CHECK_LAUNCH();
    }
    return 0;
}

// N20: the two kernels behind vv_ode_diff_reduce.  which & 1: the reduction, which & 2: the item sums.
int vvk_ode_diff_reduce(const vv_ode_diff_args* a, int which, hipStream_t st, const char** err) {
    if (a->n_mel < 4 || a->n_mel % 4 || a->Rc < 1) { *err = "ode_diff_reduce: n_mel must be a multiple of 4, Rc >= 1"; return -22; }
    if (!a->f || !a->row_start || !a->len || !a->partials || !a->report) { *err = "ode_diff_reduce: f, row_start, len, partials and report are required"; return -22; }
    if (a->B < 1 || a->B > VVK_GUIDE_MAX_ITEMS || a->n_tiles < 1) { *err = "ode_diff_reduce: 1..1024 items, n_tiles >= 1"; return -22; }
    if (((uintptr_t)a->f | (uintptr_t)a->f_prev) % 16 || ((uintptr_t)a->partials | (uintptr_t)a->report) % 8) { *err = "ode_diff_reduce: f and f_prev 16-byte, partials and report 8-byte aligned"; return -22; }
    if (which & 1) {
        ode_diff_reduce_kernel<<<dim3(a->n_tiles, a->B), 256, 0, st>>>(a->f, a->f_prev, a->Rc, a->n_mel, a->row_start, a->len, a->n_tiles, a->partials);
        VVK_CHECK_LAUNCH();
    }
    if (which & 2) {
        ode_diff_finish_kernel<<<a->B, 64, 0, st>>>(a->partials, a->n_tiles, a->Rc, a->row_start, a->len, a->report);
        VVK_CHECK_LAUNCH();
    }
    return 0;
}

// N21: the two kernels behind vv_cfg_drift_reduce.  which & 1: the reduction, which & 2: the item sums (ode_diff_finish_kernel).
int vvk_cfg_drift_reduce(const vv_cfg_drift_args* a, int which, hipStream_t st, const char** err) {
    if (a->n_mel < 4 || a->n_mel % 4 || a->ldp % 4 || a->ldp < a->n_mel || a->Rc < 1) { *err = "cfg_drift_reduce: widths must be multiples of 4, ldp >= n_mel, Rc >= 1"; return -22; }
    if (!a->pred || !a->u_row || !a->row_start || !a->len || !a->partials || !a->report) { *err = "cfg_drift_reduce: pred, u_row, row_start, len, partials and report are required"; return -22; }
    if (a->B < 1 || a->B > VVK_GUIDE_MAX_ITEMS || a->n_tiles < 1) { *err = "cfg_drift_reduce: 1..1024 items, n_tiles >= 1"; return -22; }
    if (((uintptr_t)a->pred | (uintptr_t)a->d_buf) % 16 || ((uintptr_t)a->partials | (uintptr_t)a->report) % 8) { *err = "cfg_drift_reduce: pred and d_buf 16-byte, partials and report 8-byte aligned"; return -22; }
    GuideFlags old{};
    for (int b = 0; b < a->B && a->has_old_host; ++b)
        if (a->has_old_host[b]) old.w[b >> 5] |= 1u << (b & 31);
    if (a->has_old_host && !a->d_buf)
        for (unsigned w : old.w)
            if (w) { *err = "cfg_drift_reduce: an item with a stored difference needs d_buf"; return -22; }
    if (which & 1) {
        cfg_drift_reduce_kernel<<<dim3(a->n_tiles, a->B), 256, 0, st>>>(a->pred, a->ldp, a->Rc, a->n_mel, a->u_row, a->d_buf, old, a->row_start, a->len,
                                                                         a->n_tiles, a->partials);
        VVK_CHECK_LAUNCH();
    }
    if (which & 2) {
        ode_diff_finish_kernel<<<a->B, 64, 0, st>>>(a->partials, a->n_tiles, a->Rc, a->row_start, a->len, a->report);
        VVK_CHECK_LAUNCH();
    }
    return 0;
}

// N23: one MARK, DIFF or APPLY launch of block_span_kernel
int vvk_block_span(const vv_block_span_args* a, hipStream_t st, const char** err) {
    if (a->mode < VV_SPAN_MARK || a->mode > VV_SPAN_APPLY) { *err = "block_span: mode is VV_SPAN_MARK, VV_SPAN_DIFF or VV_SPAN_APPLY"; return -22; }
    if (a->R < 1 || a->D < 4 || a->D % 4) { *err = "block_span: R >= 1, D a multiple of 4"; return -22; }
    if (!a->x || !a->buf || (a->d2 && !a->d1)) { *err = "block_span: x and buf are required, d2 needs d1"; return -22; }
    const bool db = a->delta_dtype == VV_BF16;
    if (((uintptr_t)a->x | (uintptr_t)a->buf) % 16 || ((uintptr_t)a->d1 | (uintptr_t)a->d2) % (db ? 8 : 16)) {
        *err = "block_span: x and buf must be 16-byte aligned, the deltas 16-byte (f32) or 8-byte (bf16)"; return -22;
    }
    const size_t n4 = (size_t)a->R * a->D / 4;
    if ((uintptr_t)a->x < (uintptr_t)a->buf + n4 * 16 && (uintptr_t)a->buf < (uintptr_t)a->x + n4 * 16) { *err = "block_span: buf must be a plane of its own"; return -22; }
    const int grid = grid_for(n4);
#define SPAN_GO(Td, M) block_span_kernel<Td, M><<<grid, 256, 0, st>>>(a->x, (const Td*)a->d1, (const Td*)a->d2, a->buf, n4)
#define SPAN_DT(M) do { if (db) SPAN_GO(bf16, M); else SPAN_GO(float, M); } while (0)
    if (a->mode == VV_SPAN_MARK) SPAN_DT(VV_SPAN_MARK);
    else if (a->mode == VV_SPAN_DIFF) SPAN_DT(VV_SPAN_DIFF);
    else SPAN_DT(VV_SPAN_APPLY);
#undef SPAN_DT
#undef SPAN_GO
    VVK_CHECK_LAUNCH();
    return 0;
}

// N23: the two kernels behind vv_block_drift_reduce.  which & 1: the reduction, which & 2: the sequence sums at their [item][branch] place;
// which == 4: zeros at those places (the finishing kernel over no tiles: nothing but the tables is read).
int vvk_block_drift_reduce(const vv_block_drift_args* a, int which, hipStream_t st, const char** err) {
    if (a->D < 4 || a->D % 4 || a->R < 1) { *err = "block_drift_reduce: D must be a multiple of 4, R >= 1"; return -22; }
    if (!a->row_start || !a->len || !a->report || (which != 4 && (!a->d_new || !a->partials))) { *err = "block_drift_reduce: d_new, row_start, len, partials and report are required"; return -22; }
    if (a->n_items < 1 || a->n_items > VVK_GUIDE_MAX_ITEMS || a->n_tiles < 1) { *err = "block_drift_reduce: 1..1024 items, n_tiles >= 1"; return -22; }
    if (!((a->n_seq == a->n_items && (a->branch0 == 0 || a->branch0 == 1)) || (a->n_seq == 2 * a->n_items && a->branch0 == 0))) {
        *err = "block_drift_reduce: n_seq is n_items (one branch, branch0 0 or 1) or 2 n_items (both, branch0 0)"; return -22;
    }
    if (((uintptr_t)a->d_new | (uintptr_t)a->d_prev) % 16 || ((uintptr_t)a->partials | (uintptr_t)a->report) % 8) { *err = "block_drift_reduce: d_new and d_prev 16-byte, partials and report 8-byte aligned"; return -22; }
    if (which == 4) {
        block_drift_finish_kernel<<<a->n_seq, 64, 0, st>>>(a->partials, 0, a->R, a->row_start, a->len, a->n_items, a->branch0, a->report);
        VVK_CHECK_LAUNCH();
        return 0;
    }
    if (which & 1) {
        block_drift_reduce_kernel<<<dim3(a->n_tiles, a->n_seq), 256, 0, st>>>(a->d_new, a->d_prev, a->R, a->D, a->row_start, a->len, a->n_tiles, a->partials);
        VVK_CHECK_LAUNCH();
    }
    if (which & 2) {
        block_drift_finish_kernel<<<a->n_seq, 64, 0, st>>>(a->partials, a->n_tiles, a->R, a->row_start, a->len, a->n_items, a->branch0, a->report);
        VVK_CHECK_LAUNCH();
    }
    return 0;
}

int vvk_pack_cat_guided(int dtype, const float* x, const float* cat, const float* cat_drop, void* out, int ldo, int Rc, int row0, int n_rows,
                        int n_mel, int cond_dim, int only_x, int x_packed, const int* row_src, const int* u_src, const int* u_crow,
                        hipStream_t st, const char** err) {
    if (n_mel % 4 || cond_dim % 4 || ldo % 4 || ldo < n_mel + cond_dim) { *err = "pack_cat_guided: bad widths"; return -22; }
    if (Rc < 1 || row0 < 0 || n_rows < 1 || !row_src || !u_src || !u_crow) { *err = "pack_cat_guided: rows and their three tables"; return -22; }
    if (n_mel < 4 || cond_dim < 0) { *err = "pack_cat_guided: n_mel >= 4, cond_dim >= 0"; return -22; }
    if (!x || !out || (!only_x && cond_dim > 0 && (!cat || !cat_drop))) { *err = "pack_cat_guided: x, out and (unless only_x) cat and cat_drop are required"; return -22; }
    if (((uintptr_t)x | (uintptr_t)cat | (uintptr_t)cat_drop) % 16 || (uintptr_t)out % (dtype == VV_BF16 ? 8 : 16)) {
        *err = "pack_cat_guided: x, cat and cat_drop must be 16-byte aligned, out 16-byte (f32) or 8-byte (bf16)"; return -22;
    }
    const size_t total = (size_t)n_rows * ((only_x ? n_mel : ldo) / 4);
    if (dtype == VV_BF16)
        pack_cat_guided_kernel<bf16><<<grid_for(total), 256, 0, st>>>(x, cat, cat_drop, (bf16*)out, ldo, Rc, row0, n_rows, n_mel, cond_dim, only_x,
                                                                      x_packed, row_src, u_src, u_crow);
    else
        pack_cat_guided_kernel<float><<<grid_for(total), 256, 0, st>>>(x, cat, cat_drop, (float*)out, ldo, Rc, row0, n_rows, n_mel, cond_dim, only_x,
                                                                       x_packed, row_src, u_src, u_crow);
    VVK_CHECK_LAUNCH();
    return 0;
}

int vvk_guided_tables(const int* seq_len, const unsigned char* flags, int B, int N, int Rc, int Ru, int* row_start, int* rs_rel, int* kv_len,
                      int* row_pos, int* u_src, int* u_crow, int* u_row, hipStream_t st, const char** err) {
    if (B < 1 || B > VVK_GUIDE_MAX_ITEMS || N < 1 || Rc < 1 || Ru < 0 || Ru > Rc || !flags) { *err = "guided_tables: 1..1024 items, 0 <= Ru <= Rc"; return -22; }
    GuideFlags f{};
    for (int b = 0; b < B; ++b)
        if (flags[b]) f.w[b >> 5] |= 1u << (b & 31);
    guided_tables_kernel<<<B, 256, 0, st>>>(seq_len, f, B, N, Rc, Ru, row_start, rs_rel, kv_len, row_pos, u_src, u_crow, u_row);
    VVK_CHECK_LAUNCH();
    return 0;
}

int vvk_text_embed(const int* ids, int ld_ids, const int* text_len, const float* emb, const float* pos, float* out, int B,
                   int N, int Dt, int vocab_rows, hipStream_t st, const char** err) {
    if (Dt % 4) { *err = "text_embed: Dt % 4"; return -22; }
    text_embed_kernel<<<grid_for((size_t)2 * B * N * Dt / 4), 256, 0, st>>>(ids, ld_ids, text_len, emb, pos, out, B, N, Dt, vocab_rows);
    VVK_CHECK_LAUNCH();
    return 0;
}

int vvk_dwconv(const float* in, float* out, const float* w, const float* bias, const int* seq_len, int B, int n_seq, int N,
               int C, int KW, hipStream_t st, const char** err) {
    if (C % 4) { *err = "dwconv: C % 4"; return -22; }
    dwconv_kernel<<<grid_for((size_t)n_seq * N * C / 4), 256, 0, st>>>(in, out, w, bias, seq_len, B, n_seq, N, C, KW);
    VVK_CHECK_LAUNCH();
    return 0;
}

int vvk_grn(int dtype, void* x, float* sumsq, const float* gamma, const float* beta, const int* seq_len, int B, int n_seq,
            int N, int C, hipStream_t st, const char** err) {
    if (C % 64 || C > 8192) { *err = "grn: C must be a multiple of 64"; return -22; }
    dim3 g1(C / 64, n_seq);
    const int rpb = 16;
    dim3 g2((N + rpb - 1) / rpb, n_seq);
    if (dtype == VV_BF16) {
        grn_stats_kernel<bf16><<<g1, 256, 0, st>>>((const bf16*)x, sumsq, seq_len, B, N, C);
        grn_apply_kernel<bf16><<<g2, 256, C * sizeof(float), st>>>((bf16*)x, sumsq, gamma, beta, N, C, rpb);
    } else {
        grn_stats_kernel<float><<<g1, 256, 0, st>>>((const float*)x, sumsq, seq_len, B, N, C);
        grn_apply_kernel<float><<<g2, 256, C * sizeof(float), st>>>((float*)x, sumsq, gamma, beta, N, C, rpb);
    }
    VVK_CHECK_LAUNCH();
    return 0;
}

int vvk_build_cat(const float* mel, int F_max, const int* ref_len, const float* text, float* cat, float* cat_drop, int B, int N,
                  int n_mel, int Dt, hipStream_t st, const char** err, const uint8_t* keep, int ld_keep) {
    if (n_mel % 4 || Dt % 4) { *err = "build_cat: widths % 4"; return -22; }
    if (keep && ld_keep < N) { *err = "build_cat: ld_keep < N"; return -22; }
    const int grid = grid_for((size_t)B * N * (n_mel + Dt) / 4);
    if (keep)
        build_cat_kernel<true><<<grid, 256, 0, st>>>(mel, F_max, ref_len, text, cat, cat_drop, B, N, n_mel, Dt, keep, ld_keep);
    else
        build_cat_kernel<false><<<grid, 256, 0, st>>>(mel, F_max, ref_len, text, cat, cat_drop, B, N, n_mel, Dt, nullptr, 0);
    VVK_CHECK_LAUNCH();
    return 0;
}

int vvk_ref_len(const int* audio_len, int* ref_len, int B, int hop, hipStream_t st, const char** err) {
    if (B < 1 || hop < 1 || !audio_len || !ref_len) { *err = "ref_len: B >= 1, hop >= 1, audio_len and ref_len required"; return -22; }
    ref_len_kernel<<<(B + 63) / 64, 64, 0, st>>>(audio_len, ref_len, B, hop);
    VVK_CHECK_LAUNCH();
    return 0;
}
int vvk_decode_len(const int* seq_len, const int* ref_len, int* lens, int B, int n_levels, const int* mult, int N, int T_max, hipStream_t st,
                   const char** err) {
    if (B < 1 || n_levels < 1 || N < 1 || T_max < 1 || !seq_len || !ref_len || !lens || !mult) {
        *err = "decode_len: B, n_levels, N, T_max >= 1, seq_len, ref_len, lens and mult required"; return -22;
    }
    decode_len_kernel<<<(B + 63) / 64, 64, 0, st>>>(seq_len, ref_len, lens, B, n_levels, mult, N, T_max);
    VVK_CHECK_LAUNCH();
    return 0;
}
int vvk_row_tables(const int* seq_len, int B, int N, int Rc, int* row_start, int* row_src, int* row_pos, int* kv_len, hipStream_t st, const char** err) {
    if (B <= 0 || N <= 0 || Rc <= 0) { *err = "row_tables: empty"; return -22; }
    row_tables_kernel<<<B, 256, 0, st>>>(seq_len, B, N, Rc, row_start, row_src, row_pos, kv_len);
    hipError_t he = hipGetLastError();
    if (he != hipSuccess) { *err = hipGetErrorString(he); return -5; }
    return 0;
}

int vvk_groupnorm(const float* x, float* y, const float* gamma, const float* beta, int B, int C, int T, int G, float eps, int act,
                  hipStream_t st, const char** err) {
    if (B <= 0 || C <= 0 || T <= 0 || G <= 0 || C % G) { *err = "groupnorm: C must be a multiple of G"; return -22; }
    dim3 grid(G, B);
    groupnorm_kernel<<<grid, 256, 0, st>>>(x, y, gamma, beta, C, T, G, eps, act);
    VVK_CHECK_LAUNCH();
    return 0;
}
int vvk_rope_rows(const float* cs, const int* pos, float* out, int rows, hipStream_t st, const char** err) {
    if (rows <= 0 || !cs || !pos || !out) { *err = "rope_rows: bad arguments"; return -22; }
    rope_rows_kernel<<<(unsigned)(((size_t)rows * 16 + 255) / 256), 256, 0, st>>>(cs, pos, out, rows);
    hipError_t he = hipGetLastError();
    if (he != hipSuccess) { *err = hipGetErrorString(he); return -5; }
    return 0;
}

int vvk_rope_compact(const float* c, const float* s, float* out, int n, hipStream_t st, const char** err) {
    if (n <= 0) { *err = "rope_compact: empty"; return -22; }
    rope_compact_kernel<<<(n * 32 + 255) / 256, 256, 0, st>>>(c, s, out, n);
    VVK_CHECK_LAUNCH();
    return 0;
}
#endif
