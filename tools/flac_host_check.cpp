// Host check of csrc/vv_flac.hip: the four kernels compiled for the CPU, one std::thread per GPU thread of a workgroup,
// a barrier for __syncthreads, compiler atomics for the LDS atomics, workgroups one after the other, every buffer an exact-size heap
// block -- so that address and undefined-behaviour sanitizers see an index past an end.  tools/flac_host_check.py builds this file with
// -fsanitize=address,undefined, feeds it the rows of the GPU test and compares the bytes with the numpy mirror.
//   flac_host_check IN OUT [LPC_ORDER]      (LPC_ORDER 1 ... 12: the kernels of vv_pcm_flac_lpc, N16; needs -ffp-contract=off)
// IN : int64 {R, n_x, n_y, rate}; rows R x 4 int64; x n_x int16; y n_y bytes
// OUT: info (R + 1) x 3 int64; y n_y bytes
#include <barrier>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <thread>
#include <vector>

struct dim3 { unsigned x = 1, y = 1, z = 1; dim3(unsigned a = 1, unsigned b = 1, unsigned c = 1) : x(a), y(b), z(c) {} };
static thread_local dim3 threadIdx, blockIdx, gridDim;
static std::barrier<>* g_bar;
#define __global__
#define __device__
#define __host__
#define __forceinline__ inline
#define __restrict__
#define __shared__ static
#define __launch_bounds__(x)
static void __syncthreads() { g_bar->arrive_and_wait(); }
static unsigned atomicOr(unsigned* p, unsigned v) { return __atomic_fetch_or(p, v, __ATOMIC_RELAXED); }
static unsigned atomicXor(unsigned* p, unsigned v) { return __atomic_fetch_xor(p, v, __ATOMIC_RELAXED); }
static unsigned long long atomicAdd(unsigned long long* p, unsigned long long v) { return __atomic_fetch_add(p, v, __ATOMIC_RELAXED); }
#define VV_FLAC_HOST_CHECK
#include "../vietvoice-tts_amd/csrc/vv_flac.hip"

template <typename F> static void launch(dim3 grid, int nthreads, F f) {
    for (unsigned by = 0; by < grid.y; ++by)
        for (unsigned bx = 0; bx < grid.x; ++bx) {
            std::barrier<> bar(nthreads);
            g_bar = &bar;
            std::vector<std::thread> th;
            for (int t = 0; t < nthreads; ++t)
                th.emplace_back([=]() {
                    threadIdx = dim3(t); blockIdx = dim3(bx, by); gridDim = grid;
                    f();
                    g_bar->arrive_and_drop();          // a thread that has returned lets the others pass their barriers
                });
            for (auto& x : th) x.join();
        }
}

template <typename T> static T* block(long long n) { return (T*)malloc(sizeof(T) * (size_t)(n > 0 ? n : 1)); }

int main(int argc, char** argv) {
    if (argc < 3) return 2;
    const int lpc_order = argc > 3 ? atoi(argv[3]) : 0;
    if (lpc_order < 0 || lpc_order > MAXL) return 2;
    FILE* f = fopen(argv[1], "rb");
    if (!f) return 2;
    long long hdr[4];
    if (fread(hdr, 8, 4, f) != 4) return 2;
    const long long R = hdr[0], n_x = hdr[1], n_y = hdr[2];
    const int rate = (int)hdr[3];
    long long* rows = block<long long>(4 * R);
    int16_t* x = block<int16_t>(n_x);
    uint8_t* y = block<uint8_t>(n_y);
    if (fread(rows, 8, 4 * R, f) != (size_t)(4 * R) || fread(x, 2, n_x, f) != (size_t)n_x || fread(y, 1, n_y, f) != (size_t)n_y) return 2;
    fclose(f);
    long long total = 0, most = 0;
    for (long long r = 0; r < R; ++r) {
        const long long fr = (rows[4 * r + 1] + FB - 1) / FB;
        total += fr;
        if (fr > most) most = fr;
    }
    long long* fbase = block<long long>(R + 1);
    long long* off = block<long long>(total);
    int* rec = block<int>(REC * total);
    long long* info = block<long long>(3 * (R + 1));
    int* lrec = block<int>(lpc_order ? LREC * total : 0);
    const dim3 grid((unsigned)most, (unsigned)R);
    launch(dim3(1), NT, [&]() { flac_plan_kernel(rows, (int)R, n_x, fbase); });
    if (lpc_order) launch(grid, NT, [&]() { flac_analyse_kernel<true>(x, n_x, rows, rate, fbase, total, rec, lpc_order, lrec); });
    else launch(grid, NT, [&]() { flac_analyse_kernel<false>(x, n_x, rows, rate, fbase, total, rec, 0, nullptr); });
    launch(dim3(1), NT, [&]() { flac_scan_kernel(fbase, (int)R, total, rec, off, info); });
    if (lpc_order) launch(grid, NT, [&]() { flac_pack_kernel<true>(x, n_x, rows, rate, fbase, total, off, rec, y, n_y, lrec); });
    else launch(grid, NT, [&]() { flac_pack_kernel<false>(x, n_x, rows, rate, fbase, total, off, rec, y, n_y, nullptr); });
    f = fopen(argv[2], "wb");
    if (!f) return 2;
    fwrite(info, 8, 3 * (R + 1), f);
    fwrite(y, 1, n_y, f);
    fclose(f);
    free(rows); free(x); free(y); free(fbase); free(off); free(rec); free(info); free(lrec);
    return 0;
}
