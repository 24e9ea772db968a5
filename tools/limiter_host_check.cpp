// Host check of csrc/vv_limiter.hip: the four kernels compiled for the CPU, one std::thread per GPU thread of a
// workgroup, a barrier for __syncthreads, workgroups one after the other, every buffer an exact-size heap block -- so that address and
// undefined-behaviour sanitizers see an index past an end or a misaligned store.  tools/limiter_host_check.py builds this file with
// -fsanitize=address,undefined, feeds it the requests of the GPU test and compares the results with the numpy mirror, bit for bit.
//   limiter_host_check IN OUT [inplace] [yoff=K]
// IN : int64 {R, L, mode, n_x, n_y, has_meas}; rows R x 5 int64; window 2L+1 f64; taps 97 f64; params R x 3 f64; meas R x 4 f64 (if
//      has_meas); x n_x int16; y n_y int16
// OUT: stats R x 4 f64; y n_y int16.   yoff = the destination starts K samples (2 K bytes) past an 8-byte boundary
#include <barrier>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <thread>
#include <vector>

struct dim3 { unsigned x = 1, y = 1, z = 1; dim3(unsigned a = 1, unsigned b = 1, unsigned c = 1) : x(a), y(b), z(c) {} };
struct uint2 { uint32_t x, y; };
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
#define VV_LIMITER_HOST_CHECK
#include "../vietvoice-tts_amd/csrc/vv_limiter.hip"

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
    bool in_place = false;
    long long yoff = 0;
    for (int i = 3; i < argc; ++i) {
        if (!strcmp(argv[i], "inplace")) in_place = true;
        if (!strncmp(argv[i], "yoff=", 5)) yoff = atoll(argv[i] + 5);
    }
    FILE* f = fopen(argv[1], "rb");
    if (!f) return 2;
    long long hdr[6];
    if (fread(hdr, 8, 6, f) != 6) return 2;
    const long long R = hdr[0], n_x = hdr[3], n_y = hdr[4], has_meas = hdr[5];
    const int L = (int)hdr[1], mode = (int)hdr[2];
    long long* rows = block<long long>(5 * R);
    double* window = block<double>(2 * L + 1);
    double* taps = block<double>(8 * LH + 1);
    double* params = block<double>(3 * R);
    double* meas = has_meas ? block<double>(4 * R) : nullptr;
    int16_t* x = block<int16_t>(n_x);
    int16_t* ybase = block<int16_t>(n_y + yoff);         // malloc aligns to 16 bytes: y = ybase + yoff sits 2 * yoff bytes past that
    int16_t* y = ybase + yoff;
    if (fread(rows, 8, 5 * R, f) != (size_t)(5 * R) || fread(window, 8, 2 * L + 1, f) != (size_t)(2 * L + 1) ||
        fread(taps, 8, 8 * LH + 1, f) != (size_t)(8 * LH + 1) || fread(params, 8, 3 * R, f) != (size_t)(3 * R) ||
        (meas && fread(meas, 8, 4 * R, f) != (size_t)(4 * R)) || fread(x, 2, n_x, f) != (size_t)n_x || fread(y, 2, n_y, f) != (size_t)n_y)
        return 2;
    fclose(f);
    const int tile = limit_tile(L);
    long long total_samples = 0, total_tiles = 0, max_tiles = 0, max_out = 0;
    for (long long r = 0; r < R; ++r) {
        const long long n = rows[5 * r + 1], nt = (n + tile - 1) / tile;
        total_samples += n; total_tiles += nt;
        if (nt > max_tiles) max_tiles = nt;
        if (rows[5 * r + 4] > max_out) max_out = rows[5 * r + 4];
    }
    long long* offs = block<long long>(2 * R);           // the three parts of the scratch as blocks of their own: exact ends
    double* gains = block<double>(total_samples);
    double* recs = block<double>(3 * total_tiles);
    double* stats = block<double>(4 * R);
    launch(dim3(1), 64, [&]() { limit_offsets_kernel(rows, (int)R, tile, offs); });
    if (max_tiles > 0)
        launch(dim3((unsigned)max_tiles, (unsigned)R), NT, [&]() {
            limit_gain_kernel(x, n_x, rows, offs, L, tile, mode, window, taps, params, meas, total_samples, total_tiles, gains, recs);
        });
    launch(dim3((unsigned)R), 64, [&]() { limit_stats_kernel(rows, offs, tile, params, meas, total_tiles, recs, stats); });
    int16_t* dst = in_place ? x : y;
    const long long n_dst = in_place ? n_x : n_y;
    if (max_out > 0) {
        long long bx = (max_out / 4 + 256) / 256;
        if (bx > 4) bx = 4;                              // fewer workgroups than the device launches: the grid-stride loop covers the rest
        launch(dim3((unsigned)bx, (unsigned)R), 256, [&]() { limit_apply_kernel(x, n_x, rows, offs, params, meas, total_samples, gains, dst, n_dst); });
    }
    f = fopen(argv[2], "wb");
    if (!f) return 2;
    fwrite(stats, 8, 4 * R, f);
    fwrite(dst, 2, n_dst, f);
    fclose(f);
    free(rows); free(window); free(taps); free(params); free(meas); free(x); free(ybase); free(offs); free(gains); free(recs); free(stats);
    return 0;
}
