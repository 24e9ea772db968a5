// Host check of csrc/vv_loudness.hip: the five kernels compiled for the CPU, one std::thread per GPU thread of a
// workgroup, a barrier for __syncthreads, workgroups one after the other, every buffer an exact-size heap block -- so that address and
// undefined-behaviour sanitizers see an index past an end or a misaligned store.  tools/loudness_host_check.py builds this file with
// -fsanitize=address,undefined, feeds it the requests of the GPU test and compares the results with the numpy mirror, bit for bit.
//   loudness_host_check IN OUT [inplace] [yoff=K]
// IN : int64 {R, sub, n_x, n_y, total_runs, max_n}; rows R x 4 int64; tables 43 f64; params R x 2 f64; x n_x int16; y n_y int16
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
#define __forceinline__ inline
#define __restrict__
#define __shared__ static
#define __launch_bounds__(x)
static void __syncthreads() { g_bar->arrive_and_wait(); }
#define VV_LOUDNESS_HOST_CHECK
#include "../vietvoice-tts_amd/csrc/vv_loudness.hip"

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
    const long long R = hdr[0], sub = hdr[1], n_x = hdr[2], n_y = hdr[3], total_runs = hdr[4], max_n = hdr[5];
    long long* rows = block<long long>(4 * R);
    double* tables = block<double>(43);
    double* params = block<double>(2 * R);
    int16_t* x = block<int16_t>(n_x);
    int16_t* ybase = block<int16_t>(n_y + yoff);         // malloc aligns to 16 bytes: y = ybase + yoff sits 2 * yoff bytes past that
    int16_t* y = ybase + yoff;
    if (fread(rows, 8, 4 * R, f) != (size_t)(4 * R) || fread(tables, 8, 43, f) != 43 || fread(params, 8, 2 * R, f) != (size_t)(2 * R) ||
        fread(x, 2, n_x, f) != (size_t)n_x || fread(y, 2, n_y, f) != (size_t)n_y) return 2;
    fclose(f);
    const long long tr = total_runs > 0 ? total_runs : 1;
    char* ws = block<char>(56 * tr);
    memset(ws, 0xCD, 56 * tr);
    double* state = (double*)ws;
    double* power = state + 4 * total_runs;
    double* qbuf = power + total_runs;
    long long* peak = (long long*)(qbuf + total_runs);
    double* stats = block<double>(4 * R);
    const int rps = (int)((sub + RUN - 1) / RUN);
    if (total_runs > 0) {
        const unsigned blocks = (unsigned)((total_runs + RPB - 1) / RPB);
        launch(dim3(blocks), RPB, [&]() { loud_run_kernel<0>(x, n_x, rows, (int)R, sub, rps, total_runs, tables, state, power, peak); });
        launch(dim3((unsigned)R), 64, [&]() { loud_scan_kernel(rows, sub, rps, total_runs, tables, state); });
        launch(dim3(blocks), RPB, [&]() { loud_run_kernel<1>(x, n_x, rows, (int)R, sub, rps, total_runs, tables, state, power, peak); });
    }
    launch(dim3((unsigned)R), 256, [&]() { loud_gate_kernel(rows, sub, rps, total_runs, tables, params, power, peak, qbuf, state, stats); });
    int16_t* dst = in_place ? x : y;
    const long long n_dst = in_place ? n_x : n_y;
    if (max_n > 0) {
        long long bx = (max_n / 4 + 256) / 256;
        if (bx > 8) bx = 8;                              // fewer workgroups than the device launches: the grid-stride loop covers the rest
        launch(dim3((unsigned)bx, (unsigned)R), 256, [&]() { loud_apply_kernel(x, n_x, rows, stats, dst, n_dst); });
    }
    f = fopen(argv[2], "wb");
    if (!f) return 2;
    fwrite(stats, 8, 4 * R, f);
    fwrite(dst, 2, n_dst, f);
    fclose(f);
    free(rows); free(tables); free(params); free(x); free(ybase); free(ws); free(stats);
    return 0;
}
