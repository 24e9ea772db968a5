// Host check of csrc/vv_prosody.hip: the two kernels compiled for the CPU, one std::thread per GPU thread of a
// workgroup, a barrier for __syncthreads, workgroups one after the other, every buffer an exact-size heap block -- so that address and
// undefined-behaviour sanitizers see an index past an end or a misaligned store.  tools/prosody_host_check.py builds this file with
// -fsanitize=address,undefined, feeds it the requests of the GPU test and compares the results with the numpy mirror, bit for bit.
//   prosody_host_check IN OUT [yoff=K]
// IN : int64 {R, n_x, n_y, n_pos}; rows R x 6 int64; window 512 f64; x n_x int16; y n_y int16
// OUT: pos n_pos int32; y n_y int16.   yoff = the destination starts K samples (2 K bytes) past an 8-byte boundary
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
#define VV_PROSODY_HOST_CHECK
#include "../vietvoice-tts_amd/csrc/vv_prosody.hip"

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
    long long yoff = 0;
    for (int i = 3; i < argc; ++i)
        if (!strncmp(argv[i], "yoff=", 5)) yoff = atoll(argv[i] + 5);
    FILE* f = fopen(argv[1], "rb");
    if (!f) return 2;
    long long hdr[4];
    if (fread(hdr, 8, 4, f) != 4) return 2;
    const long long R = hdr[0], n_x = hdr[1], n_y = hdr[2], n_pos = hdr[3];
    long long* rows = block<long long>(6 * R);
    double* window = block<double>(WN);
    int16_t* x = block<int16_t>(n_x);
    int16_t* ybase = block<int16_t>(n_y + yoff);         // malloc aligns to 16 bytes: y = ybase + yoff sits 2 * yoff bytes past that
    int16_t* y = ybase + yoff;
    if (fread(rows, 8, 6 * R, f) != (size_t)(6 * R) || fread(window, 8, WN, f) != (size_t)WN || fread(x, 2, n_x, f) != (size_t)n_x ||
        fread(y, 2, n_y, f) != (size_t)n_y)
        return 2;
    fclose(f);
    long long max_out = 0;
    for (long long r = 0; r < R; ++r) {
        const long long n_s = (rows[6 * r + 1] * rows[6 * r + 3] + rows[6 * r + 4] - 1) / rows[6 * r + 4];
        if (n_s > max_out) max_out = n_s;
    }
    int* pos = block<int>(n_pos);
    for (long long i = 0; i < n_pos; ++i) pos[i] = -1431655766;
    long long* plan = block<long long>(2 * R);
    launch(dim3((unsigned)R), NT, [&]() { stretch_search_kernel(x, n_x, rows, pos, n_pos, plan); });
    if (max_out > 0) {
        long long bx = (max_out / 4 + 256) / 256;
        if (bx > 3) bx = 3;                              // fewer workgroups than the device launches: the grid-stride loop covers the rest
        launch(dim3((unsigned)bx, (unsigned)R), 256, [&]() { stretch_blend_kernel(x, n_x, rows, window, pos, n_pos, plan, y, n_y); });
    }
    f = fopen(argv[2], "wb");
    if (!f) return 2;
    fwrite(pos, 4, n_pos, f);
    fwrite(y, 2, n_y, f);
    fclose(f);
    free(rows); free(window); free(x); free(ybase); free(pos); free(plan);
    return 0;
}
