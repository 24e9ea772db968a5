// Host stand-ins for the HIP names the PCM-stage, ingest, edit, elementwise, mel and noise kernels use, for the tools/*_host_check.cpp programs: a .hip file's
// kernels are compiled for the CPU (its includes and launchers sit behind #ifndef VV_*_HOST_CHECK) and run one OS thread per GPU thread
// of a workgroup, workgroups one after the other, so that -fsanitize=address,undefined sees an index past the end of an exact-size heap
// block and -fsanitize=thread sees an LDS write and a read with no barrier between them.  Build with -std=c++20 -ffp-contract=off.
//
//   launch(grid, block, shmem_bytes, f)   f() = the kernel call; the threads of a block size are made once and kept over workgroups
//                                         and launches; dynamic LDS is an exact-size block of shmem_bytes, fresh per launch
//   exact_block<T>(n, byte_off)           n elements whose LAST byte is the allocation's last byte; the first sits byte_off bytes past
//                                         a 16-byte boundary (destinations at +2, +4, +6); release with exact_free
//
// A thread that returns from the kernel leaves the workgroup's barrier and its wave's, so the others pass theirs (a kernel may return
// early per thread, per wave, or with all lanes but a few).
// __shfl_xor and __shfl are WAVE-SCOPED exchanges: threads threadIdx.x >> 6 form a wave of 64 lanes (blockDim.x % 64 in a short last
// wave) with a barrier of its own; write a slot, wave barrier, read, wave barrier.  A wave barrier orders nothing between waves: what
// crosses waves through LDS still needs the kernel's own __syncthreads, and the thread build reports it when that is missing.  A
// shuffle that only part of a wave's live lanes reach would wait for ever: run every program under a time limit.  A lane that reads
// the slot of a lane that has returned, or that lies past the wave, gets a stale or its own value, as on the device it gets an
// undefined one.  __syncthreads_or is workgroup-wide.
#pragma once
#define VV_HIP_HOST_SHIM
#include <algorithm>
#include <cmath>
#include <condition_variable>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <functional>
#include <map>
#include <memory>
#include <mutex>
#include <thread>
#include <vector>

struct dim3 { unsigned x = 1, y = 1, z = 1; dim3(unsigned a = 1, unsigned b = 1, unsigned c = 1) : x(a), y(b), z(c) {} };
struct alignas(8) uint2 { uint32_t x, y; };
struct alignas(16) uint4 { uint32_t x, y, z, w; };
struct alignas(16) float4 { float x, y, z, w; };
struct alignas(8) float2 { float x, y; };
static inline float4 make_float4(float x, float y, float z, float w) { return float4{x, y, z, w}; }
static inline uint4 make_uint4(uint32_t x, uint32_t y, uint32_t z, uint32_t w) { return uint4{x, y, z, w}; }
static thread_local dim3 threadIdx, blockIdx, gridDim, blockDim;
#define __global__
#define __device__
#define __host__
#define __forceinline__ inline
#define __restrict__
#define __shared__ static
#define __launch_bounds__(x)
using std::max;
using std::min;

namespace vv_host {

// A barrier whose count a returning thread leaves; mutex and condition variable, which every sanitizer understands.  Two mutexes, taken
// in turn: a thread that is still waking up from barrier k must not meet, on the mutex it re-locks, a thread that already arrives at
// barrier k + 1 -- the thread sanitizer would take that for an ordering between what the second did behind barrier k and what the first
// does behind it, and a kernel's missing barrier would go unseen (seen with np_buffer_sum's first barrier taken out).
struct Barrier {
    std::mutex m[2];
    std::condition_variable cv[2];
    int expected = 0, waiting = 0, phase = 0;       // phase: read without the lock by a thread the barrier cannot complete without
    void wait() {
        const int p = phase;
        std::unique_lock<std::mutex> l(m[p]);
        if (++waiting >= expected) { waiting = 0; phase = p ^ 1; cv[p].notify_all(); return; }
        cv[p].wait(l, [&] { return phase != p; });
    }
    void leave() {
        const int p = phase;
        std::unique_lock<std::mutex> l(m[p]);
        --expected;
        if (waiting > 0 && waiting >= expected) { waiting = 0; phase = p ^ 1; cv[p].notify_all(); }
    }
};

struct Pool {
    const int n;
    Barrier work, wg, gate, done;                   // work: __syncthreads of the running workgroup (a returned thread has left it);
    Barrier wave[16];                               // wave: the exchange of one wave's shuffles (a returned lane has left it);
    std::vector<std::thread> th;                    // wg: between workgroups; gate / done: the n workers and the launcher
    dim3 grid, block;
    const std::function<void()>* f = nullptr;
    bool quit = false;
    explicit Pool(int n_) : n(n_) {
        work.expected = wg.expected = n;
        arm_waves();
        gate.expected = done.expected = n + 1;
        for (int t = 0; t < n; ++t) th.emplace_back([this, t] { run(t); });
    }
    ~Pool() {
        quit = true;
        gate.wait();
        for (auto& x : th) x.join();
    }
    void arm_waves() { for (int w = 0; w * 64 < n; ++w) wave[w].expected = std::min(64, n - w * 64); }
    void run(int t);
    void launch(dim3 g, dim3 b, const std::function<void()>& fn) {
        grid = g; block = b; f = &fn;
        gate.wait();
        done.wait();
    }
};

static Pool* g_pool = nullptr;                      // the pool of the running launch
static unsigned char* g_lds = nullptr;              // its dynamic LDS
static uint64_t g_slot[1024];                       // __shfl_xor, __shfl
static int g_or = 0;                                // __syncthreads_or

inline void Pool::run(int t) {
    for (;;) {
        gate.wait();
        if (quit) return;
        for (unsigned bz = 0; bz < grid.z; ++bz)
            for (unsigned by = 0; by < grid.y; ++by)
                for (unsigned bx = 0; bx < grid.x; ++bx) {
                    threadIdx = dim3((unsigned)t); blockIdx = dim3(bx, by, bz); gridDim = grid; blockDim = block;
                    (*f)();
                    work.leave();
                    wave[t >> 6].leave();
                    wg.wait();                      // the workgroup is over: the next one reuses the static "shared" arrays
                    if (t == 0) { work.expected = n; arm_waves(); }
                    wg.wait();
                }
        done.wait();
    }
}

template <typename T> T* exact_block(long long n, int byte_off = 0) {
    const size_t bytes = sizeof(T) * (size_t)(n > 0 ? n : 0);
    void* raw = nullptr;
    if (posix_memalign(&raw, 16, bytes + (size_t)byte_off)) { fprintf(stderr, "out of memory\n"); exit(2); }
    return (T*)((unsigned char*)raw + byte_off);
}
template <typename T> void exact_free(T* p, int byte_off = 0) { if (p) free((unsigned char*)p - byte_off); }

inline Pool* pool_of(int n) {
    static std::map<int, std::unique_ptr<Pool>> pools;          // one pool per block size, joined when the program ends
    auto& p = pools[n];
    if (!p) p.reset(new Pool(n));
    return p.get();
}

template <typename F> void launch(dim3 grid, dim3 block, size_t shmem_bytes, F f) {
    const int n = (int)block.x;
    if (block.y != 1 || block.z != 1 || n < 1 || n > 1024) { fprintf(stderr, "launch: blocks are 1-D, up to 1024 threads\n"); exit(2); }
    if (!grid.x || !grid.y || !grid.z) return;
    Pool* p = pool_of(n);
    g_pool = p;
    g_lds = shmem_bytes ? exact_block<unsigned char>((long long)shmem_bytes) : nullptr;
    const std::function<void()> fn = f;
    p->launch(grid, block, fn);
    exact_free(g_lds);
    g_lds = nullptr;
}

inline unsigned char* dynamic_lds() { return g_lds; }

}  // namespace vv_host

static inline void __syncthreads() { vv_host::g_pool->work.wait(); }
static inline int __syncthreads_or(int pred) {
    if (pred) __atomic_fetch_or(&vv_host::g_or, 1, __ATOMIC_RELAXED);
    __syncthreads();
    const int r = __atomic_load_n(&vv_host::g_or, __ATOMIC_RELAXED);
    __syncthreads();
    if (threadIdx.x == 0) __atomic_store_n(&vv_host::g_or, 0, __ATOMIC_RELAXED);
    __syncthreads();
    return r;
}
namespace vv_host {
template <typename T> inline T wave_exchange(T v, unsigned src_lane) {
    static_assert(sizeof(T) == 4 || sizeof(T) == 8, "32-bit and 64-bit values");
    const unsigned t = threadIdx.x, w0 = t & ~63u;
    Barrier& wb = g_pool->wave[t >> 6];
    memcpy(&g_slot[t], &v, sizeof(T));
    wb.wait();
    T r = v;
    if (src_lane < 64 && w0 + src_lane < blockDim.x) memcpy(&r, &g_slot[w0 + src_lane], sizeof(T));
    wb.wait();
    return r;
}
}  // namespace vv_host
template <typename T> static inline T __shfl_xor(T v, int o) { return vv_host::wave_exchange(v, (threadIdx.x & 63u) ^ (unsigned)o); }
template <typename T> static inline T __shfl(T v, int src) { return vv_host::wave_exchange(v, (unsigned)src & 63u); }
template <typename T> static inline T atomicAdd(T* p, T v) { return __atomic_fetch_add(p, v, __ATOMIC_RELAXED); }
template <typename T> static inline T atomicMax(T* p, T v) {
    T old = __atomic_load_n(p, __ATOMIC_RELAXED);
    while (old < v && !__atomic_compare_exchange_n(p, &old, v, true, __ATOMIC_RELAXED, __ATOMIC_RELAXED)) {}
    return old;
}
static inline unsigned __brev(unsigned v) { return __builtin_bitreverse32(v); }
static inline unsigned __float_as_uint(float f) { unsigned u; memcpy(&u, &f, 4); return u; }
static inline float __uint_as_float(unsigned u) { float f; memcpy(&f, &u, 4); return f; }
// separately rounded: the build has -ffp-contract=off, so no fma forms across these calls
static inline double __dmul_rn(double a, double b) { return a * b; }
static inline double __dadd_rn(double a, double b) { return a + b; }
static inline double __ddiv_rn(double a, double b) { return a / b; }
// Stand-ins, NOT the device's functions: a host result through one of these speaks for the indexing and the barriers of its path only.
static inline float rsqrtf(float x) { return 1.0f / sqrtf(x); }
static inline float cospif(float x) { return (float)cos(M_PI * (double)x); }     // in double, rounded once
static inline float sinpif(float x) { return (float)sin(M_PI * (double)x); }
static inline float vv_host_exp2f(float x) { return exp2f(x); }                   // act_apply's Mish branch (vv_common.h)
static inline float vv_host_rcpf(float x) { return 1.0f / x; }
