// Host check of csrc/vv_flac_decode.hip: the kernels compiled for the CPU with stand-ins for the HIP keywords, every buffer
// an exact-size heap block -- so that address and undefined-behaviour sanitizers see a read or a write past an end, whatever the bytes
// of the streams say.  tools/flac_decode_host_check.py builds this file with -fsanitize=address,undefined, feeds it valid and malformed
// streams and compares the result with the Python mirror.
//   flac_decode_host_check IN OUT
// IN : int64 {R, n_bytes}; rows R x 8 int64; data n_bytes (the clips 4-byte aligned, 8 bytes of padding behind the last)
// OUT: info R x 4 int64; info2 R x 2 int64; lay R x 6 int64; int64 n_pcm; pcm n_pcm bytes
// A kernel with __syncthreads runs one std::thread per GPU thread (kept over the workgroups, a barrier between them; no thread of these
// kernels returns in front of a barrier); a kernel without runs its threads one after the other.  The per-candidate grid is cut to the
// candidates found (the device launches it for the most there can be; the workgroups behind the count return at once).
#include <barrier>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <thread>
#include <vector>

struct dim3 { unsigned x = 1, y = 1, z = 1; dim3(unsigned a = 1, unsigned b = 1, unsigned c = 1) : x(a), y(b), z(c) {} };
static thread_local dim3 threadIdx, blockIdx;
static std::barrier<>* g_bar;
#define __global__
#define __device__
#define __host__
#define __forceinline__ inline
#define __restrict__
#define __shared__ static
#define __launch_bounds__(x)
static void __syncthreads() { g_bar->arrive_and_wait(); }
#define VV_FLAC_HOST_CHECK
#include "../vietvoice-tts_amd/csrc/vv_flac_decode.hip"

template <typename F> static void launch_sync(unsigned blocks, int nthreads, F f) {
    std::barrier<> bar(nthreads);
    g_bar = &bar;
    std::vector<std::thread> th;
    for (int t = 0; t < nthreads; ++t)
        th.emplace_back([=]() {
            for (unsigned b = 0; b < blocks; ++b) {
                threadIdx = dim3(t); blockIdx = dim3(b);
                f();
                g_bar->arrive_and_wait();              // the next workgroup reuses the static "shared" arrays
            }
        });
    for (auto& x : th) x.join();
}

template <typename F> static void launch(unsigned blocks, int nthreads, F f) {
    for (unsigned b = 0; b < blocks; ++b)
        for (int t = 0; t < nthreads; ++t) { threadIdx = dim3(t); blockIdx = dim3(b); f(); }
}

template <typename T> static T* block(long long n) { return (T*)malloc(sizeof(T) * (size_t)(n > 0 ? n : 1)); }

int main(int argc, char** argv) {
    if (argc < 3) return 2;
    FILE* f = fopen(argv[1], "rb");
    if (!f) return 2;
    long long hdr[2];
    if (fread(hdr, 8, 2, f) != 2) return 2;
    const long long R = hdr[0], n_bytes = hdr[1];
    if (R < 1 || R > 65535 || n_bytes < 8 || n_bytes > MAX_BYTES) return 2;
    long long* rows = block<long long>(8 * R);
    uint8_t* data = (uint8_t*)aligned_alloc(8, (size_t)((n_bytes + 7) / 8 * 8));
    if (fread(rows, 8, 8 * R, f) != (size_t)(8 * R) || fread(data, 1, n_bytes, f) != (size_t)n_bytes) return 2;
    fclose(f);
    const unsigned long long ws_bytes = ws_layout(nullptr, n_bytes, (int)R).bytes;
    void* ws = malloc(ws_bytes);
    memset(ws, 0xAA, ws_bytes);
    const Ws w = ws_layout(ws, n_bytes, (int)R);
    long long* info = block<long long>(4 * R);
    launch_sync(w.nb, NT, [&]() { flac_scan_count_kernel(data, n_bytes, rows, (int)R, w.counts); });
    launch_sync(1, NT, [&]() { flac_scan_offsets_kernel(w.counts, w.nb); });
    launch_sync(w.nb, NT, [&]() { flac_scan_write_kernel(data, n_bytes, rows, (int)R, w.counts, w.cand, w.cap); });
    const long long count = w.counts[w.nb];
    launch_sync((unsigned)((count + MT - 1) / MT + 1), MT,
                [&]() { flac_measure_kernel(data, n_bytes, rows, (int)R, w.counts, w.nb, w.cand, w.cap, w.rec, w.sub); });
    launch((unsigned)((R + MT - 1) / MT), MT,
           [&]() { flac_chain_kernel(data, n_bytes, rows, (int)R, w.counts, w.nb, w.cand, w.cap, w.rec, w.gen, w.s0, w.clip, info); });
    // the host's part between the two calls: the layout of the clips that passed
    long long* lay = block<long long>(6 * R);
    long long F = 0, S = 0, P = 0, n_pcm = 0;
    int maxch = 1;
    for (long long r = 0; r < R; ++r) {
        const bool ok = info[4 * r] == 0;
        const long long frames = ok ? info[4 * r + 2] : 0, samples = ok ? info[4 * r + 3] : 0, ch = rows[8 * r + 2], bits = rows[8 * r + 3];
        long long* l = lay + 6 * r;
        l[0] = n_pcm; l[1] = frames; l[2] = samples; l[3] = F; l[4] = P; l[5] = S;
        F += frames; S += samples; P += samples * ch;
        n_pcm += (samples * ch * (bits == 24 ? 4 : bits / 8) + 3) / 4 * 4;
        if (ch > maxch) maxch = (int)ch;
    }
    int* plane = block<int>(P);
    int* fst = block<int>(MAXCH * F);
    uint8_t* pcm = block<uint8_t>(n_pcm);
    long long* info2 = block<long long>(2 * R);
    memset(pcm, 0xAA, (size_t)(n_pcm > 0 ? n_pcm : 1));
    if (F)
        launch((unsigned)((F * maxch + MT - 1) / MT), MT, [&]() {
            flac_restore_kernel(data, n_bytes, rows, (int)R, lay, F, maxch, w.counts, w.nb, w.cand, w.cap, w.rec, w.sub, w.gen, w.s0, w.clip, plane, P, n_pcm, fst);
        });
    launch((unsigned)((R + MT - 1) / MT), MT,
           [&]() { flac_verdict_kernel(rows, (int)R, n_bytes, lay, F, w.counts, w.nb, w.cand, w.cap, w.gen, w.clip, P, n_pcm, fst, info2); });
    if (S)
        launch((unsigned)((S + MT - 1) / MT), MT, [&]() {
            flac_interleave_kernel(rows, (int)R, n_bytes, lay, S, w.counts, w.nb, w.cand, w.cap, w.rec, w.gen, w.s0, w.clip, plane, P, pcm, n_pcm);
        });
    f = fopen(argv[2], "wb");
    if (!f) return 2;
    fwrite(info, 8, 4 * R, f);
    fwrite(info2, 8, 2 * R, f);
    fwrite(lay, 8, 6 * R, f);
    fwrite(&n_pcm, 8, 1, f);
    fwrite(pcm, 1, n_pcm, f);
    fclose(f);
    free(rows); free(data); free(ws); free(info); free(lay); free(plane); free(fst); free(pcm); free(info2);
    return 0;
}
