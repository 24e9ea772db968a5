// Host check of csrc/vv_output.hip: join, output rate and G.711 compiled for the CPU on tools/hip_host_shim.h, every
// buffer an exact-size heap block (flags and gains, one scratch on the device, are two blocks here; the walk's LDS ring is a block of
// the 512 + 2 C bytes the launcher asks for).  tools/output_host_check.py builds this file with -fsanitize=address,undefined or
// -fsanitize=thread, feeds it the cases and compares with the host mirrors.  Every block is filled with 0xAA before it is read into.
//   output_host_check join IN OUT      IN : int64 {n_pcm, n_chunks, R, n_fade, n_out, max_n, body_bx}; chunk rows n_chunks x 8 int64;
//                                           request rows R x 4 int64; fade n_fade f64; pcm n_pcm int16
//                                      OUT: flags n_chunks int32; gains n_chunks f32; out n_out int16
//   output_host_check resample IN OUT  IN : int64 {n_x, n_rows, n_taps, up, down, skip, n_y, bx}; rows n_rows x 6 int64; taps f64; x int16
//                                      OUT: y n_y int16
//   output_host_check encode IN OUT    IN : int64 {n_x, n_rows, kind, n_y, bx}; rows n_rows x 3 int64; x int16       OUT: y n_y uint8
// body_bx / bx = workgroups along x: fewer than the device launches, so that the grid-stride loops take further trips.
#include "hip_host_shim.h"
#define VV_OUTPUT_HOST_CHECK
#include "../vietvoice-tts_amd/csrc/vv_output.hip"

using vv_host::exact_block;
using vv_host::exact_free;
using vv_host::launch;

template <typename T> static T* filled(long long n) {
    T* p = exact_block<T>(n);
    if (n > 0) memset(p, 0xAA, sizeof(T) * (size_t)n);
    return p;
}
template <typename T> static bool rd(FILE* f, T* p, long long n) { return n <= 0 || fread(p, sizeof(T), (size_t)n, f) == (size_t)n; }
template <typename T> static void wr(FILE* f, const T* p, long long n) { if (n > 0) fwrite(p, sizeof(T), (size_t)n, f); }

static int join(FILE* f, const char* path) {
    long long h[7];
    if (!rd(f, h, 7)) return 2;
    const long long n_pcm = h[0], n_chunks = h[1], R = h[2], n_fade = h[3], n_out = h[4], max_n = h[5], body_bx = h[6];
    if (R < 1 || n_chunks < R || n_chunks > 65535 || max_n < 0 || max_n > JOIN_MAX_N || body_bx < 1) return 2;
    long long* rows = filled<long long>(8 * n_chunks);
    long long* reqs = filled<long long>(4 * R);
    double* fade = filled<double>(n_fade);
    int16_t* pcm = filled<int16_t>(n_pcm);
    int16_t* out = filled<int16_t>(n_out);
    int* flags = filled<int>(n_chunks);
    float* gains = filled<float>(n_chunks);
    if (!rd(f, rows, 8 * n_chunks) || !rd(f, reqs, 4 * R) || !rd(f, fade, n_fade) || !rd(f, pcm, n_pcm)) return 2;
    fclose(f);
    const int C = max_n > 8 ? (int)((max_n + 7) / 8 * 8) : 8;
    launch(dim3((unsigned)n_chunks), 256, 0, [&]() { join_flag_kernel(pcm, n_pcm, rows, flags); });
    launch(dim3((unsigned)R), 256, 512 + 2 * (size_t)C,
           [&]() { join_walk_kernel(pcm, n_pcm, rows, reqs, fade, n_fade, flags, gains, out, n_out, C, (int)n_chunks); });
    launch(dim3((unsigned)body_bx, (unsigned)n_chunks), 256, 0, [&]() { join_body_kernel(pcm, n_pcm, rows, reqs, flags, gains, out, n_out, (int)R); });
    f = fopen(path, "wb");
    if (!f) return 2;
    wr(f, flags, n_chunks); wr(f, gains, n_chunks); wr(f, out, n_out);
    fclose(f);
    exact_free(rows); exact_free(reqs); exact_free(fade); exact_free(pcm); exact_free(out); exact_free(flags); exact_free(gains);
    return 0;
}

static int resample(FILE* f, const char* path) {
    long long h[8];
    if (!rd(f, h, 8)) return 2;
    const long long n_x = h[0], n_rows = h[1], n_taps = h[2], up = h[3], down = h[4], skip = h[5], n_y = h[6], bx = h[7];
    if (n_rows < 1 || n_taps < 1 || up < 1 || down < 1 || skip < 0 || bx < 1) return 2;
    long long* rows = filled<long long>(6 * n_rows);
    double* taps = filled<double>(n_taps);
    int16_t* x = filled<int16_t>(n_x);
    int16_t* y = filled<int16_t>(n_y);
    if (!rd(f, rows, 6 * n_rows) || !rd(f, taps, n_taps) || !rd(f, x, n_x)) return 2;
    fclose(f);
    launch(dim3((unsigned)bx, (unsigned)n_rows), 256, 0,
           [&]() { pcm_resample_kernel(x, n_x, rows, taps, (int)n_taps, (int)up, (int)down, (int)skip, y, n_y); });
    f = fopen(path, "wb");
    if (!f) return 2;
    wr(f, y, n_y);
    fclose(f);
    exact_free(rows); exact_free(taps); exact_free(x); exact_free(y);
    return 0;
}

static int encode(FILE* f, const char* path) {
    long long h[5];
    if (!rd(f, h, 5)) return 2;
    const long long n_x = h[0], n_rows = h[1], kind = h[2], n_y = h[3], bx = h[4];
    if (n_rows < 1 || (kind != 1 && kind != 2) || bx < 1) return 2;
    long long* rows = filled<long long>(3 * n_rows);
    int16_t* x = filled<int16_t>(n_x);
    uint8_t* y = filled<uint8_t>(n_y);
    if (!rd(f, rows, 3 * n_rows) || !rd(f, x, n_x)) return 2;
    fclose(f);
    const dim3 grid((unsigned)bx, (unsigned)n_rows);
    if (kind == 1) launch(grid, 256, 0, [&]() { pcm_encode_kernel<1>(x, n_x, rows, y, n_y); });
    else launch(grid, 256, 0, [&]() { pcm_encode_kernel<2>(x, n_x, rows, y, n_y); });
    f = fopen(path, "wb");
    if (!f) return 2;
    wr(f, y, n_y);
    fclose(f);
    exact_free(rows); exact_free(x); exact_free(y);
    return 0;
}

int main(int argc, char** argv) {
    if (argc < 4) return 2;
    FILE* f = fopen(argv[2], "rb");
    if (!f) return 2;
    if (!strcmp(argv[1], "join")) return join(f, argv[3]);
    if (!strcmp(argv[1], "resample")) return resample(f, argv[3]);
    if (!strcmp(argv[1], "encode")) return encode(f, argv[3]);
    return 2;
}
