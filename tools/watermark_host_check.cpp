// Host check of csrc/vv_watermark.hip with csrc/vv_denoise_fft.h: the embedder and the detector compiled for the CPU on
// tools/hip_host_shim.h, every buffer an exact-size heap block; the scratch is one block of exactly vvk_pcm_watermark_ws_bytes or
// vvk_pcm_watermark_detect_ws_bytes, laid out as the launcher lays it out (the detector's cells stay in it).
// tools/watermark_host_check.py builds this file with -fsanitize=address,undefined or -fsanitize=thread, feeds it the cases and compares
// with the host mirror.  Every block is filled with 0xAA before it is read into.
//   watermark_host_check embed IN OUT   IN : int64 {n_x, R, n_y, total_frames, max_hops, y_byte_off}; f64 {gp, gm}; rows R x 4 int64; chips
//                                            64 x 320 int8; window 1024 f64; twiddles 1024 f64; x n_x int16
//                                       OUT: y n_y int16                                   (y starts y_byte_off past a 16-byte boundary)
//   watermark_host_check detect IN OUT  IN : int64 {n_x, R, total_frames, max_frames}; rows R x 4 int64; chips; window; twiddles; x n_x int16
//                                       OUT: stats R x 256 x 24 x 2 int64; cells total_frames x 320 int32
// The grids are the device's: none of these kernels has a grid-stride loop.
#include "hip_host_shim.h"
#define VV_WATERMARK_HOST_CHECK
#include "../vietvoice-tts_amd/csrc/vv_watermark.hip"

using vv_host::exact_block;
using vv_host::exact_free;
using vv_host::launch;

template <typename T> static T* filled(long long n, int byte_off = 0) {
    T* p = exact_block<T>(n, byte_off);
    if (n > 0) memset(p, 0xAA, sizeof(T) * (size_t)n);
    return p;
}
template <typename T> static bool rd(FILE* f, T* p, long long n) { return n <= 0 || fread(p, sizeof(T), (size_t)n, f) == (size_t)n; }
template <typename T> static void wr(FILE* f, const T* p, long long n) { if (n > 0) fwrite(p, sizeof(T), (size_t)n, f); }

static int embed(FILE* f, const char* path) {
    long long h[6];
    double g[2];
    if (!rd(f, h, 6) || !rd(f, g, 2)) return 2;
    const long long n_x = h[0], R = h[1], n_y = h[2], total_frames = h[3], max_hops = h[4];
    const int yoff = (int)h[5];
    if (R < 1 || R > 65535 || total_frames < 3 || max_hops < 1 || max_hops > total_frames || yoff < 0 || yoff > 14 || yoff % 2) return 2;
    long long* rows = filled<long long>(4 * R);
    signed char* chips = filled<signed char>(WP * WK);
    double* window = filled<double>(DN);
    double* tw = filled<double>(DN);
    int16_t* x = filled<int16_t>(n_x);
    int16_t* y = filled<int16_t>(n_y, yoff);
    long long* plan = (long long*)filled<unsigned char>((long long)vvk_pcm_watermark_ws_bytes((int)R));
    if (!rd(f, rows, 4 * R) || !rd(f, chips, WP * WK) || !rd(f, window, DN) || !rd(f, tw, DN) || !rd(f, x, n_x)) return 2;
    fclose(f);
    launch(dim3(1), 64, 0, [&]() { watermark_plan_kernel(rows, (int)R, n_x, n_y, total_frames, plan); });
    launch(dim3((unsigned)max_hops, (unsigned)R), 256, 0, [&]() { watermark_kernel(x, rows, plan, chips, g[0], g[1], window, tw, y); });
    f = fopen(path, "wb");
    if (!f) return 2;
    wr(f, y, n_y);
    fclose(f);
    exact_free(rows); exact_free(chips); exact_free(window); exact_free(tw); exact_free(x); exact_free(y, yoff); exact_free((unsigned char*)plan);
    return 0;
}

static int detect(FILE* f, const char* path) {
    long long h[4];
    if (!rd(f, h, 4)) return 2;
    const long long n_x = h[0], R = h[1], total_frames = h[2], max_frames = h[3];
    if (R < 1 || R > 65535 || total_frames < 3 || max_frames < 3 || max_frames > total_frames) return 2;
    long long* rows = filled<long long>(4 * R);
    signed char* chips = filled<signed char>(WP * WK);
    double* window = filled<double>(DN);
    double* tw = filled<double>(DN);
    int16_t* x = filled<int16_t>(n_x);
    long long* stats = filled<long long>(R * WQ * 2 * WNB);
    unsigned char* ws = filled<unsigned char>((long long)vvk_pcm_watermark_detect_ws_bytes(total_frames, (int)R));
    if (!rd(f, rows, 4 * R) || !rd(f, chips, WP * WK) || !rd(f, window, DN) || !rd(f, tw, DN) || !rd(f, x, n_x)) return 2;
    fclose(f);
    long long* plan = (long long*)ws;                                            // the launcher's layout
    double* mags = (double*)(plan + 2 * R);
    int* cells = (int*)(mags + total_frames * WK);
    launch(dim3(1), 64, 0, [&]() { detect_plan_kernel(rows, (int)R, n_x, total_frames, plan); });
    launch(dim3((unsigned)max_frames, (unsigned)R), 256, 0, [&]() { detect_frames_kernel(x, rows, plan, window, tw, mags); });
    launch(dim3((unsigned)((max_frames * WK + 255) / 256), (unsigned)R), 256, 0, [&]() { detect_cells_kernel(plan, mags, cells); });
    launch(dim3(WQ, (unsigned)R), 256, 0, [&]() { detect_stats_kernel(plan, cells, chips, stats); });
    f = fopen(path, "wb");
    if (!f) return 2;
    wr(f, stats, R * WQ * 2 * WNB); wr(f, cells, total_frames * WK);
    fclose(f);
    exact_free(rows); exact_free(chips); exact_free(window); exact_free(tw); exact_free(x); exact_free(stats); exact_free(ws);
    return 0;
}

int main(int argc, char** argv) {
    if (argc < 4) return 2;
    FILE* f = fopen(argv[2], "rb");
    if (!f) return 2;
    if (!strcmp(argv[1], "embed")) return embed(f, argv[3]);
    if (!strcmp(argv[1], "detect")) return detect(f, argv[3]);
    return 2;
}
