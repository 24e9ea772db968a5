// Host check of csrc/vv_denoise.hip with csrc/vv_denoise_fft.h: the kernels compiled for the CPU on
// tools/hip_host_shim.h, every buffer an exact-size heap block; the scratch is one block of exactly vvk_pcm_denoise_ws_bytes or
// vvk_pcm_denoise_bias_ws_bytes, laid out as the launcher lays it out.  tools/denoise_host_check.py builds this file with
// -fsanitize=address,undefined or -fsanitize=thread, feeds it the cases and compares with the host mirror.  Every block is filled with
// 0xAA before it is read into.
//   denoise_host_check denoise IN OUT  IN : int64 {n_x, R, n_y, n_bias, total_frames, max_hops, y_byte_off}; rows R x 4 int64; strengths R
//                                           f64; bias n_bias x 513 f64; window 1024 f64; twiddles 1024 f64; x n_x int16
//                                      OUT: y n_y int16; mag total_frames x 1024 f64      (y starts y_byte_off past a 16-byte boundary)
//   denoise_host_check bias IN OUT     IN : int64 {n_x, R, total_frames, max_frames}; rows R x 4 int64; window; twiddles; x n_x int16
//                                      OUT: out R x 513 f64
// The grids are the device's: none of these kernels has a grid-stride loop.
#include "hip_host_shim.h"
#define VV_DENOISE_HOST_CHECK
#include "../vietvoice-tts_amd/csrc/vv_denoise.hip"

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

static int denoise(FILE* f, const char* path) {
    long long h[7];
    if (!rd(f, h, 7)) return 2;
    const long long n_x = h[0], R = h[1], n_y = h[2], n_bias = h[3], total_frames = h[4], max_hops = h[5];
    const int yoff = (int)h[6];
    if (R < 1 || R > 65535 || n_bias < 1 || total_frames < 3 || max_hops < 1 || max_hops > total_frames || yoff < 0 || yoff > 14 || yoff % 2) return 2;
    long long* rows = filled<long long>(4 * R);
    double* strengths = filled<double>(R);
    double* bias = filled<double>(n_bias * DB);
    double* window = filled<double>(DN);
    double* tw = filled<double>(DN);
    int16_t* x = filled<int16_t>(n_x);
    int16_t* y = filled<int16_t>(n_y, yoff);
    double* mag = filled<double>(total_frames * DN);
    long long* plan = (long long*)filled<unsigned char>((long long)vvk_pcm_denoise_ws_bytes((int)R));
    if (!rd(f, rows, 4 * R) || !rd(f, strengths, R) || !rd(f, bias, n_bias * DB) || !rd(f, window, DN) || !rd(f, tw, DN) || !rd(f, x, n_x)) return 2;
    fclose(f);
    launch(dim3(1), 64, 0, [&]() { denoise_plan_kernel(rows, strengths, (int)R, n_x, n_y, n_bias, total_frames, plan); });
    launch(dim3((unsigned)max_hops, (unsigned)R), 256, 0, [&]() { denoise_kernel(x, rows, plan, strengths, bias, window, tw, y, mag); });
    f = fopen(path, "wb");
    if (!f) return 2;
    wr(f, y, n_y); wr(f, mag, total_frames * DN);
    fclose(f);
    exact_free(rows); exact_free(strengths); exact_free(bias); exact_free(window); exact_free(tw); exact_free(x); exact_free(y, yoff);
    exact_free(mag); exact_free((unsigned char*)plan);
    return 0;
}

static int bias_of(FILE* f, const char* path) {
    long long h[4];
    if (!rd(f, h, 4)) return 2;
    const long long n_x = h[0], R = h[1], total_frames = h[2], max_frames = h[3];
    if (R < 1 || R > 65535 || total_frames < 1 || max_frames < 1 || max_frames > total_frames) return 2;
    long long* rows = filled<long long>(4 * R);
    double* window = filled<double>(DN);
    double* tw = filled<double>(DN);
    int16_t* x = filled<int16_t>(n_x);
    double* out = filled<double>(R * DB);
    unsigned char* ws = filled<unsigned char>((long long)vvk_pcm_denoise_bias_ws_bytes(total_frames, (int)R));
    if (!rd(f, rows, 4 * R) || !rd(f, window, DN) || !rd(f, tw, DN) || !rd(f, x, n_x)) return 2;
    fclose(f);
    long long* plan = (long long*)ws;                                            // the launcher's layout
    double* mags = (double*)(plan + 2 * R);
    launch(dim3(1), 64, 0, [&]() { denoise_bias_plan_kernel(rows, (int)R, n_x, total_frames, plan); });
    launch(dim3((unsigned)max_frames, (unsigned)R), 256, 0, [&]() { denoise_bias_frames_kernel(x, rows, plan, window, tw, mags); });
    launch(dim3((unsigned)((R * DB + 255) / 256)), 256, 0, [&]() { denoise_bias_mean_kernel(plan, mags, (int)R, out); });
    f = fopen(path, "wb");
    if (!f) return 2;
    wr(f, out, R * DB);
    fclose(f);
    exact_free(rows); exact_free(window); exact_free(tw); exact_free(x); exact_free(out); exact_free(ws);
    return 0;
}

int main(int argc, char** argv) {
    if (argc < 4) return 2;
    FILE* f = fopen(argv[2], "rb");
    if (!f) return 2;
    if (!strcmp(argv[1], "denoise")) return denoise(f, argv[3]);
    if (!strcmp(argv[1], "bias")) return bias_of(f, argv[3]);
    return 2;
}
