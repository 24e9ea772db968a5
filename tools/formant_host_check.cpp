// Host check of csrc/vv_formant.hip: the four kernels compiled for the CPU on tools/hip_host_shim.h, every buffer an
// exact-size heap block; the scratch is one block of exactly vvk_pcm_formant_ws_bytes, laid out as the launcher lays it out (the taps
// stay in it).  tools/formant_host_check.py builds this file with -fsanitize=address,undefined or -fsanitize=thread, feeds it the cases
// and compares with the host mirror.  Every block is filled with 0xAA before it is read into.
//   formant_host_check IN OUT   IN : int64 {n_x, n_y, R, n_z, total_frames, max_frames, z_byte_off}; rows R x 7 int64; wa 1024 f64; g 25 f64;
//                                    window 512 f64; x n_x int16; y n_y int16
//                               OUT: z n_z int16; taps total_frames x 2048 f64             (z starts z_byte_off past a 16-byte boundary)
// The grids are the device's: none of these kernels has a grid-stride loop.
#include "hip_host_shim.h"
#define VV_FORMANT_HOST_CHECK
#include "../vietvoice-tts_amd/csrc/vv_formant.hip"

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

int main(int argc, char** argv) {
    if (argc < 3) return 2;
    FILE* f = fopen(argv[1], "rb");
    if (!f) return 2;
    long long h[7];
    if (!rd(f, h, 7)) return 2;
    const long long n_x = h[0], n_y = h[1], R = h[2], n_z = h[3], total_frames = h[4], max_frames = h[5];
    const int zoff = (int)h[6];
    if (R < 1 || R > 65535 || total_frames < 1 || max_frames < 1 || max_frames > total_frames || zoff < 0 || zoff > 14 || zoff % 2) return 2;
    long long* rows = filled<long long>(7 * R);
    double* wa = filled<double>(FNA);
    double* g = filled<double>(FP + 1);
    double* window = filled<double>(2 * FH);
    int16_t* x = filled<int16_t>(n_x);
    int16_t* y = filled<int16_t>(n_y);
    int16_t* z = filled<int16_t>(n_z, zoff);
    unsigned char* ws = filled<unsigned char>((long long)vvk_pcm_formant_ws_bytes(total_frames, (int)R));
    if (!rd(f, rows, 7 * R) || !rd(f, wa, FNA) || !rd(f, g, FP + 1) || !rd(f, window, 2 * FH) || !rd(f, x, n_x) || !rd(f, y, n_y)) return 2;
    fclose(f);
    long long* plan = (long long*)ws;                                            // the launcher's layout
    double* coef = (double*)(plan + 2 * R);
    double* taps = coef + total_frames * 2 * COEF;
    launch(dim3(1), 64, 0, [&]() { formant_plan_kernel(rows, (int)R, n_x, n_y, n_z, total_frames, plan); });
    launch(dim3((unsigned)max_frames, (unsigned)R, 2), 256, 0, [&]() { formant_analysis_kernel(x, y, rows, plan, wa, g, coef); });
    launch(dim3((unsigned)((max_frames + 63) / 64), (unsigned)R), 64, 0, [&]() { formant_filter_kernel(plan, coef, taps); });
    if (max_frames > 1) launch(dim3((unsigned)(max_frames - 1), (unsigned)R), 64, 0, [&]() { formant_apply_kernel(y, rows, plan, taps, window, z); });
    f = fopen(argv[2], "wb");
    if (!f) return 2;
    wr(f, z, n_z); wr(f, taps, total_frames * FL);
    fclose(f);
    exact_free(rows); exact_free(wa); exact_free(g); exact_free(window); exact_free(x); exact_free(y); exact_free(z, zoff); exact_free(ws);
    return 0;
}
