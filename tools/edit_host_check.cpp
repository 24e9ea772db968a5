// Host check of csrc/vv_edit.hip: the two kernels compiled for the CPU on tools/hip_host_shim.h, every buffer an exact-size
// heap block.  tools/edit_host_check.py builds this file with -fsanitize=address,undefined or -fsanitize=thread, feeds it the cases and
// compares with numpy, bit for bit.
//   edit_host_check splice IN OUT     IN : int64 {n_src, n_rows, B, ld_out}; desc n_rows x 4 int64; src n_src int16
//                                     OUT: out B x ld_out int16                  (the device's grid: the kernel has no grid-stride loop)
//   edit_host_check restore IN OUT    IN : int64 {B, N, n_mel, cd, ld_keep, grid}; x B N n_mel f32; cat B N cd f32; keep B x ld_keep u8;
//                                          seq_len B int32
//                                     OUT: x                                     (grid = workgroups launched, fewer than the device's)
#include "hip_host_shim.h"
#define VV_EDIT_HOST_CHECK
#include "../vietvoice-tts_amd/csrc/vv_edit.hip"

using vv_host::exact_block;
using vv_host::exact_free;
using vv_host::launch;

template <typename T> static bool rd(FILE* f, T* p, long long n) { return n <= 0 || fread(p, sizeof(T), (size_t)n, f) == (size_t)n; }

int main(int argc, char** argv) {
    if (argc < 4) return 2;
    FILE* f = fopen(argv[2], "rb");
    if (!f) return 2;
    if (!strcmp(argv[1], "splice")) {
        long long h[4];
        if (!rd(f, h, 4)) return 2;
        const long long n_src = h[0], n_rows = h[1], B = h[2], ld_out = h[3];
        if (B < 1 || ld_out < 4 || ld_out % 4) return 2;
        long long* desc = exact_block<long long>(4 * n_rows);
        int16_t* src = exact_block<int16_t>(n_src);
        int16_t* out = exact_block<int16_t>(B * ld_out);
        if (!rd(f, desc, 4 * n_rows) || !rd(f, src, n_src)) return 2;
        fclose(f);
        memset(out, 0xAA, (size_t)(2 * B * ld_out));
        launch(dim3((unsigned)((ld_out / 4 + 255) / 256), (unsigned)B), 256, 0,
               [&]() { edit_splice_kernel(src, n_src, desc, (int)n_rows, out, (int)ld_out); });
        f = fopen(argv[3], "wb");
        if (!f) return 2;
        fwrite(out, 2, (size_t)(B * ld_out), f);
        fclose(f);
        exact_free(desc); exact_free(src); exact_free(out);
        return 0;
    }
    if (!strcmp(argv[1], "restore")) {
        long long h[6];
        if (!rd(f, h, 6)) return 2;
        const long long B = h[0], N = h[1], n_mel = h[2], cd = h[3], ld_keep = h[4], grid = h[5];
        if (B < 1 || N < 1 || ld_keep < N || n_mel % 4 || cd % 4 || cd < n_mel || grid < 1) return 2;
        float* x = exact_block<float>(B * N * n_mel);
        float* cat = exact_block<float>(B * N * cd);
        uint8_t* keep = exact_block<uint8_t>(B * ld_keep);
        int* seq_len = exact_block<int>(B);
        if (!rd(f, x, B * N * n_mel) || !rd(f, cat, B * N * cd) || !rd(f, keep, B * ld_keep) || !rd(f, seq_len, B)) return 2;
        fclose(f);
        launch(dim3((unsigned)grid), 256, 0, [&]() { edit_restore_kernel(x, cat, keep, (int)ld_keep, seq_len, (int)B, (int)N, (int)n_mel, (int)cd); });
        f = fopen(argv[3], "wb");
        if (!f) return 2;
        fwrite(x, 4, (size_t)(B * N * n_mel), f);
        fclose(f);
        exact_free(x); exact_free(cat); exact_free(keep); exact_free(seq_len);
        return 0;
    }
    return 2;
}
