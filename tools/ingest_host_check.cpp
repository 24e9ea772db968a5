// Host check of csrc/vv_ingest.hip (N3 / a8): the ingest, normalize and polyphase kernels compiled for the CPU on tools/hip_host_shim.h,
// every buffer an exact-size heap block; the normalize scratch is ONE block of exactly vvk_normalize_scratch_bytes, laid out as the
// launcher lays it out.  tools/ingest_host_check.py builds this file with -fsanitize=address,undefined or -fsanitize=thread, feeds it
// the cases and compares with the host mirrors.  Every block is filled with 0xAA before it is read into.
//   ingest_host_check ingest IN OUT     IN : int64 {n_bytes, n_clips, total_out, bx}; desc n_clips x 8 int64; pcm n_bytes
//                                       OUT: out total_out f32
//   ingest_host_check normalize IN OUT  IN : int64 {n_clips, total, max_len, chunk_bx, bx}; off (n_clips + 1) int64; x total f32
//                                       OUT: out total int16
//   ingest_host_check resample IN OUT   IN : int64 {n_in, n_taps, up, down, skip, n_out}; taps f64; x f32        OUT: y n_out f32
// bx / chunk_bx = workgroups along x: fewer than the device launches, so that the grid-stride loops take further trips.
#include "hip_host_shim.h"
#define VV_INGEST_HOST_CHECK
#include "../vietvoice-tts_amd/csrc/vv_ingest.hip"

using vv_host::exact_block;
using vv_host::exact_free;
using vv_host::launch;

template <typename T> static T* filled(long long n) {
    T* p = exact_block<T>(n);
    if (n > 0) memset(p, 0xAA, sizeof(T) * (size_t)n);
    return p;
}
template <typename T> static bool rd(FILE* f, T* p, long long n) { return n <= 0 || fread(p, sizeof(T), (size_t)n, f) == (size_t)n; }
template <typename T> static int wr(const char* path, const T* p, long long n) {
    FILE* f = fopen(path, "wb");
    if (!f) return 2;
    if (n > 0) fwrite(p, sizeof(T), (size_t)n, f);
    fclose(f);
    return 0;
}

static int ingest(FILE* f, const char* path) {
    long long h[4];
    if (!rd(f, h, 4)) return 2;
    const long long n_bytes = h[0], n_clips = h[1], total_out = h[2], bx = h[3];
    if (n_clips < 1 || n_clips > 65535 || bx < 1) return 2;
    long long* desc = filled<long long>(8 * n_clips);
    unsigned char* pcm = filled<unsigned char>(n_bytes);
    float* out = filled<float>(total_out);
    if (!rd(f, desc, 8 * n_clips) || !rd(f, pcm, n_bytes)) return 2;
    fclose(f);
    launch(dim3((unsigned)bx, (unsigned)n_clips), 256, 0, [&]() { ingest_pcm_kernel(pcm, desc, out); });
    const int rc = wr(path, out, total_out);
    exact_free(desc); exact_free(pcm); exact_free(out);
    return rc;
}

static int normalize(FILE* f, const char* path) {
    long long h[5];
    if (!rd(f, h, 5)) return 2;
    const long long n_clips = h[0], total = h[1], max_len = h[2], chunk_bx = h[3], bx = h[4];
    if (n_clips < 1 || n_clips > 65535 || max_len < 1 || chunk_bx < 1 || bx < 1) return 2;
    long long* off = filled<long long>(n_clips + 1);
    float* x = filled<float>(total);
    int16_t* out = filled<int16_t>(total);
    unsigned char* scratch = filled<unsigned char>((long long)vvk_normalize_scratch_bytes((int)n_clips, total));
    if (!rd(f, off, n_clips + 1) || !rd(f, x, total)) return 2;
    fclose(f);
    double* stats = (double*)scratch;                                            // the launcher's layout
    float* chunk_sum = (float*)(stats + 2 * (size_t)n_clips);
    launch(dim3((unsigned)chunk_bx, (unsigned)n_clips), 256, 0, [&]() { clip_chunk_sum_kernel(x, off, chunk_sum); });
    launch(dim3((unsigned)((n_clips + 63) / 64)), 64, 0, [&]() { clip_mean_kernel(off, chunk_sum, stats, (int)n_clips); });
    launch(dim3((unsigned)bx, (unsigned)n_clips), 256, 0, [&]() { clip_peak_kernel(x, off, stats); });
    launch(dim3((unsigned)bx, (unsigned)n_clips), 256, 0, [&]() { clip_scale_kernel(x, off, stats, out); });
    const int rc = wr(path, out, total);
    exact_free(off); exact_free(x); exact_free(out); exact_free(scratch);
    return rc;
}

static int resample(FILE* f, const char* path) {
    long long h[6];
    if (!rd(f, h, 6)) return 2;
    const long long n_in = h[0], n_taps = h[1], up = h[2], down = h[3], skip = h[4], n_out = h[5];
    if (n_in < 1 || n_taps < 1 || up < 1 || down < 1 || skip < 0 || n_out < 1) return 2;
    double* taps = filled<double>(n_taps);
    float* x = filled<float>(n_in);
    float* y = filled<float>(n_out);
    if (!rd(f, taps, n_taps) || !rd(f, x, n_in)) return 2;
    fclose(f);
    launch(dim3((unsigned)((n_out + 255) / 256)), 256, 0,
           [&]() { resample_poly_kernel(x, (int)n_in, taps, (int)n_taps, (int)up, (int)down, (int)skip, y, (int)n_out); });
    const int rc = wr(path, y, n_out);
    exact_free(taps); exact_free(x); exact_free(y);
    return rc;
}

int main(int argc, char** argv) {
    if (argc < 4) return 2;
    FILE* f = fopen(argv[2], "rb");
    if (!f) return 2;
    if (!strcmp(argv[1], "ingest")) return ingest(f, argv[3]);
    if (!strcmp(argv[1], "normalize")) return normalize(f, argv[3]);
    if (!strcmp(argv[1], "resample")) return resample(f, argv[3]);
    return 2;
}
