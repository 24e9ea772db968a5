// What tools/{elementwise,mel,noise}_host_check.cpp share: one input file holds a list of launches, each a kernel's name, a grid and the
// kernel's arguments in order; every pointer argument is an exact-size heap block (tools/hip_host_shim.h) filled from the file, so an
// output arrives with its 0xAA fill and what no thread owns must still hold it afterwards.  tools/host_check_common.py (Batch) writes
// the file and reads the result: every block of every launch, in order, as it is after the launch.
//   file   : int64 n_launches, then per launch
//            int64 name_len, name; int64 {gx, gy, gz, block, shmem_bytes, n_args}; per argument int64 tag and
//              tag 0: int64 value            tag 1: double value           tag 2: int64 k: the block of argument k once more (an alias)
//              tag 3: int64 {bytes, byte_off} and the bytes; bytes < 0: a null pointer
//   result : per launch, per tag-3 argument that is not null: its bytes
#pragma once
#include <string>

namespace vv_driver {

struct Arg { long long tag = 0, i = 0, bytes = -1, off = 0; double f = 0.0; unsigned char* p = nullptr; };

struct Launch {
    std::string name;
    dim3 grid;
    unsigned block = 0;
    size_t shmem = 0;
    std::vector<Arg> a;
    long long i(int k) const { return a[(size_t)k].i; }
    double f(int k) const { return a[(size_t)k].f; }
    template <typename T> T* p(int k) const { const Arg& x = a[(size_t)k]; return (T*)(x.tag == 2 ? a[(size_t)x.i].p : x.p); }
};

template <typename T> static bool rd(FILE* f, T* p, long long n) { return n <= 0 || fread(p, sizeof(T), (size_t)n, f) == (size_t)n; }

static bool read_launch(FILE* f, Launch& L) {
    long long n = 0, h[6];
    if (!rd(f, &n, 1) || n < 1 || n > 200) return false;
    L.name.resize((size_t)n);
    if (!rd(f, &L.name[0], n) || !rd(f, h, 6)) return false;
    L.grid = dim3((unsigned)h[0], (unsigned)h[1], (unsigned)h[2]);
    L.block = (unsigned)h[3];
    L.shmem = (size_t)h[4];
    L.a.resize((size_t)h[5]);
    for (Arg& x : L.a) {
        if (!rd(f, &x.tag, 1)) return false;
        if (x.tag == 0 || x.tag == 2) { if (!rd(f, &x.i, 1)) return false; }
        else if (x.tag == 1) { if (!rd(f, &x.f, 1)) return false; }
        else if (x.tag == 3) {
            long long b[2];
            if (!rd(f, b, 2)) return false;
            x.bytes = b[0]; x.off = b[1];
            if (x.bytes >= 0) {
                x.p = vv_host::exact_block<unsigned char>(x.bytes, (int)x.off);
                if (!rd(f, x.p, x.bytes)) return false;
            }
        } else return false;
    }
    return true;
}

// run(L) launches the kernel L.name and returns false when it knows no such kernel
template <typename F> static int main_of(int argc, char** argv, F run) {
    if (argc < 3) return 2;
    FILE* f = fopen(argv[1], "rb");
    FILE* o = fopen(argv[2], "wb");
    long long n = 0;
    if (!f || !o || !rd(f, &n, 1)) return 2;
    for (long long k = 0; k < n; ++k) {
        Launch L;
        if (!read_launch(f, L)) { fprintf(stderr, "launch %lld: bad input\n", k); return 2; }
        if (!run(L)) { fprintf(stderr, "launch %lld: no kernel %s\n", k, L.name.c_str()); return 2; }
        for (Arg& x : L.a)
            if (x.tag == 3 && x.bytes >= 0) {
                fwrite(x.p, 1, (size_t)x.bytes, o);
                vv_host::exact_free(x.p, (int)x.off);
            }
    }
    fclose(f);
    fclose(o);
    return 0;
}

}  // namespace vv_driver

#define VV_I(k) ((int)L.i(k))
#define VV_F(k) ((float)L.f(k))
#define VV_D(k) (L.f(k))
#define VV_P(T, k) (L.p<T>(k))
#define VV_GO(call) (vv_host::launch(L.grid, L.block, L.shmem, [&]() { call; }), true)
