// Host check of csrc/vv_noise.hip: noise_fill_kernel<0> and <1> compiled for the CPU on tools/hip_host_shim.h, every
// buffer an exact-size heap block.  tools/noise_host_check.py builds this file with -fsanitize=address,undefined or -fsanitize=thread,
// writes the launches (tools/host_check_driver.h) and compares with tests/philox_reference.py.
//   noise_host_check IN OUT     launches "noise_fill<0>" (normal; cospif / sinpif are the shim's stand-ins) and "noise_fill<1>" (uniform):
//                               x, seq_len, keys, N, n_mel, per_item, total
#include "hip_host_shim.h"
#include "host_check_driver.h"
#define VV_NOISE_HOST_CHECK
#include "../vietvoice-tts_amd/csrc/vv_noise.hip"

int main(int argc, char** argv) {
    return vv_driver::main_of(argc, argv, [](const vv_driver::Launch& L) {
        typedef unsigned long long u64;
        if (L.name == "noise_fill<0>")
            return VV_GO(noise_fill_kernel<0>(VV_P(float, 0), VV_P(const int, 1), VV_P(const u64, 2), VV_I(3), VV_I(4), (u64)L.i(5), (u64)L.i(6)));
        if (L.name == "noise_fill<1>")
            return VV_GO(noise_fill_kernel<1>(VV_P(float, 0), VV_P(const int, 1), VV_P(const u64, 2), VV_I(3), VV_I(4), (u64)L.i(5), (u64)L.i(6)));
        return false;
    });
}
