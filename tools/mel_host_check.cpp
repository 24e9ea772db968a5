// Host check of csrc/vv_mel.hip (K1): mel_kernel compiled for the CPU on tools/hip_host_shim.h, every buffer an exact-size heap block, the
// dynamic LDS an exact block of the launcher's (3 n_fft + n_fft / 2 + 1) floats.  tools/mel_host_check.py builds this file with
// -fsanitize=address,undefined or -fsanitize=thread, writes the launches (tools/host_check_driver.h) and compares with the float64
// reference of tests/gpu_util.py.
//   mel_host_check IN OUT     launches "mel": audio, ld_audio, audio_len, window, tw_cos, tw_sin, fb, mel, F_max, n_fft, hop, n_mel
#include "hip_host_shim.h"
#include "host_check_driver.h"
#define VV_MEL_HOST_CHECK
#include "../vietvoice-tts_amd/csrc/vv_mel.hip"

int main(int argc, char** argv) {
    return vv_driver::main_of(argc, argv, [](const vv_driver::Launch& L) {
        if (L.name == "mel")
            return VV_GO(mel_kernel(VV_P(const int16_t, 0), VV_I(1), VV_P(const int, 2), VV_P(const float, 3), VV_P(const float, 4), VV_P(const float, 5),
                                    VV_P(const float, 6), VV_P(float, 7), VV_I(8), VV_I(9), VV_I(10), VV_I(11)));
        return false;
    });
}
