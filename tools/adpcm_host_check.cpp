// Host check of csrc/vv_adpcm.hip: the encoder, the header check and the two decoders compiled for the CPU on
// tools/hip_host_shim.h, every buffer an exact-size heap block.  tools/adpcm_host_check.py builds this file with
// -fsanitize=address,undefined or -fsanitize=thread, writes the launches (tools/host_check_driver.h) and compares with the mirror of
// core/audio_processor.py.  It has its own main and loads nothing into another process.
//   adpcm_host_check IN OUT     launches "adpcm_encode": x, n_x, rows, spb, y, n_y          (grid (blocks, R), 128 threads)
//                                        "wav_check":    data, n_data, rows, n_pcm, status  (grid R, 256 threads)
//                                        "adpcm_decode": data, n_data, rows, pcm, n_pcm     (grid (bx, R), 256 threads)
//                                        "g711_decode":  data, n_data, rows, pcm, n_pcm     (grid (bx, R), 256 threads)
#include "hip_host_shim.h"
#include "host_check_driver.h"
#define VV_ADPCM_HOST_CHECK
#include "../vietvoice-tts_amd/csrc/vv_adpcm.hip"

int main(int argc, char** argv) {
    return vv_driver::main_of(argc, argv, [](const vv_driver::Launch& L) {
        typedef long long i64;
        if (L.name == "adpcm_encode")
            return VV_GO(adpcm_encode_kernel(VV_P(const int16_t, 0), L.i(1), VV_P(const i64, 2), VV_I(3), VV_P(uint8_t, 4), L.i(5)));
        if (L.name == "wav_check")
            return VV_GO(wav_check_kernel(VV_P(const uint8_t, 0), L.i(1), VV_P(const i64, 2), L.i(3), VV_P(i64, 4)));
        if (L.name == "adpcm_decode")
            return VV_GO(adpcm_decode_kernel(VV_P(const uint8_t, 0), L.i(1), VV_P(const i64, 2), VV_P(uint8_t, 3), L.i(4)));
        if (L.name == "g711_decode")
            return VV_GO(g711_decode_kernel(VV_P(const uint8_t, 0), L.i(1), VV_P(const i64, 2), VV_P(uint8_t, 3), L.i(4)));
        return false;
    });
}
