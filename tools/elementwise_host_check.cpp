// Host check of csrc/vv_elementwise.hip: its kernels compiled for the CPU on tools/hip_host_shim.h (wave-scoped shuffles: ln_mod_kernel's
// waves return one by one, grn_apply_kernel and groupnorm_kernel cross the waves through LDS, apg_coef_kernel shuffles doubles), every
// buffer an exact-size heap block.  tools/elementwise_host_check.py builds this file with -fsanitize=address,undefined or
// -fsanitize=thread, writes the launches (tools/host_check_driver.h) and compares with the mirrors of the device tests.
//   elementwise_host_check IN OUT     a launch names a kernel as below; its arguments are the kernel's, in the kernel's order, with
//                                     a GuideFlags as a block of 32 words, OdeStagePrev as k[0..2] then c[0..2], and OdeStageReuse as
//                                     d_buf, load, store behind the last argument
#include "hip_host_shim.h"
#include "host_check_driver.h"
#include "../include/vvtts.h"                 // VV_APG_TILE
#define VVK_GUIDE_MAX_ITEMS 1024              // csrc/vv_kernels.h (which includes the HIP runtime)
#define VV_ELEMENTWISE_HOST_CHECK
#include "../vietvoice-tts_amd/csrc/vv_common.h"
#include "../vietvoice-tts_amd/csrc/vv_elementwise.hip"

using vv_driver::Launch;

static GuideFlags flags_of(const Launch& L, int k) {
    GuideFlags f{};
    if (L.p<unsigned>(k)) memcpy(f.w, L.p<unsigned>(k), sizeof(f.w));
    return f;
}

template <typename To, typename Td> static bool ln(const Launch& L) {
    return VV_GO((ln_mod_kernel<To, Td>(VV_P(float, 0), VV_I(1), VV_P(To, 2), VV_I(3), VV_I(4), VV_I(5), VV_P(const float, 6), VV_P(const float, 7), VV_I(8),
                                        VV_F(9), VV_P(const Td, 10), VV_I(11), VV_P(const Td, 12), VV_I(13), VV_I(14), VV_I(15), VV_P(const float, 16), VV_I(17),
                                        VV_P(const float, 18))));
}

template <typename T> static bool pack(const Launch& L) {
    return VV_GO(pack_cat_kernel<T>(VV_P(const float, 0), VV_P(const float, 1), VV_P(const float, 2), VV_P(T, 3), VV_I(4), VV_I(5), VV_I(6), VV_I(7), VV_I(8),
                                    VV_P(const int, 9)));
}

template <typename T> static bool pack_guided(const Launch& L) {
    return VV_GO(pack_cat_guided_kernel<T>(VV_P(const float, 0), VV_P(const float, 1), VV_P(const float, 2), VV_P(T, 3), VV_I(4), VV_I(5), VV_I(6), VV_I(7), VV_I(8),
                                           VV_I(9), VV_I(10), VV_I(11), VV_P(const int, 12), VV_P(const int, 13), VV_P(const int, 14)));
}

template <bool G, bool A, bool R, bool Nm = false> static bool stage(const Launch& L) {
    OdeStagePrev pv{};
    for (int j = 0; j < 3; ++j) { pv.k[j] = VV_P(const float, 9 + j); pv.c[j] = VV_F(12 + j); }
    std::conditional_t<R, OdeStageReuse, OdeStageNoReuse> ru{};
    if constexpr (R) { ru.d_buf = VV_P(float, 23); ru.load = flags_of(L, 24); ru.store = flags_of(L, 25); }
    return VV_GO((ode_stage_kernel<G, A, R, Nm>(VV_P(float, 0), VV_P(const float, 1), VV_I(2), VV_I(3), VV_I(4), VV_F(5), VV_P(const float, 6), VV_I(7),
                                            VV_P(const int, 8), pv, VV_F(15), VV_P(float, 16), VV_P(float, 17), VV_P(const int, 18), VV_P(const float, 19),
                                            VV_P(const float, 20), VV_I(21), VV_F(22), ru)));
}

template <typename Td, int M> static bool span(const Launch& L) {
    return VV_GO((block_span_kernel<Td, M>(VV_P(float, 0), VV_P(const Td, 1), VV_P(const Td, 2), VV_P(float, 3), (size_t)L.i(4))));
}

template <typename Td> static bool span_of(const Launch& L, const std::string& m) {
    if (m == "mark") return span<Td, VV_SPAN_MARK>(L);
    if (m == "diff") return span<Td, VV_SPAN_DIFF>(L);
    if (m == "apply") return span<Td, VV_SPAN_APPLY>(L);
    return false;
}

template <typename T> static bool grn_stats(const Launch& L) {
    return VV_GO(grn_stats_kernel<T>(VV_P(const T, 0), VV_P(float, 1), VV_P(const int, 2), VV_I(3), VV_I(4), VV_I(5)));
}

template <typename T> static bool grn_apply(const Launch& L) {
    return VV_GO(grn_apply_kernel<T>(VV_P(T, 0), VV_P(const float, 1), VV_P(const float, 2), VV_P(const float, 3), VV_I(4), VV_I(5), VV_I(6)));
}

template <bool M> static bool build_cat(const Launch& L) {
    return VV_GO(build_cat_kernel<M>(VV_P(const float, 0), VV_I(1), VV_P(const int, 2), VV_P(const float, 3), VV_P(float, 4), VV_P(float, 5), VV_I(6), VV_I(7),
                                     VV_I(8), VV_I(9), VV_P(const uint8_t, 10), VV_I(11)));
}

static bool run(const Launch& L) {
    const std::string& n = L.name;
    if (n == "ln_mod<f32,f32>") return ln<float, float>(L);
    if (n == "ln_mod<f32,bf16>") return ln<float, bf16>(L);
    if (n == "ln_mod<bf16,f32>") return ln<bf16, float>(L);
    if (n == "ln_mod<bf16,bf16>") return ln<bf16, bf16>(L);
    if (n == "pack_cat<f32>") return pack<float>(L);
    if (n == "pack_cat<bf16>") return pack<bf16>(L);
    if (n == "pack_cat_guided<f32>") return pack_guided<float>(L);
    if (n == "pack_cat_guided<bf16>") return pack_guided<bf16>(L);
    if (n == "cfg_euler")
        return VV_GO(cfg_euler_kernel(VV_P(float, 0), VV_P(const float, 1), VV_I(2), VV_I(3), VV_I(4), VV_F(5), VV_F(6), VV_P(const int, 7)));
    if (n == "ode_stage<plain>") return stage<false, false, false>(L);
    if (n == "ode_stage<guided>") return stage<true, false, false>(L);
    if (n == "ode_stage<apg>") return stage<false, true, false>(L);
    if (n == "ode_stage<apg_guided>") return stage<true, true, false>(L);
    if (n == "ode_stage<reuse>") return stage<true, false, true>(L);
    if (n == "ode_stage<norm>") return stage<true, false, false, true>(L);
    if (n == "cfg_gram_reduce")
        return VV_GO(cfg_gram_reduce_kernel(VV_P(const float, 0), VV_I(1), VV_I(2), VV_I(3), VV_P(const int, 4), VV_P(const int, 5), VV_P(const int, 6), VV_I(7),
                                            VV_P(double, 8)));
    if (n == "cfg_norm_coef")
        return VV_GO(cfg_norm_coef_kernel(VV_P(const double, 0), VV_I(1), VV_I(2), VV_I(3), VV_P(const int, 4), VV_P(const int, 5), VV_P(const int, 6), VV_F(7),
                                          VV_P(const float, 8), VV_P(const float, 9), VV_P(const float, 10), VV_P(float, 11), VV_P(float, 12)));
    if (n == "apg_reduce")
        return VV_GO(apg_reduce_kernel(VV_P(const float, 0), VV_I(1), VV_I(2), VV_I(3), VV_P(const int, 4), VV_P(const float, 5), VV_P(const int, 6),
                                       VV_P(const int, 7), VV_P(const int, 8), VV_I(9), VV_D(10), VV_P(double, 11)));
    if (n == "apg_coef")
        return VV_GO(apg_coef_kernel(VV_P(const double, 0), VV_I(1), VV_I(2), VV_I(3), VV_P(const int, 4), VV_P(const int, 5), VV_P(const int, 6), VV_D(7), VV_F(8),
                                     VV_P(const float, 9), VV_P(const float, 10), VV_P(const float, 11), VV_P(float, 12)));
    if (n == "ode_diff_reduce")
        return VV_GO(ode_diff_reduce_kernel(VV_P(const float, 0), VV_P(const float, 1), VV_I(2), VV_I(3), VV_P(const int, 4), VV_P(const int, 5), VV_I(6),
                                            VV_P(double, 7)));
    if (n == "ode_diff_finish")
        return VV_GO(ode_diff_finish_kernel(VV_P(const double, 0), VV_I(1), VV_I(2), VV_P(const int, 3), VV_P(const int, 4), VV_P(double, 5)));
    if (n == "cfg_drift_reduce")
        return VV_GO(cfg_drift_reduce_kernel(VV_P(const float, 0), VV_I(1), VV_I(2), VV_I(3), VV_P(const int, 4), VV_P(const float, 5), flags_of(L, 6),
                                             VV_P(const int, 7), VV_P(const int, 8), VV_I(9), VV_P(double, 10)));
    if (n.rfind("block_span<f32,", 0) == 0) return span_of<float>(L, n.substr(15, n.size() - 16));
    if (n.rfind("block_span<bf16,", 0) == 0) return span_of<bf16>(L, n.substr(16, n.size() - 17));
    if (n == "block_drift_reduce")
        return VV_GO(block_drift_reduce_kernel(VV_P(const float, 0), VV_P(const float, 1), VV_I(2), VV_I(3), VV_P(const int, 4), VV_P(const int, 5), VV_I(6),
                                               VV_P(double, 7)));
    if (n == "block_drift_finish")
        return VV_GO(block_drift_finish_kernel(VV_P(const double, 0), VV_I(1), VV_I(2), VV_P(const int, 3), VV_P(const int, 4), VV_I(5), VV_I(6),
                                               VV_P(double, 7)));
    if (n == "text_embed")
        return VV_GO(text_embed_kernel(VV_P(const int, 0), VV_I(1), VV_P(const int, 2), VV_P(const float, 3), VV_P(const float, 4), VV_P(float, 5), VV_I(6), VV_I(7),
                                       VV_I(8), VV_I(9)));
    if (n == "dwconv")
        return VV_GO(dwconv_kernel(VV_P(const float, 0), VV_P(float, 1), VV_P(const float, 2), VV_P(const float, 3), VV_P(const int, 4), VV_I(5), VV_I(6), VV_I(7),
                                   VV_I(8), VV_I(9)));
    if (n == "grn_stats<f32>") return grn_stats<float>(L);
    if (n == "grn_stats<bf16>") return grn_stats<bf16>(L);
    if (n == "grn_apply<f32>") return grn_apply<float>(L);
    if (n == "grn_apply<bf16>") return grn_apply<bf16>(L);
    if (n == "build_cat<plain>") return build_cat<false>(L);
    if (n == "build_cat<masked>") return build_cat<true>(L);
    if (n == "ref_len") return VV_GO(ref_len_kernel(VV_P(const int, 0), VV_P(int, 1), VV_I(2), VV_I(3)));
    if (n == "decode_len")
        return VV_GO(decode_len_kernel(VV_P(const int, 0), VV_P(const int, 1), VV_P(int, 2), VV_I(3), VV_I(4), VV_P(const int, 5), VV_I(6), VV_I(7)));
    if (n == "row_tables")
        return VV_GO(row_tables_kernel(VV_P(const int, 0), VV_I(1), VV_I(2), VV_I(3), VV_P(int, 4), VV_P(int, 5), VV_P(int, 6), VV_P(int, 7)));
    if (n == "guided_tables")
        return VV_GO(guided_tables_kernel(VV_P(const int, 0), flags_of(L, 1), VV_I(2), VV_I(3), VV_I(4), VV_I(5), VV_P(int, 6), VV_P(int, 7), VV_P(int, 8),
                                          VV_P(int, 9), VV_P(int, 10), VV_P(int, 11), VV_P(int, 12)));
    if (n == "groupnorm")
        return VV_GO(groupnorm_kernel(VV_P(const float, 0), VV_P(float, 1), VV_P(const float, 2), VV_P(const float, 3), VV_I(4), VV_I(5), VV_I(6), VV_F(7), VV_I(8)));
    if (n == "rope_compact") return VV_GO(rope_compact_kernel(VV_P(const float, 0), VV_P(const float, 1), VV_P(float, 2), VV_I(3)));
    if (n == "rope_rows") return VV_GO(rope_rows_kernel(VV_P(const float, 0), VV_P(const int, 1), VV_P(float, 2), VV_I(3)));
    return false;
}

int main(int argc, char** argv) { return vv_driver::main_of(argc, argv, run); }
