// C ABI + native stage drivers: context, named weight binding, workspace arena, the preprocess /
// transformer-steps / decode launch sequences, and HIP-event profiling per kernel class.
// No torch types, no exceptions across the ABI, no device allocation inside the step loop.
#include <hip/hip_runtime.h>
#include <algorithm>
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstring>
#include <map>
#include <string>
#include <utility>
#include <vector>
#include "vv_kernels.h"

#define VV_VERSION_STR "vvtts-hip 0.15 (gfx950)"

namespace {
std::string g_create_error;

struct Bound { const void* p; uint64_t bytes; };

struct ProfRec { hipEvent_t a, b; int cls, sub; };

inline size_t align_up(size_t v, size_t a) { return (v + a - 1) / a * a; }
inline int pad_to(int v, int a) { return (v + a - 1) / a * a; }
}  // namespace

struct vv_ctx {
    int device = 0;
    vv_model_cfg cfg{};
    int dt = VV_DTYPE_BF16;             // acoustic operand dtype
    std::string err;
    std::map<std::string, Bound> w;
    bool finalized = false;
    bool ever_finalized = false;        // vv_set_vocos is refused once the weights have been finalized
    bool vocos = false;                 // N6: the Vocos decoder instead of the HiFi-GAN generator (vv_set_vocos)
    vv_vocos_cfg vcfg{};
    float post_bias = 0.f;
    // time grid tables
    int n_steps = 0;                    // ODE steps of the plan in force
    std::vector<float> dt_host;
    float* modtab = nullptr;            // [depth][n_steps * ode_s][6D]: one row per evaluation (step n, stage i at n * ode_s + i)
    float* fintab = nullptr;            // [n_steps * ode_s][2D]
    // N7: explicit Runge-Kutta tableau of the plan (vv_set_ode_plan; vv_set_time_grid = Euler, ode_s 1)
    int ode_s = 1;
    double ode_a[16] = {}, ode_b[4] = {1.0, 0, 0, 0};
    int ode_kslot[4] = {-1, -1, -1, -1};   // slope buffer of k_j, -1 = k_j is consumed by the launch that makes it and never read again
    int ode_nk = 0;                     // slope buffers a step needs (<= ode_s - 1)
    // N20: Adams-Bashforth multistep plan (vv_set_ode_multistep) on the one-stage tables; ms_q 0 = none.  Any other plan clears it.
    int ms_q = 0;                       // slopes a step combines: the fresh one and ms_q - 1 kept from the steps before
    std::vector<double> ms_beta;        // [n_steps][ms_q], j = 0 the newest slope
    double* ode_report = nullptr;       // N20 step report (vv_set_ode_report): caller-owned device [report_steps][report_B][2], nullptr = off
    int report_steps = 0, report_B = 0;
    // workspace block
    char* ws = nullptr;                 // context-owned block: may MOVE when a later call needs more bytes (ensure_ws)
    size_t ws_cap = 0;
    uint64_t ws_generation = 0;         // bumped whenever ws is reallocated
    int* d_mult = nullptr;              // decode length multipliers
    int rope_rows = 0;                  // 1: the QKV rope epilogue reads row-gathered tables (vv_rope_rows).  Off by default: 11 % faster in a
                                        // back-to-back GEMM loop (tables stay cached), 0.9 % SLOWER inside the step, where the 52 MB of row
                                        // tables come from HBM each time while the 0.8 MB position tables stay in L2 (profiles/r02/gemm_notes.md)
    int split_k_tail = 0;               // bf16 gate-store GEMMs: split the K range of the last row panels when the tile count leaves a partial
                                        // last round of the persistent kernel (vv_gemm_tail_plan); the LayerNorm sums the fp32 parts and rounds
                                        // once.  0 off (default), 1 out-projection and FF2, 2 FF2 only.  OFF since round 4: a tail row's fp32
                                        // summation order differs from a plain row's, the next bf16 rounding turns that into bf16-level noise
                                        // (22 LSB of PCM between two batchings of one text, tests/test_longform_gpu.py), and with the parts in
                                        // fp32 the tail no longer pays either (GEMM -3.6 ms, norms +7.1 ms per headline step,
                                        // profiles/r04/tail_fp32_notes.md).  Off, every row's arithmetic is independent of its batch neighbours.
    int chip_share = 1;                 // 2 while a call runs two lanes (vv_gemm_args.chip_share of its GEMM launches)
    int ring_tiles_max = 256;           // the tile-count bound of that rule (the CU count)
    int ring_tiles = 1;                 // 1 (default since round 5; same bits): N <= 1024 bf16 GEMMs whose 64 x 128 tiles are fewer than the CUs take the 64 x 64 three-stage-ring tiling (vv_gemm tile 6464)
    int pp_min_tiles = -1;              // bf16 GEMMs of the path: -1 = the launcher's own choice between the persistent 256 x 256 kernel and the 128 x 128 one
                                        // (vv_gemm.hip launch(): about one full round of 256-tiles, or the wide QKV shape); n >= 0 = the persistent
                                        // kernel whenever M >= 4096, N % 256 == 0 and the shape has >= n 256-tiles (0 = the rule of rounds 1-3; lets a
                                        // small model exercise the persistent kernel in the whole pipeline, tests/test_e2e_gpu.py).  Same bits either way.
    int lanes = 0;                      // transformer steps as two half batches on two streams: 0 auto (bf16, >= VV_LANE_MIN_ROWS packed rows), 1 never,
                                        // 2 whenever B >= 2
    hipStream_t side_stream[1] = {};    // lane 1's stream (created on first use), forked from / joined to the caller's stream inside the call
    hipEvent_t ev_fork = nullptr, ev_join[1] = {};
    float rope_theta = 0.f;             // > 0 (vv_set_rope_theta): the caller's rope tables are the standard ones of this base; the bf16 QKV epilogue then
                                        // computes cos / sin from the position (no table load), q leaves the GEMM without the softmax scale and the
                                        // attention kernel applies it (q_scale).  Overrides rope_q_attn.
    int rope_q_attn = 1;                // bf16: 1 = the QKV GEMM ropes the k columns only and the attention kernel ropes Q while loading it
    int voc_x3 = -1;                    // vocoder conv products: 0 = v_mfma_f32_32x32x2_f32, 1 = exact 3-way bf16 split on the bf16 matrix pipe
                                        // (vv_vocoder_x3.hip: six piece products, fp32 accumulate, fp32 fidelity); -1 = by acoustic dtype (bf16
                                        // context: 1, fp32 context: 0 -- the numerics configuration stays on the f32 instruction)
    int voc_x3_rows = 0;                // x3 workgroup rows for stages with > 64 rows: 0 = default (64, 4 waves), 128 = 8-wave workgroups
    char* x3_buf = nullptr;             // split weight slabs of every vocoder conv (built by vv_finalize_weights)
    std::map<std::string, const void*> x3_w;
    int fuse_mrf = 2;                   // K12 fused MRF pairs (C <= 64 stages): 0 never, 1 always, 2 auto = for decodes of <= 8 items
                                        // (fewer launches win when the stage is launch-bound; at B = 32 the halo recompute costs 1.3 %)
    // profiling
    bool prof = false;
    std::vector<ProfRec> recs;
    std::vector<hipEvent_t> pool;
    int64_t p_launch[VV_PROF_NCLASS]{};
    double p_flops[VV_PROF_NCLASS]{}, p_bytes[VV_PROF_NCLASS]{}, p_ms[VV_PROF_NCLASS]{};

    int fail(int code, const char* fmt, ...) {
        char buf[1024];
        va_list ap;
        va_start(ap, fmt);
        vsnprintf(buf, sizeof buf, fmt, ap);
        va_end(ap);
        err = buf;
        return code;
    }
    const void* W(const std::string& n) const {
        auto it = w.find(n);
        return it == w.end() ? nullptr : it->second.p;
    }
    const float* Wf(const std::string& n) const { return (const float*)W(n); }
    int esz() const { return dt == VV_DTYPE_BF16 ? 2 : 4; }
    int bk() const { return dt == VV_DTYPE_BF16 ? 64 : 32; }
};

namespace {

#define HIPCHK(ctx, call)                                                                   \
    do {                                                                                    \
        hipError_t e__ = (call);                                                            \
        if (e__ != hipSuccess) return (ctx)->fail(-5, "%s: %s", #call, hipGetErrorString(e__)); \
    } while (0)

#define KCHK(ctx, call)                                              \
    do {                                                             \
        const char* m__ = "";                                        \
        int r__ = (call);                                            \
        if (r__ != 0) return (ctx)->fail(r__, "%s", m__);            \
    } while (0)

struct Prof {
    vv_ctx* c; int idx = -1; hipStream_t st;
    Prof(vv_ctx* c_, int cls, double flops, double bytes, hipStream_t st_, int sub = -1) : c(c_), st(st_) {
        if (!c->prof) return;
        ProfRec r; r.cls = cls; r.sub = sub;
        if (sub >= 0) { c->p_launch[sub]++; c->p_flops[sub] += flops; c->p_bytes[sub] += bytes; }
        auto get = [&]() { hipEvent_t e; if (!c->pool.empty()) { e = c->pool.back(); c->pool.pop_back(); } else hipEventCreate(&e); return e; };
        r.a = get(); r.b = get();
        hipEventRecord(r.a, st);
        c->recs.push_back(r); idx = (int)c->recs.size() - 1;
        c->p_launch[cls]++; c->p_flops[cls] += flops; c->p_bytes[cls] += bytes;
    }
    ~Prof() { if (idx >= 0) hipEventRecord(c->recs[idx].b, st); }
};

// The workspace of ONE call.  A stage names its buffers in one function that takes them from an arena, and runs it twice (plan_ws):
// on a null-based arena for the byte count, then on the block for the pointers.  A zero-length take still aligns.
struct Arena {
    char* base = nullptr; size_t cap = 0, off = 0;
    template <typename T> T* take(size_t n) { off = align_up(off, 256); T* p = base ? (T*)(base + off) : nullptr; off += n * sizeof(T); return p; }
};
template <typename F> size_t plan_bytes(F&& plan) { Arena dry; plan(dry); return dry.off; }
// The context's own block, grown to `bytes` (it may move: nothing a captured hipGraph points into).
int ensure_ws(vv_ctx* c, size_t bytes, Arena* a) {
    if (bytes > c->ws_cap) {
        if (c->ws) { hipDeviceSynchronize(); hipFree(c->ws); c->ws = nullptr; c->ws_cap = 0; }
        const size_t want = align_up(bytes + bytes / 16, 1 << 20);
        hipError_t e = hipMalloc((void**)&c->ws, want);
        if (e != hipSuccess) return c->fail(-12, "workspace hipMalloc(%zu MiB): %s", want >> 20, hipGetErrorString(e));
        c->ws_cap = want; ++c->ws_generation;
    }
    *a = Arena{c->ws, c->ws_cap, 0};
    return 0;
}
// A caller-owned block as the arena of one call (memory that can never move: what a captured hipGraph must point into).
int use_ws(vv_ctx* c, void* block, size_t have, size_t need, Arena* a) {
    if ((uintptr_t)block % 256) return c->fail(-22, "workspace block must be 256-byte aligned");
    if (have < need) return c->fail(-22, "workspace block too small: %zu < %zu bytes", have, need);
    *a = Arena{(char*)block, have, 0};
    return 0;
}
// plan(Arena&) twice: the bytes, then the pointers into `block` (caller-owned) or, block == nullptr, the context's block.
template <typename F> int plan_ws(vv_ctx* c, void* block, size_t have, F&& plan) {
    const size_t need = plan_bytes(plan);
    Arena a;
    if (int r = block ? use_ws(c, block, have, need, &a) : ensure_ws(c, need, &a)) return r;
    plan(a);
    if (a.off > a.cap) return c->fail(-14, "workspace plan took %zu bytes of a %zu-byte block", a.off, a.cap);
    return 0;
}

// ---- GEMM launches over bound weights -----------------------------------------------------
// gemm_args fills what every launch has; the call site sets everything optional by field name and hands the launch to launch_gemm.
struct Gemm : vv_gemm_args { const char* wname; };
Gemm gemm_args(const vv_ctx* c, int dtype, int out_dtype, int mode, int act, const void* A, int lda, const char* wname, int ldw,
               const char* bname, void* C, int ldc, int M, int N, int K) {
    Gemm g{};
    g.dtype = dtype; g.out_dtype = out_dtype; g.mode = mode; g.act = act;
    g.A = A; g.lda = lda; g.W = c->W(wname); g.ldw = ldw; g.C = C; g.ldc = ldc; g.M = M; g.N = N; g.K = K;
    g.bias = bname ? c->Wf(bname) : nullptr; g.wname = wname;
    if (bname && !g.bias) g.W = nullptr;          // a named bias that is not bound: refused by launch_gemm like an unbound weight
    return g;
}
// The context's tile rules and chip_share where the call site pinned neither, the profiling record under class `cls`, the launch.
// alg_flops >= 0: the flops of the un-padded product, where N or K is padded.
int launch_gemm(vv_ctx* c, Gemm g, int cls, hipStream_t st, double alg_flops = -1) {
    if (!g.W) return c->fail(-2, "weight '%s' is not bound", g.wname);
    const int M = g.M, N = g.N, K = g.K, bf16 = g.dtype == VV_DTYPE_BF16;
    if (!g.chip_share) g.chip_share = c->chip_share;
    if (g.tile == 0 && c->pp_min_tiles >= 0 && bf16 && N % 256 == 0)
        g.tile = (M >= 4096 && (long long)((M + 255) / 256) * (N / 256) >= c->pp_min_tiles) ? 256 : 128;
    if (c->ring_tiles && g.tile == 0 && bf16 && N <= 1024 && N % 64 == 0 && (long long)((M + 63) / 64) * (N / 128) <= c->ring_tiles_max)
        g.tile = 6464;
    const int esz = bf16 ? 2 : 4, osz = g.out_dtype == VV_DTYPE_BF16 ? 2 : 4;
    const double fl = alg_flops >= 0 ? alg_flops : 2.0 * M * (double)N * K;
    Prof p(c, cls, fl, (double)M * K * esz + (double)N * K * esz + (double)M * N * osz * (g.mode == VV_EPI_GATE_RES ? 2 : 1), st);
    const char* m = "";
    if (int r = vvk_gemm(&g, st, &m)) return c->fail(r, "%s (weight %s, M=%d N=%d K=%d)", m, g.wname, M, N, K);
    return 0;
}

std::string blk(int i, const char* s) { return "blocks." + std::to_string(i) + s; }

// ---- the checks the PCM entries (N10 ... N19) share.  Each refusal is -22 with the entry's name in front, before anything is launched.
// the prologue, behind the entry's own ``if (!c) return -22``: the context's device is made current -> the caller's stream
inline hipStream_t enter(vv_ctx* c, void* stream) {
    hipSetDevice(c->device);
    return (hipStream_t)stream;
}

// off + n <= total for non-negative off and n, without forming the sum
inline bool fits(int64_t off, int64_t n, int64_t total) { return off >= 0 && n >= 0 && n <= total && off <= total - n; }

inline bool spans_overlap(const void* a, uint64_t na, const void* b, uint64_t nb) {
    return (uintptr_t)a < (uintptr_t)b + nb && (uintptr_t)b < (uintptr_t)a + na;
}

struct PtrArg { const char* name; const void* p; unsigned align = 1; bool may_be_null = false; };

int check_ptrs(vv_ctx* c, const char* entry, std::initializer_list<PtrArg> args) {
    for (const PtrArg& a : args) {
        if (!a.p && !a.may_be_null) return c->fail(-22, "%s: null pointer (%s)", entry, a.name);
        if ((uintptr_t)a.p % a.align) return c->fail(-22, "%s: misaligned pointer (%s: %u bytes)", entry, a.name, a.align);
    }
    return 0;
}

int check_ws(vv_ctx* c, const char* entry, uint64_t have, uint64_t need, const char* what = "ws") {
    return have < need ? c->fail(-22, "%s: %s of %llu bytes, %llu are needed", entry, what, (unsigned long long)have, (unsigned long long)need) : 0;
}

// the clip rows of vv_flac_index and vv_flac_decode: ascending, 4-byte aligned, 8 bytes of padding behind the last; -> 0 or the refusal
int flac_rows(vv_ctx* c, const char* name, const int64_t* rows, const int64_t* rows_host, int R, int64_t n_bytes, int* max_channels) {
    if (R < 1 || R > 65535 || n_bytes < 8 || n_bytes > ((int64_t)1 << 31) - 64)
        return c->fail(-22, "%s: bad sizes (1 <= R <= 65535, 8 <= n_bytes <= 2^31 - 64)", name);
    if (int e = check_ptrs(c, name, {{"rows", rows, 8}, {"rows_host", rows_host, 8}})) return e;
    int64_t at = 0;
    *max_channels = 1;
    for (int r = 0; r < R; ++r) {
        const int64_t* q = rows_host + 8 * (size_t)r;
        if (q[0] < at || q[0] % 4 || !fits(q[0], q[1], n_bytes - 8))
            return c->fail(-22, "%s: row %d: the clips lie in ascending order, 4-byte aligned, inside data less 8 bytes of padding", name, r);
        if (q[2] < 1 || q[2] > 8 || (q[3] != 8 && q[3] != 16 && q[3] != 24) || q[5] < 16 || q[5] > 65535 || q[4] < 0 || q[4] > q[5] || q[6] < 1 ||
            q[6] > 1048575 || q[7] < 0 || q[7] > VV_FLAC_MAX_CLIP)
            return c->fail(-22, "%s: row %d: channels 1 ... 8, bits 8 / 16 / 24, 16 <= max block <= 65535, min <= max, rate 1 ... 1048575, total <= 2^26", name, r);
        at = q[0] + q[1];
        if (q[2] > *max_channels) *max_channels = (int)q[2];
    }
    return 0;
}

}  // namespace

// =====================================================================================  ABI
extern "C" {

const char* vv_version(void) { return VV_VERSION_STR; }

const char* vv_last_error(const vv_ctx* ctx) { return ctx ? ctx->err.c_str() : g_create_error.c_str(); }

int vv_create(vv_ctx** out, int device, const vv_model_cfg* cfg, int acoustic_dtype) {
    if (!out || !cfg) { g_create_error = "vv_create: null argument"; return -22; }
    *out = nullptr;
    int n = 0;
    hipError_t e = hipGetDeviceCount(&n);
    if (e != hipSuccess || n <= 0) { g_create_error = "vv_create: no HIP device visible (the HIP path has no CPU fallback)"; return -19; }
    if (device < 0 || device >= n) { g_create_error = "vv_create: device index out of range"; return -22; }
    if (acoustic_dtype != VV_DTYPE_F32 && acoustic_dtype != VV_DTYPE_BF16) { g_create_error = "vv_create: dtype must be f32 or bf16"; return -22; }
    if (cfg->head_dim != 64 || cfg->heads * 64 != cfg->dim) { g_create_error = "vv_create: head_dim must be 64"; return -22; }
    if (cfg->dim % 128 || cfg->text_dim % 128 || cfg->dim / cfg->pos_conv_groups != 64 || cfg->n_mel % 4 || cfg->dim > 1024 ||
        cfg->text_dim > 1024) {
        g_create_error = "vv_create: dim/text_dim must be multiples of 128 (<=1024), 64 channels per pos-conv group"; return -22;
    }
    if (cfg->voc_n_up < 1 || cfg->voc_n_up > VV_MAX_UP || cfg->voc_n_res > VV_MAX_RES || cfg->voc_n_dil > VV_MAX_RES) {
        g_create_error = "vv_create: vocoder topology out of range"; return -22;
    }
    e = hipSetDevice(device);
    if (e != hipSuccess) { g_create_error = hipGetErrorString(e); return -5; }
    vv_ctx* c = new vv_ctx();
    c->device = device; c->cfg = *cfg; c->dt = acoustic_dtype;
    *out = c;
    return 0;
}

void vv_destroy(vv_ctx* c) {
    if (!c) return;
    hipSetDevice(c->device);
    hipDeviceSynchronize();
    if (c->ws) hipFree(c->ws);
    if (c->modtab) hipFree(c->modtab);
    if (c->fintab) hipFree(c->fintab);
    if (c->d_mult) hipFree(c->d_mult);
    if (c->x3_buf) hipFree(c->x3_buf);
    for (auto q : c->side_stream) if (q) hipStreamDestroy(q);
    if (c->ev_fork) hipEventDestroy(c->ev_fork);
    for (auto e : c->ev_join) if (e) hipEventDestroy(e);
    for (auto& r : c->recs) { hipEventDestroy(r.a); hipEventDestroy(r.b); }
    for (auto e : c->pool) hipEventDestroy(e);
    delete c;
}

int vv_bind_weight(vv_ctx* c, const char* name, const void* p, uint64_t bytes) {
    if (!c || !name || !p) return c ? c->fail(-22, "vv_bind_weight: null argument") : -22;
    if ((uintptr_t)p % 16) return c->fail(-22, "vv_bind_weight(%s): pointer must be 16-byte aligned", name);
    c->w[name] = Bound{p, bytes};
    c->finalized = false;
    return 0;
}

int vv_finalize_weights(vv_ctx* c) {
    if (!c) return -22;
    const vv_model_cfg& g = c->cfg;
    const int D = g.dim, Dt = g.text_dim, FF = g.dim * g.ff_mult, es = c->esz();
    const int KP = pad_to(2 * g.n_mel + Dt, 64), MP = pad_to(g.n_mel, 128);
    std::string missing;
    auto need = [&](const std::string& n, uint64_t bytes) {
        auto it = c->w.find(n);
        if (it == c->w.end()) { missing += n + " "; return; }
        if (it->second.bytes < bytes) missing += n + "(short:" + std::to_string(it->second.bytes) + "<" + std::to_string(bytes) + ") ";
    };
    need("const.window", 4ull * g.n_fft); need("const.tw_cos", 4ull * g.n_fft); need("const.tw_sin", 4ull * g.n_fft);
    need("const.mel_fb", 4ull * (g.n_fft / 2 + 1) * g.n_mel);
    need("const.text_pos", 4ull * g.max_pos * Dt);
    need("text.embed.weight", 4ull * g.vocab_rows * Dt);
    for (int i = 0; i < g.text_layers; ++i) {
        const std::string p = "text.blocks." + std::to_string(i);
        need(p + ".dwconv.weight", 4ull * Dt * g.text_conv_k); need(p + ".dwconv.bias", 4ull * Dt);
        need(p + ".norm.weight", 4ull * Dt); need(p + ".norm.bias", 4ull * Dt);
        need(p + ".pwconv1.weight", (uint64_t)es * Dt * g.text_ff_mult * Dt); need(p + ".pwconv1.bias", 4ull * Dt * g.text_ff_mult);
        need(p + ".grn.gamma", 4ull * Dt * g.text_ff_mult); need(p + ".grn.beta", 4ull * Dt * g.text_ff_mult);
        need(p + ".pwconv2.weight", (uint64_t)es * Dt * g.text_ff_mult * Dt); need(p + ".pwconv2.bias", 4ull * Dt);
    }
    need("input.proj.weight", (uint64_t)es * D * KP); need("input.proj.bias", 4ull * D);
    for (int j = 1; j <= 2; ++j) {
        need("input.pos_conv" + std::to_string(j) + ".weight", (uint64_t)es * D * 64 * g.pos_conv_k);
        need("input.pos_conv" + std::to_string(j) + ".bias", 4ull * D);
    }
    need("time.mlp1.weight", 4ull * D * g.time_freq_dim); need("time.mlp1.bias", 4ull * D);
    need("time.mlp2.weight", 4ull * D * D); need("time.mlp2.bias", 4ull * D);
    for (int i = 0; i < g.depth; ++i) {
        need(blk(i, ".adaln.weight"), 4ull * 6 * D * D); need(blk(i, ".adaln.bias"), 4ull * 6 * D);
        need(blk(i, ".attn.qkv.weight"), (uint64_t)es * 3 * D * D); need(blk(i, ".attn.qkv.bias"), 4ull * 3 * D);
        need(blk(i, ".attn.out.weight"), (uint64_t)es * D * D); need(blk(i, ".attn.out.bias"), 4ull * D);
        need(blk(i, ".ff1.weight"), (uint64_t)es * FF * D); need(blk(i, ".ff1.bias"), 4ull * FF);
        need(blk(i, ".ff2.weight"), (uint64_t)es * D * FF); need(blk(i, ".ff2.bias"), 4ull * D);
    }
    need("final.adaln.weight", 4ull * 2 * D * D); need("final.adaln.bias", 4ull * 2 * D);
    need("final.proj.weight", (uint64_t)es * MP * D); need("final.proj.bias", 4ull * MP);
    if (c->vocos) {                                        // N6: the Vocos tensors instead of the HiFi-GAN ones (all fp32)
        const vv_vocos_cfg& v = c->vcfg;
        const uint64_t V = v.dim, I = v.intermediate, KE = pad_to(v.embed_k * g.n_mel, 32), HP = pad_to(v.n_fft + 2, 128);
        need("const.istft_basis", 4ull * v.n_fft * v.n_fft);
        need("voc.embed.weight", 4 * V * KE); need("voc.embed.bias", 4 * V);
        for (const char* n : {"voc.norm", "voc.final_norm"}) { need(std::string(n) + ".weight", 4 * V); need(std::string(n) + ".bias", 4 * V); }
        for (int i = 0; i < v.layers; ++i) {
            const std::string p = "voc.blocks." + std::to_string(i);
            need(p + ".dwconv.weight", 4 * V * v.dw_k); need(p + ".dwconv.bias", 4 * V);
            need(p + ".norm.weight", 4 * V); need(p + ".norm.bias", 4 * V);
            need(p + ".pwconv1.weight", 4 * I * V); need(p + ".pwconv1.bias", 4 * I);
            need(p + ".pwconv2.weight", 4 * V * I); need(p + ".pwconv2.bias", 4 * V);
            need(p + ".gamma", 4 * V);
        }
        need("voc.head.weight", 4 * HP * V); need("voc.head.bias", 4 * HP);
        if (!missing.empty()) return c->fail(-2, "missing or short weights: %s", missing.c_str());
        c->finalized = c->ever_finalized = true;
        return 0;
    }
    int ch = g.voc_pre_ch;
    struct ConvW { std::string name; int cin_pad, kw, rows_pad; };
    std::vector<ConvW> convs;                              // every vocoder conv slab [cin_pad][kw][rows_pad]: split for the x3 kernels below
    convs.push_back({"voc.pre.weight", pad_to(g.n_mel, 8), g.voc_pre_k, pad_to(ch, 64)});
    need("voc.pre.weight", 4ull * pad_to(g.n_mel, 8) * g.voc_pre_k * pad_to(ch, 64)); need("voc.pre.bias", 4ull * ch);
    for (int s = 0; s < g.voc_n_up; ++s) {
        const int cin = ch, cout = ch / 2, u = g.voc_up_rates[s];
        const std::string p = "voc.up." + std::to_string(s);
        need(p + ".weight", 4ull * pad_to(cin, 8) * 2 * pad_to(cout * u, 64)); need(p + ".bias", 4ull * cout);
        convs.push_back({p + ".weight", pad_to(cin, 8), 2, pad_to(cout * u, 64)});
        for (int a = 0; a < g.voc_n_res; ++a)
            for (int b = 0; b < g.voc_n_dil; ++b)
                for (int k = 1; k <= 2; ++k) {
                    const std::string q = "voc.res." + std::to_string(s) + "." + std::to_string(a) + "." + std::to_string(b) + ".conv" + std::to_string(k);
                    need(q + ".weight", 4ull * pad_to(cout, 8) * g.voc_res_kernels[a] * pad_to(cout, 64)); need(q + ".bias", 4ull * cout);
                    convs.push_back({q + ".weight", pad_to(cout, 8), g.voc_res_kernels[a], pad_to(cout, 64)});
                }
        ch = cout;
    }
    need("voc.post.weight", 4ull * ch * g.voc_post_k); need("voc.post.bias", 4);
    if (!missing.empty()) return c->fail(-2, "missing or short weights: %s", missing.c_str());
    hipSetDevice(c->device);
    HIPCHK(c, hipMemcpy(&c->post_bias, c->W("voc.post.bias"), 4, hipMemcpyDeviceToHost));
    {   // x3 slabs: w = h + m + l in bf16 pieces, [chunk][kw][piece][row][16] (vv_vocoder_x3.hip); 1.5x the fp32 bytes
        size_t total = 0;
        for (const ConvW& w : convs) total = align_up(total, 256) + vvk_conv_split_bytes(w.cin_pad, w.kw, w.rows_pad);
        if (c->x3_buf) { HIPCHK(c, hipFree(c->x3_buf)); c->x3_buf = nullptr; }
        c->x3_w.clear();
        HIPCHK(c, hipMalloc((void**)&c->x3_buf, total));
        size_t off = 0;
        for (const ConvW& w : convs) {
            off = align_up(off, 256);
            const char* m__ = "";
            if (int r = vvk_conv_split_weights(c->Wf(w.name), w.cin_pad, w.kw, w.rows_pad, c->x3_buf + off, nullptr, &m__))
                return c->fail(r, "%s (%s)", m__, w.name.c_str());
            c->x3_w[w.name] = c->x3_buf + off;
            off += vvk_conv_split_bytes(w.cin_pad, w.kw, w.rows_pad);
        }
        HIPCHK(c, hipStreamSynchronize(nullptr));
    }
    // decode length multipliers: level 0 = frames, level s+1 = after upsample s
    std::vector<int> mult(g.voc_n_up + 1, 1);
    for (int s = 0; s < g.voc_n_up; ++s) mult[s + 1] = mult[s] * g.voc_up_rates[s];
    if (!c->d_mult) HIPCHK(c, hipMalloc((void**)&c->d_mult, sizeof(int) * (VV_MAX_UP + 1)));
    HIPCHK(c, hipMemcpy(c->d_mult, mult.data(), sizeof(int) * mult.size(), hipMemcpyHostToDevice));
    c->finalized = c->ever_finalized = true;
    return 0;
}

int vv_set_vocos(vv_ctx* c, const vv_vocos_cfg* v) {
    if (!c) return -22;
    if (!v) return c->fail(-22, "vv_set_vocos: null cfg");
    if (c->ever_finalized) return c->fail(-22, "vv_set_vocos: only between vv_create and vv_finalize_weights");
    const vv_model_cfg& g = c->cfg;
    if (v->dim < 128 || v->dim > 1024 || v->dim % 128 || v->intermediate < 128 || v->intermediate > 16384 || v->intermediate % 128)
        return c->fail(-22, "vv_set_vocos: dim must be a multiple of 128 in [128, 1024], intermediate a multiple of 128 (fp32 GEMM tiles)");
    if (v->layers < 1 || v->layers > 64 || v->embed_k < 1 || v->embed_k > 31 || v->embed_k % 2 == 0 || v->dw_k < 1 || v->dw_k > 31 || v->dw_k % 2 == 0 ||
        !(v->ln_eps > 0.f))
        return c->fail(-22, "vv_set_vocos: 1..64 layers, odd kernel sizes up to 31, ln_eps > 0");
    if (v->n_fft != v->win_length || v->n_fft != g.n_fft || g.win_length != g.n_fft || v->hop_length != g.hop_length || v->n_fft % 128 ||
        v->hop_length < 1 || v->n_fft % v->hop_length || v->n_fft / v->hop_length > 16)
        return c->fail(-22, "vv_set_vocos: the ISTFT needs n_fft == win_length == the model's n_fft (a multiple of 128) and the model's hop "
                            "(dividing n_fft, at most 16 frames per sample)");
    c->vcfg = *v;
    c->vocos = true;
    return 0;
}

// The tables of a plan: one modulation row per EVALUATION (n_steps * s of them; s = 1: the Euler time grid).  Everything is validated
// before the tables in force are touched.
static int set_plan_impl(vv_ctx* c, const char* who, const float* sinus_host, const float* dt_host, int n_steps, int s, const double* a,
                         const double* b, void* stream) {
    if (!c) return -22;
    if (!c->finalized) return c->fail(-1, "%s: weights not finalized", who);
    if (n_steps < 1 || n_steps > 512 || !sinus_host || !dt_host) return c->fail(-22, "%s: bad arguments", who);
    if (s < 1 || s > 4 || !a || !b) return c->fail(-22, "%s: 1 to 4 stages with their tableau", who);
    if ((long long)n_steps * s > 512) return c->fail(-22, "%s: %d steps x %d stages exceed 512 evaluations", who, n_steps, s);
    double sum_b = 0;
    for (int i = 0; i < s; ++i) {
        if (!std::isfinite(b[i])) return c->fail(-22, "%s: the tableau must be finite", who);
        sum_b += b[i];
        for (int j = 0; j < s; ++j) {
            if (!std::isfinite(a[i * s + j])) return c->fail(-22, "%s: the tableau must be finite", who);
            if (j >= i && a[i * s + j] != 0.0) return c->fail(-22, "%s: the tableau must be strictly lower triangular (explicit method)", who);
        }
    }
    if (!(std::fabs(sum_b - 1.0) < 1e-6)) return c->fail(-22, "%s: the weights b must sum to 1", who);
    for (int n = 0; n < n_steps; ++n)
        if (!std::isfinite(dt_host[n])) return c->fail(-22, "%s: the step sizes must be finite", who);
    hipSetDevice(c->device);
    hipStream_t st = (hipStream_t)stream;
    const int D = c->cfg.dim, S = n_steps * s, TF = c->cfg.time_freq_dim, L = c->cfg.depth;
    if (TF % 32) return c->fail(-22, "time_freq_dim must be a multiple of 32");
    if (c->modtab) { hipDeviceSynchronize(); hipFree(c->modtab); hipFree(c->fintab); c->modtab = c->fintab = nullptr; }
    HIPCHK(c, hipMalloc((void**)&c->modtab, sizeof(float) * (size_t)L * S * 6 * D));
    HIPCHK(c, hipMalloc((void**)&c->fintab, sizeof(float) * (size_t)S * 2 * D));
    float *sin_d, *t1, *t2;                  // the sinusoids of every evaluation and the two MLP outputs
    auto bufs = [&](Arena& a) { sin_d = a.take<float>((size_t)S * TF); t1 = a.take<float>((size_t)S * D); t2 = a.take<float>((size_t)S * D); };
    if (int r = plan_ws(c, nullptr, 0, bufs)) return r;
    HIPCHK(c, hipMemcpyAsync(sin_d, sinus_host, 4ull * S * TF, hipMemcpyHostToDevice, st));
    HIPCHK(c, hipStreamSynchronize(st));     // host buffer may be pageable; keep its lifetime simple
    const int f32 = VV_DTYPE_F32, store = VV_EPI_STORE;
    if (int r = launch_gemm(c, gemm_args(c, f32, f32, store, VV_ACT_SILU_, sin_d, TF, "time.mlp1.weight", TF, "time.mlp1.bias", t1, D, S, D, TF), VV_PROF_GEMM, st)) return r;
    if (int r = launch_gemm(c, gemm_args(c, f32, f32, store, VV_ACT_SILU_, t1, D, "time.mlp2.weight", D, "time.mlp2.bias", t2, D, S, D, D), VV_PROF_GEMM, st)) return r;
    // t2 = SiLU(t_emb): every AdaLN consumes the embedding through SiLU only
    for (int l = 0; l < L; ++l) {
        const std::string wn = blk(l, ".adaln.weight"), bn = blk(l, ".adaln.bias");
        if (int r = launch_gemm(c, gemm_args(c, f32, f32, store, VV_ACT_NONE_, t2, D, wn.c_str(), D, bn.c_str(), c->modtab + (size_t)l * S * 6 * D, 6 * D, S, 6 * D, D), VV_PROF_GEMM, st)) return r;
    }
    if (int r = launch_gemm(c, gemm_args(c, f32, f32, store, VV_ACT_NONE_, t2, D, "final.adaln.weight", D, "final.adaln.bias", c->fintab, 2 * D, S, 2 * D, D), VV_PROF_GEMM, st)) return r;
    HIPCHK(c, hipStreamSynchronize(st));
    c->n_steps = n_steps;
    c->dt_host.assign(dt_host, dt_host + n_steps);
    c->ode_s = s;
    std::fill(c->ode_a, c->ode_a + 16, 0.0);
    std::fill(c->ode_b, c->ode_b + 4, 0.0);
    for (int i = 0; i < s; ++i) {
        c->ode_b[i] = b[i];
        for (int j = 0; j < i; ++j) c->ode_a[i * 4 + j] = a[i * s + j];
    }
    // k_j lives in a buffer when a launch after the one that makes it reads it: a later stage state (a[m][j], m > j + 1) or the final sum
    c->ode_nk = 0;
    for (int j = 0; j < 4; ++j) {
        bool later = j < s - 1 && c->ode_b[j] != 0.0;
        for (int m = j + 2; m < s; ++m) later = later || c->ode_a[m * 4 + j] != 0.0;
        c->ode_kslot[j] = later ? c->ode_nk++ : -1;
    }
    c->ms_q = 0; c->ms_beta.clear();             // N20: a multistep plan and a report belong to the plan that was in force
    c->ode_report = nullptr; c->report_steps = c->report_B = 0;
    return 0;
}

int vv_set_time_grid(vv_ctx* c, const float* sinus_host, const float* dt_host, int n_steps, void* stream) {
    const double a = 0.0, b = 1.0;
    return set_plan_impl(c, "vv_set_time_grid", sinus_host, dt_host, n_steps, 1, &a, &b, stream);
}

int vv_set_ode_plan(vv_ctx* c, const float* sinus_host, const float* dt_host, int n_steps, int s, const double* a, const double* b, void* stream) {
    return set_plan_impl(c, "vv_set_ode_plan", sinus_host, dt_host, n_steps, s, a, b, stream);
}

// N20: an Adams-Bashforth plan = the Euler tables (one evaluation per step) and the weights of the kept slopes.  Everything is validated
// before the plan in force is touched.
int vv_set_ode_multistep(vv_ctx* c, const float* sinus_host, const float* dt_host, int n_steps, int q, const double* beta, void* stream) {
    if (!c) return -22;
    if (n_steps < 1 || n_steps > 512) return c->fail(-22, "vv_set_ode_multistep: bad arguments");
    if (q < 1 || q > 3 || !beta) return c->fail(-22, "vv_set_ode_multistep: 1 to 3 slopes per step with their weights");
    for (int n = 0; n < n_steps; ++n) {
        double sum = 0;
        for (int j = 0; j < q; ++j) {
            const double v = beta[(size_t)n * q + j];
            if (!std::isfinite(v)) return c->fail(-22, "vv_set_ode_multistep: the weights must be finite");
            if (j > n && v != 0.0) return c->fail(-22, "vv_set_ode_multistep: step %d has a weight on a slope from before step 0", n);
            sum += v;
        }
        if (!(std::fabs(sum - 1.0) < 1e-6)) return c->fail(-22, "vv_set_ode_multistep: the weights of step %d must sum to 1", n);
    }
    const double a = 0.0, b = 1.0;
    if (int r = set_plan_impl(c, "vv_set_ode_multistep", sinus_host, dt_host, n_steps, 1, &a, &b, stream)) return r;
    c->ms_q = q;
    c->ms_beta.assign(beta, beta + (size_t)n_steps * q);
    return 0;
}

int vv_set_ode_report(vv_ctx* c, double* report, int n_steps, int B) {
    if (!c) return -22;
    if (!report) { c->ode_report = nullptr; c->report_steps = c->report_B = 0; return 0; }
    if (c->ms_q < 1) return c->fail(-22, "vv_set_ode_report: the report needs a multistep plan (vv_set_ode_multistep)");
    if (n_steps != c->n_steps || B < 1 || B > VVK_GUIDE_MAX_ITEMS) return c->fail(-22, "vv_set_ode_report: [%d steps of the plan][1..%d items][2]", c->n_steps, VVK_GUIDE_MAX_ITEMS);
    if ((uintptr_t)report % 8) return c->fail(-22, "vv_set_ode_report: report must be a float64 array");
    c->ode_report = report; c->report_steps = n_steps; c->report_B = B;
    return 0;
}

// --------------------------------------------------------------------------------- preprocess
static int preprocess_impl(vv_ctx* c, int B, int N, const int16_t* audio, int ld_audio, int max_audio_len, const int32_t* audio_len,
                           const int32_t* audio_len_host, const int32_t* text_ids, int ld_text, const int32_t* text_len, const int32_t* seq_len,
                           float* cat, float* cat_drop, int32_t* ref_len, void* stream, const uint8_t* keep = nullptr, int ld_keep = 0) {
    // keep != nullptr (vv_preprocess_edit): the mel conditioning is masked by keep[b][t] on top of t < audio_len / hop + 1, and
    // ref_signal_len is 0 (the whole clip is decoded)
    if (!c) return -22;
    if (!c->finalized) return c->fail(-1, "vv_preprocess: weights not finalized");
    if (B < 1 || N < 1 || !audio || !audio_len || !text_ids || !text_len || !seq_len || !cat || !cat_drop || !ref_len)
        return c->fail(-22, "vv_preprocess: bad arguments");
    const vv_model_cfg& g = c->cfg;
    if (N > g.max_pos) return c->fail(-22, "vv_preprocess: N=%d exceeds the position tables (%d)", N, g.max_pos);
    if (max_audio_len < g.n_fft || max_audio_len > ld_audio) return c->fail(-22, "vv_preprocess: reference clips must hold >= n_fft samples and fit ld_audio");
    // A centred STFT reflects n_fft / 2 samples at both ends of a clip: defined only for clips of more than n_fft / 2 samples (torch.stft
    // refuses shorter ones).  The host lengths let the call refuse such an item before anything is launched; without them the mel kernel
    // clamps the doubly reflected index (finite and deterministic, but no reference defines it).
    if (audio_len_host)
        for (int b = 0; b < B; ++b)
            if (audio_len_host[b] < g.n_fft / 2 + 1 || audio_len_host[b] > max_audio_len)
                return c->fail(-22, "vv_preprocess: reference clip %d has %d samples; a clip needs between n_fft/2 + 1 = %d and max_audio_len = %d",
                               b, audio_len_host[b], g.n_fft / 2 + 1, max_audio_len);
    hipSetDevice(c->device);
    hipStream_t st = (hipStream_t)stream;
    const int Dt = g.text_dim, C2 = Dt * g.text_ff_mult, M = g.n_mel, es = c->esz();
    const int F_max = max_audio_len / g.hop_length + 1;
    const size_t R2 = (size_t)2 * B * N;
    float *mel, *tx, *ty, *sumsq;            // the reference mels, the text stream and its conv output (fp32), the GRN sums
    char *th, *tm;                           // operand dtype: the norm output and the MLP plane
    auto bufs = [&](Arena& a) {
        mel = a.take<float>((size_t)B * F_max * M);
        tx = a.take<float>(R2 * Dt); ty = a.take<float>(R2 * Dt);
        th = a.take<char>((size_t)es * R2 * Dt); tm = a.take<char>((size_t)es * R2 * C2);
        sumsq = a.take<float>((size_t)2 * B * C2);
    };
    if (int r = plan_ws(c, nullptr, 0, bufs)) return r;

    KCHK(c, vvk_ref_len(audio_len, ref_len, B, g.hop_length, st, &m__));
    {
        Prof p(c, VV_PROF_MEL, 4.0 * B * F_max * (double)g.n_fft * (g.n_fft / 2 + 1), 2.0 * B * max_audio_len + 4.0 * B * F_max * M, st);
        KCHK(c, vvk_mel(audio, ld_audio, audio_len, c->Wf("const.window"), c->Wf("const.tw_cos"), c->Wf("const.tw_sin"),
                        c->Wf("const.mel_fb"), mel, B, F_max, g.n_fft, g.hop_length, M, st, &m__));
    }
    {
        Prof p(c, VV_PROF_TEXT, 0, 8.0 * R2 * Dt, st);
        KCHK(c, vvk_text_embed(text_ids, ld_text, text_len, c->Wf("text.embed.weight"), c->Wf("const.text_pos"), tx, B, N, Dt, g.vocab_rows, st, &m__));
    }
    for (int i = 0; i < g.text_layers; ++i) {
        const std::string p = "text.blocks." + std::to_string(i);
        {
            Prof pr(c, VV_PROF_TEXT, 2.0 * R2 * Dt * g.text_conv_k, 8.0 * R2 * Dt, st);
            KCHK(c, vvk_dwconv(tx, ty, c->Wf(p + ".dwconv.weight"), c->Wf(p + ".dwconv.bias"), seq_len, B, 2 * B, N, Dt, g.text_conv_k, st, &m__));
        }
        {
            vv_ln_args a{}; a.out_dtype = c->dt; a.x = ty; a.ldx = Dt; a.y = th; a.ldy = Dt; a.R = (int)R2; a.D = Dt;
            a.w = c->Wf(p + ".norm.weight"); a.b = c->Wf(p + ".norm.bias"); a.add_one = 0; a.eps = 1e-6f;
            Prof pr(c, VV_PROF_NORM, 0, (4.0 + es) * R2 * Dt, st);
            KCHK(c, vvk_ln_mod(&a, st, &m__));
        }
        const std::string w1 = p + ".pwconv1.weight", b1 = p + ".pwconv1.bias", w2 = p + ".pwconv2.weight", b2 = p + ".pwconv2.bias";
        if (int r = launch_gemm(c, gemm_args(c, c->dt, c->dt, VV_EPI_STORE, VV_ACT_GELU_ERF_, th, Dt, w1.c_str(), Dt, b1.c_str(), tm, C2, (int)R2, C2, Dt), VV_PROF_GEMM, st)) return r;
        {
            Prof pr(c, VV_PROF_TEXT, 0, 3.0 * es * R2 * C2, st);
            KCHK(c, vvk_grn(c->dt, tm, sumsq, c->Wf(p + ".grn.gamma"), c->Wf(p + ".grn.beta"), seq_len, B, 2 * B, N, C2, st, &m__));
        }
        if (int r = launch_gemm(c, gemm_args(c, c->dt, VV_DTYPE_F32, VV_EPI_GATE_RES, VV_ACT_NONE_, tm, C2, w2.c_str(), C2, b2.c_str(), tx, Dt, (int)R2, Dt, C2), VV_PROF_GEMM, st)) return r;
    }
    {
        Prof p(c, VV_PROF_ELEMWISE, 0, 12.0 * B * N * (M + Dt) + (keep ? (double)B * N : 0.0), st);
        KCHK(c, vvk_build_cat(mel, F_max, ref_len, tx, cat, cat_drop, B, N, M, Dt, st, &m__, keep, ld_keep));
    }
    if (keep) HIPCHK(c, hipMemsetAsync(ref_len, 0, sizeof(int32_t) * B, st));     // the frame bound of the build above, now the decode start
    return 0;
}

int vv_preprocess(vv_ctx* c, int B, int N, const int16_t* audio, int ld_audio, int max_audio_len, const int32_t* audio_len,
                  const int32_t* text_ids, int ld_text, const int32_t* text_len, const int32_t* seq_len, float* cat,
                  float* cat_drop, int32_t* ref_len, void* stream) {
    return preprocess_impl(c, B, N, audio, ld_audio, max_audio_len, audio_len, nullptr, text_ids, ld_text, text_len, seq_len, cat, cat_drop, ref_len, stream);
}

// Same, with the clip lengths ALSO given on the host (the same values as the device array): an item shorter than n_fft / 2 + 1 samples
// is refused with -22 before anything is launched.
int vv_preprocess_h(vv_ctx* c, int B, int N, const int16_t* audio, int ld_audio, int max_audio_len, const int32_t* audio_len,
                    const int32_t* audio_len_host, const int32_t* text_ids, int ld_text, const int32_t* text_len, const int32_t* seq_len,
                    float* cat, float* cat_drop, int32_t* ref_len, void* stream) {
    if (c && !audio_len_host) return c->fail(-22, "vv_preprocess_h: host lengths missing");
    return preprocess_impl(c, B, N, audio, ld_audio, max_audio_len, audio_len, audio_len_host, text_ids, ld_text, text_len, seq_len, cat, cat_drop, ref_len, stream);
}

// Speech editing (N5): the conditioning as a frame mask keep [B][ld_keep] (device, ld_keep >= N) instead of the clip's prefix.
int vv_preprocess_edit(vv_ctx* c, int B, int N, const int16_t* audio, int ld_audio, int max_audio_len, const int32_t* audio_len,
                       const int32_t* audio_len_host, const int32_t* text_ids, int ld_text, const int32_t* text_len, const int32_t* seq_len,
                       float* cat, float* cat_drop, int32_t* ref_len, const uint8_t* keep, int ld_keep, void* stream) {
    if (!c) return -22;
    if (!audio_len_host) return c->fail(-22, "vv_preprocess_edit: host lengths missing");
    if (!keep || ld_keep < N) return c->fail(-22, "vv_preprocess_edit: keep must be a device array [B][ld_keep] with ld_keep >= N");
    return preprocess_impl(c, B, N, audio, ld_audio, max_audio_len, audio_len, audio_len_host, text_ids, ld_text, text_len, seq_len, cat, cat_drop,
                           ref_len, stream, keep, ld_keep);
}

int vv_edit_splice(vv_ctx* c, const int16_t* src, int64_t n_src, const int64_t* desc, int n_rows, int B, int16_t* out, int ld_out, void* stream) {
    if (!c) return -22;
    if (B < 1 || n_rows < 0 || n_src < 0 || !out || ld_out < 4 || ld_out % 4 || (uintptr_t)out % 8 || (n_rows > 0 && (!src || !desc)))
        return c->fail(-22, "vv_edit_splice: bad arguments (out [B][ld_out] 8-byte aligned with ld_out %% 4 == 0; src and desc for n_rows > 0)");
    hipSetDevice(c->device);
    hipStream_t st = (hipStream_t)stream;
    Prof p(c, VV_PROF_ELEMWISE, 0, 4.0 * B * ld_out + 32.0 * n_rows, st);
    KCHK(c, vvk_edit_splice(src, (long long)n_src, (const long long*)desc, n_rows, B, out, ld_out, st, &m__));
    return 0;
}

int vv_edit_restore(vv_ctx* c, int B, int N, float* x, const float* cat, const uint8_t* keep, int ld_keep, const int32_t* seq_len, void* stream) {
    if (!c) return -22;
    const int M = c->cfg.n_mel, cd = c->cfg.n_mel + c->cfg.text_dim;
    if (B < 1 || N < 1 || !x || !cat || !keep || !seq_len || ld_keep < N || (uintptr_t)x % 16 || (uintptr_t)cat % 16)
        return c->fail(-22, "vv_edit_restore: bad arguments (x, cat 16-byte aligned; keep [B][ld_keep] with ld_keep >= N)");
    hipSetDevice(c->device);
    hipStream_t st = (hipStream_t)stream;
    Prof p(c, VV_PROF_ELEMWISE, 0, (double)B * N * (1 + 8.0 * M), st);
    KCHK(c, vvk_edit_restore(x, cat, keep, ld_keep, seq_len, B, N, M, cd, st, &m__));
    return 0;
}

// N9: the start noise of the flow ODE, drawn on the device.  Every argument is checked before the launch; a refused call launches nothing.
int vv_noise_fill(vv_ctx* c, int B, int N, int n_mel, float* x, const int32_t* seq_len, const uint64_t* keys, int kind, void* stream) {
    if (!c) return -22;
    if (B < 1 || N < 1 || n_mel < 4 || n_mel % 4 || (kind != 0 && kind != 1) || !x || !seq_len || !keys || (uintptr_t)x % 16 || (uintptr_t)keys % 8)
        return c->fail(-22, "vv_noise_fill: bad arguments (B, N >= 1; n_mel %% 4 == 0; x 16-byte aligned; keys [B][2] uint64; kind 0 or 1)");
    hipSetDevice(c->device);
    hipStream_t st = (hipStream_t)stream;
    Prof p(c, VV_PROF_ELEMWISE, 0, (double)B * (12.0 + 4.0 * N * n_mel), st);
    KCHK(c, vvk_noise_fill(x, seq_len, (const unsigned long long*)keys, B, N, n_mel, kind, st, &m__));
    return 0;
}

// N10: the output stage.  Every argument the host can see is checked before a launch; a refused call launches nothing.
int vv_join_chunks(vv_ctx* c, const int16_t* pcm, int64_t n_pcm, const int64_t* chunk_rows, const int64_t* chunk_rows_host, int n_chunks,
                   const int64_t* req_rows, const int64_t* req_rows_host, int R, const double* fade, int64_t n_fade, int max_n, int64_t max_len,
                   int16_t* out, int64_t n_out, void* ws, void* stream) {
    if (!c) return -22;
    hipStream_t st = enter(c, stream);
    if (R < 1 || n_chunks < R || max_n < 0 || max_n > vvk_join_max_n())
        return c->fail(-22, "vv_join_chunks: bad arguments (1 <= R <= n_chunks; max_n <= %d)", vvk_join_max_n());
    if (int e = check_ptrs(c, "vv_join_chunks", {{"pcm", pcm}, {"chunk_rows", chunk_rows}, {"req_rows", req_rows}, {"out", out, 16}, {"ws", ws}})) return e;
    if ((chunk_rows_host == nullptr) != (req_rows_host == nullptr)) return c->fail(-22, "vv_join_chunks: host rows come as a pair or not at all");
    if (chunk_rows_host) {               // the same rows on the host: checked here, before anything is launched
        for (int r = 0; r < R; ++r) {
            const int64_t* q = req_rows_host + 4 * (size_t)r;
            if (q[1] < 1 || !fits(q[0], q[1], n_chunks) || !fits(q[2], q[3], n_out))
                return c->fail(-22, "vv_join_chunks: request row %d does not fit the chunk rows or the output", r);
            for (int64_t k = q[0]; k < q[0] + q[1]; ++k) {
                const int64_t* w = chunk_rows_host + 8 * (size_t)k;
                if (!fits(w[0], w[1], n_pcm) || w[2] < 0 || w[3] < 0 || w[3] > max_n || w[1] > max_len || w[7] != r ||
                    (w[3] > 0 && !fits(w[5], 2 * w[3], n_fade)))
                    return c->fail(-22, "vv_join_chunks: chunk row %lld does not fit the buffers", (long long)k);
                if (q[1] >= 2 && w[1] <= 0)
                    return c->fail(-22, "vv_join_chunks: chunk %lld is empty inside a request of %lld chunks", (long long)k, (long long)q[1]);
            }
        }
    }
    Prof p(c, VV_PROF_ELEMWISE, 0, 4.0 * (double)n_out + 96.0 * n_chunks, st);
    KCHK(c, vvk_join_chunks(pcm, (long long)n_pcm, (const long long*)chunk_rows, n_chunks, (const long long*)req_rows, R, fade, (long long)n_fade,
                            max_n, (long long)max_len, out, (long long)n_out, ws, st, &m__));
    return 0;
}

int vv_pcm_resample(vv_ctx* c, const int16_t* x, int64_t n_x, const int64_t* rows, int n_rows, int64_t max_out, const double* taps, int n_taps,
                    int up, int down, int skip, int16_t* y, int64_t n_y, void* stream) {
    if (!c) return -22;
    hipStream_t st = enter(c, stream);
    if (n_rows < 1 || n_taps < 1 || up < 1 || down < 1 || skip < 0 || max_out < 0)
        return c->fail(-22, "vv_pcm_resample: bad arguments (n_rows, n_taps, up, down >= 1; skip, max_out >= 0)");
    if (int e = check_ptrs(c, "vv_pcm_resample", {{"x", x}, {"rows", rows}, {"taps", taps}, {"y", y}})) return e;
    Prof p(c, VV_PROF_ELEMWISE, 2.0 * (double)n_y * (n_taps / up + 1), 2.0 * (double)(n_x + n_y), st);
    KCHK(c, vvk_pcm_resample(x, (long long)n_x, (const long long*)rows, n_rows, (long long)max_out, taps, n_taps, up, down, skip, y, (long long)n_y,
                             st, &m__));
    return 0;
}

int vv_pcm_encode(vv_ctx* c, const int16_t* x, int64_t n_x, const int64_t* rows, int n_rows, int64_t max_n, int kind, uint8_t* y, int64_t n_y,
                  void* stream) {
    if (!c) return -22;
    hipStream_t st = enter(c, stream);
    if (n_rows < 1 || (kind != 1 && kind != 2) || max_n < 0)
        return c->fail(-22, "vv_pcm_encode: bad arguments (n_rows >= 1; kind 1 = mu-law, 2 = A-law)");
    if (int e = check_ptrs(c, "vv_pcm_encode", {{"x", x}, {"rows", rows}, {"y", y, 8}})) return e;
    Prof p(c, VV_PROF_ELEMWISE, 0, 2.0 * (double)n_x + (double)n_y, st);
    KCHK(c, vvk_pcm_encode(x, (long long)n_x, (const long long*)rows, n_rows, (long long)max_n, kind, y, (long long)n_y, st, &m__));
    return 0;
}

// N12: loudness normalisation of the joined signal.  The rows come in host memory too, so everything is checked before a launch.
uint64_t vv_pcm_loudness_ws_bytes(int64_t total_runs, int R) { return vvk_pcm_loudness_ws_bytes((long long)total_runs, R); }

int vv_pcm_loudness(vv_ctx* c, const int16_t* x, int64_t n_x, const int64_t* rows, const int64_t* rows_host, int R, int64_t sub,
                    const double* tables, const double* params, int16_t* y, int64_t n_y, double* stats, void* ws, uint64_t ws_bytes,
                    void* stream) {
    if (!c) return -22;
    hipStream_t st = enter(c, stream);
    if (R < 1 || R > 65535 || sub < VV_LOUD_RUN || sub > (1 << 24) || n_x < 0 || n_y < 0)
        return c->fail(-22, "vv_pcm_loudness: bad sizes (1 <= R <= 65535; sub >= %d)", VV_LOUD_RUN);
    if (int e = check_ptrs(c, "vv_pcm_loudness", {{"x", x, 2}, {"y", y, 2, true}, {"rows", rows, 8}, {"rows_host", rows_host}, {"tables", tables, 8},
                                                  {"params", params, 8}, {"stats", stats, 8}, {"ws", ws, 8}})) return e;
    const int64_t rps = (sub + VV_LOUD_RUN - 1) / VV_LOUD_RUN;
    int64_t total_runs = 0, max_n = 0;
    for (int r = 0; r < R; ++r) {
        const int64_t* q = rows_host + 4 * (size_t)r;
        if (!fits(q[0], q[1], n_x) || q[1] >= ((int64_t)1 << 40))
            return c->fail(-22, "vv_pcm_loudness: row %d does not fit the %lld samples of x", r, (long long)n_x);
        if (y && !fits(q[2], q[1], n_y)) return c->fail(-22, "vv_pcm_loudness: row %d does not fit the %lld samples of y", r, (long long)n_y);
        if (y == x && q[2] != q[0]) return c->fail(-22, "vv_pcm_loudness: in place (y == x) needs dst_off == src_off, row %d", r);
        if (q[3] != total_runs) return c->fail(-22, "vv_pcm_loudness: row %d: run_off is the sum of the runs of the rows before it", r);
        const int64_t J = q[1] / sub;
        total_runs += J * rps + (q[1] - J * sub + VV_LOUD_RUN - 1) / VV_LOUD_RUN;
        if (q[1] > max_n) max_n = q[1];
    }
    if (int e = check_ws(c, "vv_pcm_loudness", ws_bytes, vvk_pcm_loudness_ws_bytes((long long)total_runs, R))) return e;
    Prof p(c, VV_PROF_ELEMWISE, 60.0 * (double)n_x, 6.0 * (double)n_x + 128.0 * (double)total_runs, st);
    KCHK(c, vvk_pcm_loudness(x, (long long)n_x, (const long long*)rows, R, (long long)sub, (long long)total_runs, (long long)max_n, tables,
                             params, y, (long long)n_y, stats, ws, st, &m__));
    return 0;
}

// N13: look-ahead peak limiter of the joined signal.  As with N12 the rows come in host memory too: everything is checked before a launch.
int vv_pcm_limit_tile(int L) { return L < 1 || L > VV_LIMIT_MAX_L ? -22 : vvk_pcm_limit_tile(L); }

uint64_t vv_pcm_limit_ws_bytes(int64_t total_samples, int64_t total_tiles, int R) {
    return vvk_pcm_limit_ws_bytes((long long)total_samples, (long long)total_tiles, R);
}

int vv_pcm_limit(vv_ctx* c, const int16_t* x, int64_t n_x, const int64_t* rows, const int64_t* rows_host, int R, int L, int mode,
                 const double* window, const double* taps, const double* params, const double* meas, int16_t* y, int64_t n_y, double* stats,
                 void* ws, uint64_t ws_bytes, void* stream) {
    if (!c) return -22;
    hipStream_t st = enter(c, stream);
    if (R < 1 || R > 65535 || L < 1 || L > VV_LIMIT_MAX_L || (mode != 0 && mode != 1) || n_x < 0 || n_y < 0)
        return c->fail(-22, "vv_pcm_limit: bad sizes (1 <= R <= 65535; 1 <= L <= %d; mode 0 or 1)", VV_LIMIT_MAX_L);
    if (int e = check_ptrs(c, "vv_pcm_limit", {{"x", x, 2}, {"y", y, 2, true}, {"rows", rows, 8}, {"rows_host", rows_host}, {"window", window, 8},
                                               {"taps", taps, 8}, {"params", params, 8}, {"meas", meas, 8, true}, {"stats", stats, 8}, {"ws", ws, 8}})) return e;
    const int64_t tile = vvk_pcm_limit_tile(L);
    int64_t total_samples = 0, total_tiles = 0, max_tiles = 0, max_out = 0;
    for (int r = 0; r < R; ++r) {
        const int64_t* q = rows_host + 5 * (size_t)r;
        if (q[0] < 0 || q[1] < 0 || q[2] < 0 || q[3] < 0 || q[4] < 0) return c->fail(-22, "vv_pcm_limit: row %d has a negative field", r);
        if (!fits(q[0], q[1], n_x) || q[1] >= ((int64_t)1 << 40))
            return c->fail(-22, "vv_pcm_limit: row %d does not fit the %lld samples of x", r, (long long)n_x);
        if (!fits(q[3], q[4], q[1])) return c->fail(-22, "vv_pcm_limit: row %d: out_lo + out_n exceeds n", r);
        if (y && !fits(q[2], q[4], n_y)) return c->fail(-22, "vv_pcm_limit: row %d does not fit the %lld samples of y", r, (long long)n_y);
        if (y == x && q[4] > 0 && q[2] != q[0] + q[3])
            return c->fail(-22, "vv_pcm_limit: in place (y == x) needs dst_off == src_off + out_lo, row %d", r);
        const int64_t nt = (q[1] + tile - 1) / tile;
        total_samples += q[1];
        total_tiles += nt;
        if (nt > max_tiles) max_tiles = nt;
        if (q[4] > max_out) max_out = q[4];
    }
    if (int e = check_ws(c, "vv_pcm_limit", ws_bytes, vvk_pcm_limit_ws_bytes((long long)total_samples, (long long)total_tiles, R))) return e;
    Prof p(c, VV_PROF_ELEMWISE, (mode ? 640.0 : 500.0) * (double)total_samples * (double)(2 * L + 1) / 241.0,
           20.0 * (double)total_samples + 2.0 * (double)max_out * R, st);
    KCHK(c, vvk_pcm_limit(x, (long long)n_x, (const long long*)rows, R, L, mode, (long long)total_samples, (long long)total_tiles,
                          (long long)max_tiles, (long long)max_out, window, taps, params, meas, y, (long long)n_y, stats, ws, st, &m__));
    return 0;
}

// N14: WSOLA time stretch of the joined signal.  As with N12 and N13 the rows come in host memory too: everything is checked before a launch.
uint64_t vv_pcm_stretch_ws_bytes(int R) { return vvk_pcm_stretch_ws_bytes(R); }

int vv_pcm_stretch(vv_ctx* c, const int16_t* x, int64_t n_x, const int64_t* rows, const int64_t* rows_host, int R, const double* window,
                   int16_t* y, int64_t n_y, int32_t* pos, int64_t n_pos, void* ws, uint64_t ws_bytes, void* stream) {
    if (!c) return -22;
    hipStream_t st = enter(c, stream);
    if (R < 1 || R > 65535 || n_x < 0 || n_y < 0 || n_pos < 0) return c->fail(-22, "vv_pcm_stretch: bad sizes (1 <= R <= 65535)");
    if (int e = check_ptrs(c, "vv_pcm_stretch", {{"x", x, 2}, {"y", y, 2, true}, {"rows", rows, 8}, {"rows_host", rows_host}, {"window", window, 8},
                                                 {"pos", pos, 4}, {"ws", ws, 8}})) return e;
    if (y && spans_overlap(x, 2ull * n_x, y, 2ull * n_y))
        return c->fail(-22, "vv_pcm_stretch: y overlaps x (an output sample reads two frames of the input: not in place)");
    if (int e = check_ws(c, "vv_pcm_stretch", ws_bytes, vvk_pcm_stretch_ws_bytes(R))) return e;
    std::vector<std::pair<int64_t, int64_t>> on_y, on_pos;
    int64_t total_out = 0, total_frames = 0, max_out = 0;
    for (int r = 0; r < R; ++r) {
        const int64_t* q = rows_host + 6 * (size_t)r;
        if (q[0] < 0 || q[1] < 0 || q[2] < 0 || q[5] < 0) return c->fail(-22, "vv_pcm_stretch: row %d has a negative field", r);
        if (q[3] < 1 || q[3] > VV_WSOLA_MAX_PQ || q[4] < 1 || q[4] > VV_WSOLA_MAX_PQ || q[3] == q[4] || 4 * q[3] < q[4] || q[3] > 4 * q[4])
            return c->fail(-22, "vv_pcm_stretch: row %d: p and q in 1 ... %d, p != q, 1/4 <= p / q <= 4", r, VV_WSOLA_MAX_PQ);
        if (!fits(q[0], q[1], n_x) || q[1] > ((int64_t)1 << 30))
            return c->fail(-22, "vv_pcm_stretch: row %d does not fit the %lld samples of x", r, (long long)n_x);
        const int64_t n_s = (q[1] * q[3] + q[4] - 1) / q[4], M = (n_s + VV_WSOLA_HS - 1) / VV_WSOLA_HS;
        if (y && !fits(q[2], n_s, n_y)) return c->fail(-22, "vv_pcm_stretch: row %d does not fit the %lld samples of y", r, (long long)n_y);
        if (!fits(q[5], M + 1, n_pos)) return c->fail(-22, "vv_pcm_stretch: row %d does not fit the %lld entries of pos", r, (long long)n_pos);
        if (y && n_s > 0) on_y.emplace_back(q[2], q[2] + n_s);
        on_pos.emplace_back(q[5], q[5] + M + 1);
        total_out += n_s;
        total_frames += M;
        if (n_s > max_out) max_out = n_s;
    }
    for (auto* spans : {&on_y, &on_pos}) {
        std::sort(spans->begin(), spans->end());
        for (size_t i = 1; i < spans->size(); ++i)
            if ((*spans)[i].first < (*spans)[i - 1].second)
                return c->fail(-22, "vv_pcm_stretch: rows overlap on %s", spans == &on_y ? "y" : "pos");
    }
    Prof p(c, VV_PROF_ELEMWISE, 2.0 * (double)total_frames * VV_WSOLA_N * 2 * VV_WSOLA_D + 3.0 * (double)total_out,
           2.0 * (double)total_frames * (2 * VV_WSOLA_N + 2 * VV_WSOLA_D) + 6.0 * (double)total_out, st);
    KCHK(c, vvk_pcm_stretch(x, (long long)n_x, (const long long*)rows, R, (long long)max_out, window, y, (long long)n_y, (int*)pos,
                            (long long)n_pos, ws, st, &m__));
    return 0;
}

// N18: the envelope correction of a pitch shift.  As with N12 ... N14 the rows come in host memory too: everything is checked before a launch.
uint64_t vv_pcm_formant_ws_bytes(int64_t total_frames, int R) { return vvk_pcm_formant_ws_bytes((long long)total_frames, R); }

int vv_pcm_formant(vv_ctx* c, const int16_t* x, int64_t n_x, const int16_t* y, int64_t n_y, const int64_t* rows, const int64_t* rows_host, int R,
                   const double* wa, const double* g, const double* window, int16_t* z, int64_t n_z, double* h_out, int64_t n_h, void* ws,
                   uint64_t ws_bytes, void* stream) {
    if (!c) return -22;
    hipStream_t st = enter(c, stream);
    if (R < 1 || R > 65535 || n_x < 0 || n_y < 0 || n_z < 0 || n_h < 0) return c->fail(-22, "vv_pcm_formant: bad sizes (1 <= R <= 65535)");
    if (int e = check_ptrs(c, "vv_pcm_formant", {{"x", x, 2}, {"y", y, 2}, {"rows", rows, 8}, {"rows_host", rows_host}, {"wa", wa, 8}, {"g", g, 8},
                                                 {"window", window, 8}, {"z", z, 2}, {"h_out", h_out, 8, true}, {"ws", ws, 8}})) return e;
    if (spans_overlap(x, 2ull * n_x, z, 2ull * n_z) || spans_overlap(y, 2ull * n_y, z, 2ull * n_z))
        return c->fail(-22, "vv_pcm_formant: z overlaps x or y (an output sample reads L samples of y: not in place)");
    std::vector<std::pair<int64_t, int64_t>> on_z;
    int64_t total_frames = 0, max_frames = 0, total_out = 0;
    for (int r = 0; r < R; ++r) {
        const int64_t* q = rows_host + 7 * (size_t)r;
        if (q[0] < 0 || q[1] < 0 || q[2] < 0 || q[3] < 0 || q[4] < 0) return c->fail(-22, "vv_pcm_formant: row %d has a negative field", r);
        if (q[5] < 1 || q[5] > VV_WSOLA_MAX_PQ || q[6] < 1 || q[6] > VV_WSOLA_MAX_PQ)
            return c->fail(-22, "vv_pcm_formant: row %d: tn and td in 1 ... %d", r, VV_WSOLA_MAX_PQ);
        if (!fits(q[0], q[1], n_x) || q[1] > ((int64_t)1 << 30))
            return c->fail(-22, "vv_pcm_formant: row %d does not fit the %lld samples of x", r, (long long)n_x);
        if (q[3] != (q[1] * q[6] + q[5] - 1) / q[5]) return c->fail(-22, "vv_pcm_formant: row %d: n_f is not ceil(n td / tn)", r);
        if (!fits(q[2], q[3], n_y)) return c->fail(-22, "vv_pcm_formant: row %d does not fit the %lld samples of y", r, (long long)n_y);
        if (!fits(q[4], q[3], n_z)) return c->fail(-22, "vv_pcm_formant: row %d does not fit the %lld samples of z", r, (long long)n_z);
        const int64_t frames = (q[3] + VV_FORMANT_H - 1) / VV_FORMANT_H + 1;
        if (q[3] > 0) on_z.emplace_back(q[4], q[4] + q[3]);
        total_frames += frames;
        total_out += q[3];
        if (frames > max_frames) max_frames = frames;
    }
    std::sort(on_z.begin(), on_z.end());
    for (size_t i = 1; i < on_z.size(); ++i)
        if (on_z[i].first < on_z[i - 1].second) return c->fail(-22, "vv_pcm_formant: rows overlap on z");
    if (h_out && n_h / VV_FORMANT_L < total_frames)
        return c->fail(-22, "vv_pcm_formant: h_out of %lld doubles, %lld are needed", (long long)n_h, (long long)total_frames * VV_FORMANT_L);
    if (int e = check_ws(c, "vv_pcm_formant", ws_bytes, vvk_pcm_formant_ws_bytes((long long)total_frames, R))) return e;
    Prof p(c, VV_PROF_ELEMWISE, 4.0 * (double)total_out * VV_FORMANT_L + 2.0 * (double)total_frames * VV_FORMANT_L * VV_FORMANT_P,
           24.0 * (double)total_frames * VV_FORMANT_L + 4.0 * (double)total_out, st);
    KCHK(c, vvk_pcm_formant(x, (long long)n_x, y, (long long)n_y, (const long long*)rows, R, (long long)total_frames, (long long)max_frames, wa, g,
                            window, z, (long long)n_z, h_out, ws, st, &m__));
    return 0;
}

// N19: the vocoder-bias denoiser.  As with N12 ... N18 the rows come in host memory too, and so do the strengths: everything is checked before
// a launch.
uint64_t vv_pcm_denoise_ws_bytes(int R) { return vvk_pcm_denoise_ws_bytes(R); }

int vv_pcm_denoise(vv_ctx* c, const int16_t* x, int64_t n_x, const int64_t* rows, const int64_t* rows_host, int R, const double* strengths,
                   const double* strengths_host, const double* bias, int64_t n_bias, const double* window, const double* twiddles, int16_t* y,
                   int64_t n_y, double* mag_out, int64_t n_mag, void* ws, uint64_t ws_bytes, void* stream) {
    if (!c) return -22;
    hipStream_t st = enter(c, stream);
    if (R < 1 || R > 65535 || n_x < 0 || n_y < 0 || n_bias < 1 || n_mag < 0) return c->fail(-22, "vv_pcm_denoise: bad sizes (1 <= R <= 65535, n_bias >= 1)");
    if (int e = check_ptrs(c, "vv_pcm_denoise", {{"x", x, 2}, {"rows", rows, 8}, {"rows_host", rows_host}, {"strengths", strengths, 8},
                                                 {"strengths_host", strengths_host}, {"bias", bias, 8}, {"window", window, 8},
                                                 {"twiddles", twiddles, 8}, {"y", y, 2}, {"mag_out", mag_out, 8, true}, {"ws", ws, 8}})) return e;
    if (spans_overlap(x, 2ull * n_x, y, 2ull * n_y))
        return c->fail(-22, "vv_pcm_denoise: y overlaps x (a hop reads the input under its neighbours: not in place)");
    std::vector<std::pair<int64_t, int64_t>> on_y;
    int64_t total_frames = 0, max_hops = 1, total_hops = 0;
    for (int r = 0; r < R; ++r) {
        const int64_t* q = rows_host + 4 * (size_t)r;
        if (q[0] < 0 || q[1] < 0 || q[2] < 0 || q[3] < 0) return c->fail(-22, "vv_pcm_denoise: row %d has a negative field", r);
        if (q[3] >= n_bias) return c->fail(-22, "vv_pcm_denoise: row %d: bias_row %lld of %lld", r, (long long)q[3], (long long)n_bias);
        if (!(strengths_host[r] >= 0.0 && strengths_host[r] <= 16.0)) return c->fail(-22, "vv_pcm_denoise: row %d: a strength in 0 ... 16 is needed", r);
        if (!fits(q[0], q[1], n_x) || q[1] > ((int64_t)1 << 30))
            return c->fail(-22, "vv_pcm_denoise: row %d does not fit the %lld samples of x", r, (long long)n_x);
        if (!fits(q[2], q[1], n_y)) return c->fail(-22, "vv_pcm_denoise: row %d does not fit the %lld samples of y", r, (long long)n_y);
        const int64_t M = (q[1] + VV_DENOISE_H - 1) / VV_DENOISE_H, hops = M > 0 ? M : 1;
        if (q[1] > 0) on_y.emplace_back(q[2], q[2] + q[1]);
        total_frames += M + 3;
        total_hops += hops;
        if (hops > max_hops) max_hops = hops;
    }
    std::sort(on_y.begin(), on_y.end());
    for (size_t i = 1; i < on_y.size(); ++i)
        if (on_y[i].first < on_y[i - 1].second) return c->fail(-22, "vv_pcm_denoise: rows overlap on y");
    if (mag_out && n_mag / VV_DENOISE_N < total_frames)
        return c->fail(-22, "vv_pcm_denoise: mag_out of %lld doubles, %lld are needed", (long long)n_mag, (long long)total_frames * VV_DENOISE_N);
    if (int e = check_ws(c, "vv_pcm_denoise", ws_bytes, vvk_pcm_denoise_ws_bytes(R))) return e;
    Prof p(c, VV_PROF_ELEMWISE, (double)total_hops * 8.0 * 10.0 * 512.0 * 10.0, 16.0 * (double)total_hops * VV_DENOISE_H, st);
    KCHK(c, vvk_pcm_denoise(x, (long long)n_x, (const long long*)rows, R, (long long)total_frames, (long long)max_hops, strengths, bias,
                            (long long)n_bias, window, twiddles, y, (long long)n_y, mag_out, ws, st, &m__));
    return 0;
}

uint64_t vv_pcm_denoise_bias_ws_bytes(int64_t total_frames, int R) { return vvk_pcm_denoise_bias_ws_bytes((long long)total_frames, R); }

int vv_pcm_denoise_bias(vv_ctx* c, const int16_t* x, int64_t n_x, const int64_t* rows, const int64_t* rows_host, int R, const double* window,
                        const double* twiddles, double* out, int64_t n_out, void* ws, uint64_t ws_bytes, void* stream) {
    if (!c) return -22;
    hipStream_t st = enter(c, stream);
    if (R < 1 || R > 65535 || n_x < 0 || n_out < 0) return c->fail(-22, "vv_pcm_denoise_bias: bad sizes (1 <= R <= 65535)");
    if (int e = check_ptrs(c, "vv_pcm_denoise_bias", {{"x", x, 2}, {"rows", rows, 8}, {"rows_host", rows_host}, {"window", window, 8},
                                                      {"twiddles", twiddles, 8}, {"out", out, 8}, {"ws", ws, 8}})) return e;
    int64_t total_frames = 0, max_frames = 0;
    for (int r = 0; r < R; ++r) {
        const int64_t* q = rows_host + 4 * (size_t)r;
        if (q[0] < 0 || q[1] < 0 || q[2] < 0 || q[3] < 0) return c->fail(-22, "vv_pcm_denoise_bias: row %d has a negative field", r);
        if (q[1] < VV_DENOISE_N || q[1] > VV_DENOISE_BIAS_MAX_N || !fits(q[0], q[1], n_x))
            return c->fail(-22, "vv_pcm_denoise_bias: row %d: a signal of %d ... %d samples inside the %lld samples of x is needed (one full frame)", r,
                           VV_DENOISE_N, VV_DENOISE_BIAS_MAX_N, (long long)n_x);
        const int64_t F = (q[1] - VV_DENOISE_N) / VV_DENOISE_H + 1;
        total_frames += F;
        if (F > max_frames) max_frames = F;
    }
    if (n_out / (VV_DENOISE_N / 2 + 1) < R)
        return c->fail(-22, "vv_pcm_denoise_bias: out of %lld doubles, %lld are needed", (long long)n_out, (long long)R * (VV_DENOISE_N / 2 + 1));
    if (int e = check_ws(c, "vv_pcm_denoise_bias", ws_bytes, vvk_pcm_denoise_bias_ws_bytes((long long)total_frames, R))) return e;
    Prof p(c, VV_PROF_ELEMWISE, (double)total_frames * 10.0 * 512.0 * 10.0, (double)total_frames * (2.0 * VV_DENOISE_N + 16.0 * (VV_DENOISE_N / 2 + 1)), st);
    KCHK(c, vvk_pcm_denoise_bias(x, (long long)n_x, (const long long*)rows, R, (long long)total_frames, (long long)max_frames, window, twiddles, out,
                                 ws, st, &m__));
    return 0;
}

// N22: the keyed audio watermark and its detector.  As with N12 ... N19 the rows come in host memory too: everything is checked before a launch.
// Accounted under the class of the denoiser, whose loop the embedder is.
uint64_t vv_pcm_watermark_ws_bytes(int R) { return vvk_pcm_watermark_ws_bytes(R); }

int vv_pcm_watermark(vv_ctx* c, const int16_t* x, int64_t n_x, const int64_t* rows, const int64_t* rows_host, int R, const int8_t* chips,
                     int64_t n_chips, double gp, double gm, const double* window, const double* twiddles, int16_t* y, int64_t n_y, void* ws,
                     uint64_t ws_bytes, void* stream) {
    if (!c) return -22;
    hipStream_t st = enter(c, stream);
    if (R < 1 || R > 65535 || n_x < 0 || n_y < 0) return c->fail(-22, "vv_pcm_watermark: bad sizes (1 <= R <= 65535)");
    if (int e = check_ptrs(c, "vv_pcm_watermark", {{"x", x, 2}, {"rows", rows, 8}, {"rows_host", rows_host}, {"chips", chips, 4}, {"window", window, 8},
                                                   {"twiddles", twiddles, 8}, {"y", y, 2}, {"ws", ws, 8}})) return e;
    if (n_chips < (int64_t)VV_WATERMARK_P * VV_WATERMARK_K)
        return c->fail(-22, "vv_pcm_watermark: chips of %lld entries, %d are needed", (long long)n_chips, VV_WATERMARK_P * VV_WATERMARK_K);
    if (!(gp >= 1.0 && gp <= 1.5 && gm >= 0.5 && gm <= 1.0)) return c->fail(-22, "vv_pcm_watermark: gains 1 <= gp <= 1.5 and 0.5 <= gm <= 1 are needed");
    if (spans_overlap(x, 2ull * n_x, y, 2ull * n_y))
        return c->fail(-22, "vv_pcm_watermark: y overlaps x (a hop reads the input under its neighbours: not in place)");
    std::vector<std::pair<int64_t, int64_t>> on_y;
    int64_t total_frames = 0, max_hops = 1, total_hops = 0;
    for (int r = 0; r < R; ++r) {
        const int64_t* q = rows_host + 4 * (size_t)r;
        if (q[0] < 0 || q[1] < 0 || q[2] < 0 || q[3] < 0) return c->fail(-22, "vv_pcm_watermark: row %d has a negative field", r);
        if (q[3] >= ((int64_t)1 << VV_WATERMARK_NB)) return c->fail(-22, "vv_pcm_watermark: row %d: a message of %d bits is needed", r, VV_WATERMARK_NB);
        if (!fits(q[0], q[1], n_x) || q[1] > ((int64_t)1 << 30))
            return c->fail(-22, "vv_pcm_watermark: row %d does not fit the %lld samples of x", r, (long long)n_x);
        if (!fits(q[2], q[1], n_y)) return c->fail(-22, "vv_pcm_watermark: row %d does not fit the %lld samples of y", r, (long long)n_y);
        const int64_t M = (q[1] + VV_DENOISE_H - 1) / VV_DENOISE_H, hops = M > 0 ? M : 1;
        if (q[1] > 0) on_y.emplace_back(q[2], q[2] + q[1]);
        total_frames += M + 3;
        total_hops += hops;
        if (hops > max_hops) max_hops = hops;
    }
    std::sort(on_y.begin(), on_y.end());
    for (size_t i = 1; i < on_y.size(); ++i)
        if (on_y[i].first < on_y[i - 1].second) return c->fail(-22, "vv_pcm_watermark: rows overlap on y");
    if (int e = check_ws(c, "vv_pcm_watermark", ws_bytes, vvk_pcm_watermark_ws_bytes(R))) return e;
    Prof p(c, VV_PROF_ELEMWISE, (double)total_hops * 8.0 * 10.0 * 512.0 * 10.0, 16.0 * (double)total_hops * VV_DENOISE_H, st);
    KCHK(c, vvk_pcm_watermark(x, (long long)n_x, (const long long*)rows, R, (long long)total_frames, (long long)max_hops, chips, gp, gm, window,
                              twiddles, y, (long long)n_y, ws, st, &m__));
    return 0;
}

uint64_t vv_pcm_watermark_detect_ws_bytes(int64_t total_frames, int R) { return vvk_pcm_watermark_detect_ws_bytes((long long)total_frames, R); }

int vv_pcm_watermark_detect(vv_ctx* c, const int16_t* x, int64_t n_x, const int64_t* rows, const int64_t* rows_host, int R, const int8_t* chips,
                            int64_t n_chips, const double* window, const double* twiddles, int64_t* stats, int64_t n_stats, int32_t* cells_out,
                            int64_t n_cells, void* ws, uint64_t ws_bytes, void* stream) {
    if (!c) return -22;
    hipStream_t st = enter(c, stream);
    if (R < 1 || R > 65535 || n_x < 0 || n_stats < 0 || n_cells < 0) return c->fail(-22, "vv_pcm_watermark_detect: bad sizes (1 <= R <= 65535)");
    if (int e = check_ptrs(c, "vv_pcm_watermark_detect", {{"x", x, 2}, {"rows", rows, 8}, {"rows_host", rows_host}, {"chips", chips, 4},
                                                          {"window", window, 8}, {"twiddles", twiddles, 8}, {"stats", stats, 8},
                                                          {"cells_out", cells_out, 4, true}, {"ws", ws, 8}})) return e;
    if (n_chips < (int64_t)VV_WATERMARK_P * VV_WATERMARK_K)
        return c->fail(-22, "vv_pcm_watermark_detect: chips of %lld entries, %d are needed", (long long)n_chips, VV_WATERMARK_P * VV_WATERMARK_K);
    int64_t total_frames = 0, max_frames = 0;
    for (int r = 0; r < R; ++r) {
        const int64_t* q = rows_host + 4 * (size_t)r;
        if (q[0] < 0 || q[1] < 0 || q[2] < 0 || q[3] < 0) return c->fail(-22, "vv_pcm_watermark_detect: row %d has a negative field", r);
        if (q[1] > VV_WATERMARK_DETECT_MAX_N || !fits(q[0], q[1], n_x))
            return c->fail(-22, "vv_pcm_watermark_detect: row %d: a signal of at most %d samples inside the %lld samples of x is needed", r,
                           VV_WATERMARK_DETECT_MAX_N, (long long)n_x);
        const int64_t F = (q[1] + VV_DENOISE_H - 1) / VV_DENOISE_H + 3;
        total_frames += F;
        if (F > max_frames) max_frames = F;
    }
    const int64_t per_row = (int64_t)VV_WATERMARK_P * VV_WATERMARK_G * VV_WATERMARK_NB * 2;
    if (n_stats / per_row < R)
        return c->fail(-22, "vv_pcm_watermark_detect: stats of %lld entries, %lld are needed", (long long)n_stats, (long long)R * per_row);
    if (cells_out && n_cells / VV_WATERMARK_K < total_frames)
        return c->fail(-22, "vv_pcm_watermark_detect: cells_out of %lld entries, %lld are needed", (long long)n_cells,
                       (long long)total_frames * VV_WATERMARK_K);
    if (int e = check_ws(c, "vv_pcm_watermark_detect", ws_bytes, vvk_pcm_watermark_detect_ws_bytes((long long)total_frames, R))) return e;
    Prof p(c, VV_PROF_ELEMWISE, (double)total_frames * (10.0 * 512.0 * 10.0 + 3.0 * VV_WATERMARK_K * VV_WATERMARK_P * VV_WATERMARK_G),
           (double)total_frames * (2.0 * VV_DENOISE_H + 24.0 * VV_WATERMARK_K) + 8.0 * (double)R * per_row, st);
    KCHK(c, vvk_pcm_watermark_detect(x, (long long)n_x, (const long long*)rows, R, (long long)total_frames, (long long)max_frames, chips, window,
                                     twiddles, (long long*)stats, (int*)cells_out, ws, st, &m__));
    return 0;
}

// N15: FLAC frames of the final PCM.  As with N12 ... N14 the rows come in host memory too: everything is checked before a launch.
uint64_t vv_flac_frame_bound(int64_t m) { return vvk_flac_frame_bound((long long)m); }

uint64_t vv_pcm_flac_ws_bytes(int64_t total_frames, int R) { return vvk_pcm_flac_ws_bytes((long long)total_frames, R); }

// both entries: lpc_order 0 = vv_pcm_flac (N15), 1 ... 12 = vv_pcm_flac_lpc (N16)
static int pcm_flac(vv_ctx* c, const char* name, const int16_t* x, int64_t n_x, const int64_t* rows, const int64_t* rows_host, int R, int sample_rate,
                    int lpc_order, uint8_t* y, int64_t n_y, int64_t* info, void* ws, uint64_t ws_bytes, void* stream) {
    hipStream_t st = enter(c, stream);
    if (R < 1 || R > 65535 || n_x < 0 || n_y < 0) return c->fail(-22, "%s: bad sizes (1 <= R <= 65535)", name);
    if (sample_rate < 1 || sample_rate > 655350) return c->fail(-22, "%s: a sample rate in 1 ... 655350 Hz is needed", name);
    if (int e = check_ptrs(c, name, {{"x", x, 2}, {"rows", rows, 8}, {"rows_host", rows_host, 8}, {"y", y}, {"info", info, 8}, {"ws", ws, 8}})) return e;
    if (spans_overlap(x, 2ull * n_x, y, (uint64_t)n_y)) return c->fail(-22, "%s: y overlaps x (a frame is packed while others are still read)", name);
    int64_t total_frames = 0, max_frames = 0, total_samples = 0;
    uint64_t need = 0;
    for (int r = 0; r < R; ++r) {
        const int64_t* q = rows_host + 4 * (size_t)r;
        if (q[0] < 0 || q[1] < 0 || q[2] < 0 || q[3] < 0) return c->fail(-22, "%s: row %d has a negative field", name, r);
        if (q[1] < 1) return c->fail(-22, "%s: row %d is empty (n >= 1)", name, r);
        if (!fits(q[0], q[1], n_x)) return c->fail(-22, "%s: row %d does not fit the %lld samples of x", name, r, (long long)n_x);
        const int64_t frames = (q[1] + VV_FLAC_BLOCK - 1) / VV_FLAC_BLOCK;
        if (!fits(q[2], frames, (int64_t)1 << 31)) return c->fail(-22, "%s: row %d: frame0 + frames exceeds 2^31", name, r);
        if (q[3] > 1 || (q[3] == 0 && q[1] % VV_FLAC_BLOCK))
            return c->fail(-22, "%s: row %d: last is 0 or 1, and last = 0 needs n to be a multiple of %d", name, r, VV_FLAC_BLOCK);
        need += (uint64_t)(frames - 1) * vvk_flac_frame_bound(VV_FLAC_BLOCK) + vvk_flac_frame_bound(q[1] - (frames - 1) * VV_FLAC_BLOCK);
        total_frames += frames;
        total_samples += q[1];
        if (frames > max_frames) max_frames = frames;
    }
    if ((uint64_t)n_y < need)
        return c->fail(-22, "%s: y of %lld bytes, the frame bounds add up to %llu", name, (long long)n_y, (unsigned long long)need);
    if (int e = check_ws(c, name, ws_bytes, lpc_order ? vvk_pcm_flac_lpc_ws_bytes((long long)total_frames, R) : vvk_pcm_flac_ws_bytes((long long)total_frames, R)))
        return e;
    Prof p(c, VV_PROF_ELEMWISE, (lpc_order ? 800.0 : 200.0) * (double)total_samples, 4.0 * (double)total_samples + 2.0 * (double)need, st);
    KCHK(c, vvk_pcm_flac(x, (long long)n_x, (const long long*)rows, R, sample_rate, lpc_order, (long long)total_frames, (long long)max_frames, y, (long long)n_y,
                         (long long*)info, ws, st, &m__));
    return 0;
}

int vv_pcm_flac(vv_ctx* c, const int16_t* x, int64_t n_x, const int64_t* rows, const int64_t* rows_host, int R, int sample_rate, uint8_t* y,
                int64_t n_y, int64_t* info, void* ws, uint64_t ws_bytes, void* stream) {
    if (!c) return -22;
    return pcm_flac(c, "vv_pcm_flac", x, n_x, rows, rows_host, R, sample_rate, 0, y, n_y, info, ws, ws_bytes, stream);
}

// N16: the same with LPC subframes of order 1 ... lpc_order among the candidates; the workspace also holds the frames' predictors
uint64_t vv_pcm_flac_lpc_ws_bytes(int64_t total_frames, int R, int lpc_order) {
    return lpc_order < 1 || lpc_order > VV_FLAC_MAX_LPC_ORDER ? 0 : vvk_pcm_flac_lpc_ws_bytes((long long)total_frames, R);
}

int vv_pcm_flac_lpc(vv_ctx* c, const int16_t* x, int64_t n_x, const int64_t* rows, const int64_t* rows_host, int R, int sample_rate, int lpc_order,
                    uint8_t* y, int64_t n_y, int64_t* info, void* ws, uint64_t ws_bytes, void* stream) {
    if (!c) return -22;
    if (lpc_order < 1 || lpc_order > VV_FLAC_MAX_LPC_ORDER)
        return c->fail(-22, "vv_pcm_flac_lpc: lpc_order in 1 ... %d is needed (vv_pcm_flac is the encoder without LPC)", VV_FLAC_MAX_LPC_ORDER);
    return pcm_flac(c, "vv_pcm_flac_lpc", x, n_x, rows, rows_host, R, sample_rate, lpc_order, y, n_y, info, ws, ws_bytes, stream);
}

// N17: FLAC input.  The rows come in host memory too: everything the host can see is checked before a launch; a refused call launches
// nothing.  What the bytes of the streams say is the kernels' business (csrc/vv_flac_decode.hip: every read bounded).
uint64_t vv_flac_decode_frame_bound(int block, int channels, int bits) {
    return bits != 8 && bits != 16 && bits != 24 ? 0 : vvk_flac_decode_frame_bound(block, channels, bits);
}

uint64_t vv_flac_index_ws_bytes(int64_t n_bytes, int R) { return vvk_flac_index_ws_bytes((long long)n_bytes, R); }

uint64_t vv_flac_decode_ws_bytes(int64_t plane_samples, int64_t total_frames) { return vvk_flac_decode_ws_bytes((long long)plane_samples, (long long)total_frames); }

int vv_flac_index(vv_ctx* c, const uint8_t* data, int64_t n_bytes, const int64_t* rows, const int64_t* rows_host, int R, int64_t* info, void* ws,
                  uint64_t ws_bytes, void* stream) {
    if (!c) return -22;
    hipStream_t st = enter(c, stream);
    int maxch = 1;
    if (int e = flac_rows(c, "vv_flac_index", rows, rows_host, R, n_bytes, &maxch)) return e;
    if (int e = check_ptrs(c, "vv_flac_index", {{"data", data, 8}, {"info", info, 8}, {"ws", ws, 8}})) return e;
    if (int e = check_ws(c, "vv_flac_index", ws_bytes, vvk_flac_index_ws_bytes((long long)n_bytes, R))) return e;
    if (spans_overlap(data, (uint64_t)n_bytes, ws, ws_bytes) || spans_overlap(info, 32ull * R, ws, ws_bytes) || spans_overlap(data, (uint64_t)n_bytes, info, 32ull * R))
        return c->fail(-22, "vv_flac_index: data, info and ws overlap");
    Prof p(c, VV_PROF_ELEMWISE, 0, 4.0 * (double)n_bytes, st);
    KCHK(c, vvk_flac_index(data, (long long)n_bytes, (const long long*)rows, R, (long long*)info, ws, st, &m__));
    return 0;
}

int vv_flac_decode(vv_ctx* c, const uint8_t* data, int64_t n_bytes, const int64_t* rows, const int64_t* rows_host, int R, const int64_t* lay,
                   const int64_t* lay_host, const void* ws, uint64_t ws_bytes, uint8_t* pcm, int64_t n_pcm, int64_t* info2, void* ws2, uint64_t ws2_bytes,
                   void* stream) {
    if (!c) return -22;
    hipStream_t st = enter(c, stream);
    int maxch = 1;
    if (int e = flac_rows(c, "vv_flac_decode", rows, rows_host, R, n_bytes, &maxch)) return e;
    if (n_pcm < 0) return c->fail(-22, "vv_flac_decode: bad sizes (n_pcm >= 0)");
    if (int e = check_ptrs(c, "vv_flac_decode", {{"data", data, 8}, {"lay", lay, 8}, {"lay_host", lay_host, 8}, {"ws", ws, 8}, {"pcm", pcm},
                                                 {"info2", info2, 8}, {"ws2", ws2, 8}})) return e;
    int64_t F = 0, S = 0, P = 0, at = 0;
    for (int r = 0; r < R; ++r) {
        const int64_t* l = lay_host + 6 * (size_t)r;
        const int64_t* q = rows_host + 8 * (size_t)r;
        const int64_t width = q[3] == 24 ? 4 : q[3] / 8;
        if (l[1] < 0 || l[2] < 0 || l[2] > VV_FLAC_MAX_CLIP || l[1] > l[2] || l[1] > q[1] || l[3] != F || l[4] != P || l[5] != S)
            return c->fail(-22, "vv_flac_decode: lay row %d: frames <= samples <= 2^26 and the three prefix sums are needed", r);
        const int64_t bytes = l[2] * q[2] * width;
        if (l[0] < at || !fits(l[0], bytes, n_pcm)) return c->fail(-22, "vv_flac_decode: lay row %d does not fit the %lld bytes of pcm, in ascending order", r, (long long)n_pcm);
        at = l[0] + bytes;
        F += l[1]; S += l[2]; P += l[2] * q[2];
    }
    if (int e = check_ws(c, "vv_flac_decode", ws_bytes, vvk_flac_index_ws_bytes((long long)n_bytes, R))) return e;
    if (int e = check_ws(c, "vv_flac_decode", ws2_bytes, vvk_flac_decode_ws_bytes((long long)P, (long long)F), "ws2")) return e;
    const void* span[5] = {data, ws, pcm, info2, ws2};
    const uint64_t len[5] = {(uint64_t)n_bytes, ws_bytes, (uint64_t)n_pcm, 16ull * R, ws2_bytes};
    for (int i = 0; i < 5; ++i)
        for (int j = i + 1; j < 5; ++j)
            if (len[i] && len[j] && spans_overlap(span[i], len[i], span[j], len[j])) return c->fail(-22, "vv_flac_decode: data, ws, pcm, info2 and ws2 overlap");
    Prof p(c, VV_PROF_ELEMWISE, 40.0 * (double)P, 2.0 * (double)n_bytes + 8.0 * (double)P + (double)n_pcm, st);
    KCHK(c, vvk_flac_decode(data, (long long)n_bytes, (const long long*)rows, R, (const long long*)lay, (long long)F, (long long)S, (long long)P, maxch,
                            (void*)ws, pcm, (long long)n_pcm, (long long*)info2, ws2, st, &m__));
    return 0;
}

// N25: IMA ADPCM blocks of the final PCM; IMA ADPCM and G.711 clips into the PCM vv_ingest_pcm reads.  The rows come in host memory too.
int vv_pcm_adpcm(vv_ctx* c, const int16_t* x, int64_t n_x, const int64_t* rows, const int64_t* rows_host, int R, int spb, uint8_t* y, int64_t n_y,
                 void* stream) {
    if (!c) return -22;
    hipStream_t st = enter(c, stream);
    if (R < 1 || R > 65535 || n_x < 0 || n_y < 0) return c->fail(-22, "vv_pcm_adpcm: bad sizes (1 <= R <= 65535)");
    if (spb < 9 || (spb - 1) % 8 || (spb - 1) / 2 + 4 > VV_ADPCM_MAX_BLOCK_ALIGN)
        return c->fail(-22, "vv_pcm_adpcm: samples_per_block is 8 k + 1 in 9 ... %d", (VV_ADPCM_MAX_BLOCK_ALIGN - 4) * 2 + 1);
    if (int e = check_ptrs(c, "vv_pcm_adpcm", {{"x", x, 2}, {"rows", rows, 8}, {"rows_host", rows_host, 8}, {"y", y, 8}})) return e;
    if (spans_overlap(x, 2ull * n_x, y, (uint64_t)n_y)) return c->fail(-22, "vv_pcm_adpcm: y overlaps x");
    const int64_t ba = (spb - 1) / 2 + 4;
    int64_t max_blocks = 0, total = 0, at = 0;
    for (int r = 0; r < R; ++r) {
        const int64_t* q = rows_host + 3 * (size_t)r;
        if (q[1] < 1 || !fits(q[0], q[1], n_x)) return c->fail(-22, "vv_pcm_adpcm: row %d does not fit the %lld samples of x (n >= 1)", r, (long long)n_x);
        const int64_t blocks = (q[1] + spb - 1) / spb;
        if (q[2] < 0 || q[2] % 4 || q[2] > n_y || blocks > (n_y - q[2]) / ba)
            return c->fail(-22, "vv_pcm_adpcm: row %d: %lld blocks of %lld bytes at dst_off %lld (a multiple of 4) do not fit the %lld bytes of y", r,
                           (long long)blocks, (long long)ba, (long long)q[2], (long long)n_y);
        if (q[2] < at) return c->fail(-22, "vv_pcm_adpcm: row %d: the rows' blocks lie in ascending order on y, disjoint", r);
        at = q[2] + blocks * ba;
        if (blocks > max_blocks) max_blocks = blocks;
        total += q[1];
    }
    Prof p(c, VV_PROF_ELEMWISE, 40.0 * 90.0 * (double)total, 2.5 * (double)total, st);
    KCHK(c, vvk_pcm_adpcm(x, (long long)n_x, (const long long*)rows, R, spb, (long long)max_blocks, y, (long long)n_y, st, &m__));
    return 0;
}

int vv_wav_decode(vv_ctx* c, const uint8_t* data, int64_t n_bytes, const int64_t* rows, const int64_t* rows_host, int R, uint8_t* pcm, int64_t n_pcm,
                  int64_t* status, void* stream) {
    if (!c) return -22;
    hipStream_t st = enter(c, stream);
    if (R < 1 || R > 65535 || n_bytes < 0 || n_pcm < 0) return c->fail(-22, "vv_wav_decode: bad sizes (1 <= R <= 65535)");
    if (int e = check_ptrs(c, "vv_wav_decode", {{"data", data, 16}, {"rows", rows, 8}, {"rows_host", rows_host, 8}, {"pcm", pcm, 16}, {"status", status, 8}}))
        return e;
    int64_t at = 0, max_heads = 0, max_codes = 0, samples = 0;
    for (int r = 0; r < R; ++r) {
        const int64_t* q = rows_host + 8 * (size_t)r;
        const int64_t tag = q[2], ch = q[3], ba = q[4], frames = q[5];
        if (q[0] % 16 || !fits(q[0], q[1], n_bytes)) return c->fail(-22, "vv_wav_decode: row %d: a clip at a 16-byte aligned offset inside data is needed", r);
        if (ch < 1 || ch > 65535 || frames < 0) return c->fail(-22, "vv_wav_decode: row %d: channels in 1 ... 65535 and frames >= 0 are needed", r);
        int64_t holds = 0;
        if (tag == VV_WAVE_TAG_ADPCM) {
            if (ch > 2 || ba < 8 * ch || ba % (4 * ch) || ba > 65535)
                return c->fail(-22, "vv_wav_decode: row %d: IMA ADPCM has 1 or 2 channels and a block alignment that is a multiple of 4 x channels, at least 8 x channels", r);
            const int64_t rem = q[1] % ba;
            if (rem >= 4 * ch) {
                const int64_t m = (rem - 4 * ch) % (4 * ch) - 4 * (ch - 1);
                holds = 1 + 8 * ((rem - 4 * ch) / (4 * ch)) + 2 * (m > 0 ? m : 0);
            }
            holds += q[1] / ba * ((ba / ch - 4) * 2 + 1);
            const int64_t heads = (q[1] / ba + (rem >= 4 * ch ? 1 : 0)) * ch;
            if (heads > max_heads) max_heads = heads;
        } else if (tag == VV_WAVE_TAG_ALAW || tag == VV_WAVE_TAG_ULAW) {
            holds = q[1] / ch;
            if (frames * ch > max_codes) max_codes = frames * ch;
        } else {
            return c->fail(-22, "vv_wav_decode: row %d: format tag %lld (6, 7 and 17 are decoded)", r, (long long)tag);
        }
        if (frames > holds) return c->fail(-22, "vv_wav_decode: row %d: %lld frames, the bytes hold %lld", r, (long long)frames, (long long)holds);
        if (q[6] < at || q[6] % 16 || q[6] > n_pcm || frames > (n_pcm - q[6]) / (2 * ch))
            return c->fail(-22, "vv_wav_decode: row %d does not fit the %lld bytes of pcm, 16-byte aligned, in ascending order", r, (long long)n_pcm);
        at = q[6] + frames * ch * 2;
        samples += frames * ch;
    }
    if (spans_overlap(data, (uint64_t)n_bytes, pcm, (uint64_t)n_pcm) || spans_overlap(status, 16ull * R, pcm, (uint64_t)n_pcm) ||
        spans_overlap(status, 16ull * R, data, (uint64_t)n_bytes))
        return c->fail(-22, "vv_wav_decode: data, pcm and status overlap");
    Prof p(c, VV_PROF_ELEMWISE, 20.0 * (double)samples, (double)n_bytes + 2.0 * (double)samples, st);
    KCHK(c, vvk_wav_decode(data, (long long)n_bytes, (const long long*)rows, R, (long long)max_heads, (long long)max_codes, pcm, (long long)n_pcm,
                           (long long*)status, st, &m__));
    return 0;
}

// --------------------------------------------------------------------------- transformer steps
// The stage in four parts: the call (StepsCall), the lane plan (lane_plan: host values in, sizes out; lane_bufs names the buffers), the
// launches of one lane (StepsRun) and the schedule (steps_schedule: order, streams, forks and joins); transformer_steps runs them.
// LANES (round 4): a batch of independent items may run as TWO half batches ("lanes") on two HIP streams at once -- lane 0 on the
// caller's stream, lane 1 on a context-owned side stream forked from it and joined back before the call returns.  Every kernel of
// the path is row- or sequence-local with one arithmetic whatever the launch size (tests/test_mixed256_gpu.py), so the lanes produce
// exactly the bits of the whole batch; what changes is the schedule: the partial last round of one lane's persistent GEMM (1,600 tiles
// on 256 CUs = 6.25 rounds at the headline shape), the tails of its other kernels and the launch gaps of small batches are filled by
// the other lane's kernels instead of idling: -1.3 % of the step at B = 32, -3 % at 24, -5.5 % at 16 and 8, -9 % at 4
// (profiles/r04/lanes_notes.md; three and four lanes, unequal cuts and CU-masked streams measured slower).  A lane is a complete
// sub-problem: its own packed rows, row tables and buffers; the cut is the item boundary closest to half of the rows.
namespace {
constexpr size_t VV_LANE_MIN_ROWS = 1024;     // "lanes" auto: at ~600 packed rows the step is bound by the launch rate and a second stream of launches
                                              // costs ~1 % (profiles/r04/lanes_notes.md); from 1,200 rows on two lanes win at every size measured
struct Lane {
    int B = 0, b0 = 0;
    int n_seq = 0;                     // sequences the block kernels of this lane (or branch view) run on: 2 B, or B for one CFG branch
    size_t Rc = 0, R = 0, n_tab = 0, tail_rows = 0;
    double sum_sq = 0;                 // sum of len^2 over those sequences (attention flops)
    bool uniform = true, pending = false;
    int tail_row0 = 0, tp_o = 0, tp_f = 0;
    const int32_t* seq_len = nullptr;
    float* x = nullptr;
    const float *cat = nullptr, *cat_drop = nullptr;
    hipStream_t st = nullptr;
    char *xcat = nullptr, *h = nullptr, *h2 = nullptr, *h3 = nullptr, *qkv = nullptr, *att = nullptr, *ffm = nullptr;
    float *xres = nullptr, *pred = nullptr, *csq = nullptr, *csk = nullptr, *csq_rows = nullptr, *csk_rows = nullptr, *h2_tail = nullptr, *h3_tail = nullptr;
    float *xs = nullptr, *kbuf[3] = {};     // N7 (more than one stage): the stage state and the stored slopes, [Rc][n_mel] fp32 each
    int *kv_len = nullptr, *tab = nullptr;
    const int *row_start = nullptr, *row_src = nullptr, *row_pos = nullptr, *qkv_pos = nullptr;
    // N8 (a call with a guidance mask): the tables of the evaluation's guided subset, rebuilt when the subset changes (guided_tables_kernel)
    int *g_row_start = nullptr, *g_rs_rel = nullptr, *g_kv_len = nullptr, *g_row_pos = nullptr, *u_src = nullptr, *u_crow = nullptr, *u_row = nullptr;
    // N11 (a call with APG): the partial sums [B][n_tiles][3] and the coefficients [B][2] of the evaluation in hand, and a second stage state:
    // stage i reads the state it was evaluated at (x_e) while it writes the next one
    double* apg_part = nullptr;
    float *apg_coef = nullptr, *xs2 = nullptr;
    // N20 (a multistep plan): the ring of kept slopes, f_m in slot m % ms_ring(c), [Rc][n_mel] fp32 each; the report's partial sums [B][n_tiles][2]
    float* hist[3] = {};
    double* rep_part = nullptr;
    // N21 (a call that reuses guidance differences): the lane's stored D = p_c - p_u, [Rc][n_mel] fp32; the drift report's partial sums [B][n_tiles][2]
    float* d_buf = nullptr;
    double* drift_part = nullptr;
    // N23 (a call that caches a span of blocks): the stored contribution of the span, [R][D] fp32 (a second plane with a report: the stores
    // alternate); the report's partial sums [2B][n_tiles][2]
    float* bc_buf[2] = {};
    double* bc_part = nullptr;
    // N24 (a call with CFG-Zero* / rescale): the Gram sums [B][n_tiles][5] and the coefficients [B][2] of the evaluation in hand
    double* cn_part = nullptr;
    float* cn_coef = nullptr;
};
// N20: slots of the slope ring.  q - 1 without a report: the fresh slope takes the slot of the oldest one the step reads.  With a report
// one more (two at the least), so that f_{n-1} outlives the stage launch of step n.
inline int ms_ring(const vv_ctx* c) { return !c->ms_q ? 0 : c->ode_report ? std::max(c->ms_q, 2) : c->ms_q - 1; }
// N8: what the host knows of a lane's guided subset at the evaluation in hand
struct GuideState {
    std::vector<uint8_t> flags;        // [B] of the lane; empty = no tables built yet in this call
    size_t Ru = 0;                     // unconditional rows: the guided items' lengths
    int Bu = 0;                        // guided items
    double sum_sq = 0;                 // sum of len^2 over them
};

// One call of the stage, as every entry hands it over.
// guide != nullptr (N8, vv_transformer_steps_guided): HOST flags [evaluations of the plan][ld_guide], guided(b, e) at guide[e * ld_guide + b];
// an item that is not guided at an evaluation has no unconditional rows there.
// apg != nullptr (N11, vv_transformer_steps_apg): the projected combine -- per evaluation and lane, apg_reduce_kernel and apg_coef_kernel in
// front of the stage kernel, on its stream.
// ws_form, named by a size query: the workspace of a plain call, with the tables of a mask's subsets on top (whatever the mask), or with
// APG's on top of those (with or without a mask).  A call with a mask or with APG implies its form.
// N21: WS_REUSE / WS_REUSE_REPORT = the guided form plus a D buffer per lane, and the drift report's partial sums.
// N23: WS_CACHED / WS_CACHED_REPORT = the plain form plus a plane per lane, and with a report a second plane and the partial sums.
// N24: WS_NORM = the guided form plus the Gram sums and the coefficients per lane.
enum WsForm { WS_PLAIN, WS_GUIDED, WS_APG, WS_REUSE, WS_REUSE_REPORT, WS_CACHED, WS_CACHED_REPORT, WS_NORM };
struct StepsCall {
    vv_steps_args a{};
    const uint8_t* guide = nullptr; int ld_guide = 0;
    const vv_apg_args* apg = nullptr;
    // N21 (vv_transformer_steps_reuse): the mask may hold a 2 = "guided, the stored difference reused"; reuse->report asks for the drift report
    bool reuse_entry = false; const vv_reuse_args* reuse = nullptr;
    WsForm ws_form = WS_PLAIN;
    uint64_t* ws_only = nullptr;       // a size query: only the workspace bytes of the call (nothing is launched; the data pointers may be null)
    bool guided = false, with_apg = false, rk = false;     // derived once, by transformer_steps
    // N21, derived by transformer_steps: a D buffer is needed (the mask has a 2, or a report is asked for) / the report is on, and per
    // evaluation of the call and item [(e - step0 * s) * B + b] the stage kernel's mode (VV_REUSE_LOAD | VV_REUSE_STORE) and "a D of this
    // call is stored" in front of evaluation e
    bool with_reuse = false, with_drift = false;
    std::vector<uint8_t> ru_mode, ru_old;
    // N23 (vv_transformer_steps_cached): the span and the modes of the plan's evaluations; derived by transformer_steps: a plane is needed
    // (a mode other than 0, or a report) / the report is on
    const vv_block_cache_args* bc = nullptr;
    bool with_cache = false, with_cache_report = false;
    // N24 (vv_transformer_steps_norm): the optimised scale and the rescale per item; a call without a mask runs on one of ones (every item
    // guided everywhere: the guided form's tables give the stage kernel its u_row)
    const vv_cfg_norm_args* norm = nullptr;
    bool with_norm = false;
    std::vector<uint8_t> all_guided;
};
struct StepDims { int D, FF, M, CD, es, KP, MP; };

// The lane plan, from host values alone.  Option "lanes" 1 = one lane, 2 = two whenever there are two to make, 0 (default) = two when
// both halves still fill the persistent GEMM for several rounds (bf16, >= VV_LANE_MIN_ROWS packed rows in all).  Two items or more: ITEM
// lanes, cut at the item boundary closest to half of the rows.  One problem only (a single item, or a batch under the row threshold with
// "lanes" 2): its two CFG BRANCHES are the lanes -- the conditional rows [0, Rc) and the unconditional rows [Rc, 2 Rc) of the same packed
// buffers are independent from the conditioning pack at the top of a step to the CFG combine at its end, so the side stream is forked
// and joined once per step around them.
struct LanePlan { int n_lanes = 1, cut = 0; bool branch_lanes = false; Lane lanes[2]; };
LanePlan lane_plan(const vv_ctx* c, const StepDims& d, const std::vector<int>& hlen, int N) {
    LanePlan P;
    const int B = (int)hlen.size();
    const bool tails = c->split_k_tail && c->dt == VV_DTYPE_BF16;
    size_t Rc_all = 0;
    for (int v : hlen) Rc_all += v;
    const bool two = c->lanes == 2 || (c->lanes == 0 && c->dt == VV_DTYPE_BF16 && 2 * Rc_all >= (size_t)VV_LANE_MIN_ROWS);
    if (two && B >= 2) {
        size_t acc = 0, best = (size_t)-1;
        for (int b = 1; b < B; ++b) {
            acc += hlen[b - 1];
            const size_t dist = acc * 2 > Rc_all ? acc * 2 - Rc_all : Rc_all - acc * 2;
            if (dist < best) { best = dist; P.cut = b; }
        }
        P.n_lanes = 2;
    }
    P.branch_lanes = two && P.n_lanes == 1 && !tails;
    const int cuts[3] = {0, P.n_lanes == 2 ? P.cut : B, B};
    for (int li = 0; li < P.n_lanes; ++li) {
        Lane& L = P.lanes[li];
        L.b0 = cuts[li]; L.B = cuts[li + 1] - cuts[li];
        for (int b = L.b0; b < L.b0 + L.B; ++b) { L.Rc += hlen[b]; L.sum_sq += 2.0 * hlen[b] * hlen[b]; L.uniform = L.uniform && hlen[b] == N; }
        L.R = 2 * L.Rc; L.n_seq = 2 * L.B;
        // split-K tails of the two N = D gate-store GEMMs (out-proj K = D, FF2 K = FF): same row0 (it depends on M and N only)
        if (tails) {
            int r0o = 0, r0f = 0;
            if (c->split_k_tail == 1) vvk_gemm_tail_plan((int)L.R, d.D, d.D, d.D, d.D, d.D, &r0o, &L.tp_o);     // (M, N, K, lda, ldw, ldc) of the launches
            vvk_gemm_tail_plan((int)L.R, d.D, d.FF, d.FF, d.FF, d.D, &r0f, &L.tp_f);
            if (L.tp_o && L.tp_f && r0o != r0f) L.tp_o = L.tp_f = 0;   // cannot happen (row0 is a function of M, N and the CU count); refuse rather than mix
            L.tail_row0 = L.tp_o ? r0o : r0f;
        }
        L.tail_rows = (L.tp_o || L.tp_f) ? L.R - L.tail_row0 : 0;
        L.n_tab = 2 * (size_t)L.B + L.Rc + L.R;          // row_start[2B] | row_src[Rc] | row_pos[R]
    }
    return P;
}

// workspace of one lane (its B, Rc, R, n_tab and tail plan are set): buffers that only an option uses (csq_rows / csk_rows) and the
// zero-length tails are taken all the same, so the bytes depend on the shapes, the tail plan and the ODE plan alone
void lane_bufs(Arena& a, Lane& L, const vv_ctx* c, const StepDims& d, int N, bool guided, bool apg, bool reuse, bool drift, bool cache, bool cache_report,
               bool norm) {
    const size_t R = L.R, es = d.es, D = d.D, FF = d.FF, M = d.M, KP = d.KP, MP = d.MP;
    L.xcat = a.take<char>(es * R * KP);
    L.h = a.take<char>(es * R * D); L.h2 = a.take<char>(es * R * D); L.h3 = a.take<char>(es * R * D);
    L.xres = a.take<float>(R * D);
    L.qkv = a.take<char>(es * R * 3 * D); L.att = a.take<char>(es * R * D); L.ffm = a.take<char>(es * R * FF);
    L.pred = a.take<float>(R * MP); L.kv_len = a.take<int>(2 * L.B);
    L.csq = a.take<float>((size_t)N * 64); L.csk = a.take<float>((size_t)N * 64);
    L.tab = a.take<int>(L.n_tab);                  // row_start[2B] | row_src[Rc] | row_pos[R]
    L.row_start = L.tab; L.row_src = L.tab + 2 * L.B; L.row_pos = L.row_src + L.Rc;
    L.qkv_pos = L.uniform ? nullptr : L.row_pos;   // every sequence N rows: position = packed row mod N, no table lookup
    L.csq_rows = a.take<float>(R * 64); L.csk_rows = a.take<float>(R * 64);     // compact rope tables gathered per packed row, once per call
    L.h2_tail = a.take<float>(L.tail_rows * D * (L.tp_o > 1 ? L.tp_o : 0));     // fp32 [parts][tail_rows][D] K parts of the tail rows' deltas
    L.h3_tail = a.take<float>(L.tail_rows * D * (L.tp_f > 1 ? L.tp_f : 0));
    if (c->ode_s > 1) {                            // N7: the stage state and the stored slopes
        L.xs = a.take<float>(L.Rc * M);
        for (int k = 0; k < c->ode_nk; ++k) L.kbuf[k] = a.take<float>(L.Rc * M);
    }
    for (int k = 0; k < ms_ring(c); ++k) L.hist[k] = a.take<float>(L.Rc * M);        // N20: beside the stage buffers (ode_s is 1 here)
    if (c->ms_q && c->ode_report) L.rep_part = a.take<double>((size_t)L.B * ((N + VV_APG_TILE - 1) / VV_APG_TILE) * 2);
    if (guided) {                                  // N8: row_start[2B] | rs_rel[B] | kv_len[2B] | row_pos[2 Rc] | u_src[Rc] | u_crow[Rc] | u_row[Rc]
        int* t = a.take<int>(5 * (size_t)L.B + 5 * L.Rc);
        L.g_row_start = t; L.g_rs_rel = t + 2 * L.B; L.g_kv_len = t + 3 * L.B; L.g_row_pos = t + 5 * L.B;
        L.u_src = L.g_row_pos + 2 * L.Rc; L.u_crow = L.u_src + L.Rc; L.u_row = L.u_crow + L.Rc;
    }
    if (apg) {                                     // N11
        L.apg_part = a.take<double>((size_t)L.B * ((N + VV_APG_TILE - 1) / VV_APG_TILE) * 3);
        L.apg_coef = a.take<float>(2 * (size_t)L.B);
        if (c->ode_s > 1) L.xs2 = a.take<float>(L.Rc * M);
    }
    if (reuse) L.d_buf = a.take<float>(L.Rc * M);  // N21: behind everything the guided form takes, so that form's offsets stay as they are
    if (drift) L.drift_part = a.take<double>((size_t)L.B * ((N + VV_APG_TILE - 1) / VV_APG_TILE) * 2);
    if (cache) L.bc_buf[0] = a.take<float>(R * D);  // N23: behind everything the other forms take, so their offsets stay as they are
    if (cache_report) {
        L.bc_buf[1] = a.take<float>(R * D);
        L.bc_part = a.take<double>(2 * (size_t)L.B * ((N + VV_APG_TILE - 1) / VV_APG_TILE) * 2);
    }
    if (norm) {                                    // N24: behind everything the other forms take, so their offsets stay as they are
        L.cn_part = a.take<double>((size_t)L.B * ((N + VV_APG_TILE - 1) / VV_APG_TILE) * 5);
        L.cn_coef = a.take<float>(2 * (size_t)L.B);
    }
}

// The launches of one call, lane by lane: every member fills the arguments of its kernels for the Lane (or view of one) it is given and
// launches them on that Lane's stream.  None records or waits on an event or picks a stream: that is steps_schedule's.
struct StepsRun : StepDims {
    vv_ctx* c; const vv_model_cfg& g;
    const StepsCall& q; const std::vector<int>& hlen; const LanePlan& P;
    const int N, ns, S;                // S: rows of the modulation tables (evaluations)
    // bf16: the query side of the rope moves from the QKV GEMM's epilogue into the attention kernel's Q load (option "rope_q_attn",
    // default on; profiles/r04/attention_notes.md); the fp32 (numerics) path keeps all of it in the GEMM
    const float rope_theta; const int q_rope_attn;     // rope_theta > 0, computed rope: both q and k in the GEMM epilogue, scale in attention
    StepsRun(vv_ctx* c_, const StepDims& d, const StepsCall& q_, const std::vector<int>& hlen_, const LanePlan& P_)
        : StepDims(d), c(c_), g(c_->cfg), q(q_), hlen(hlen_), P(P_), N(q_.a.N), ns(c_->ode_s), S(c_->n_steps * c_->ode_s),
          rope_theta(c_->dt == VV_DTYPE_BF16 ? c_->rope_theta : 0.f),
          q_rope_attn((c_->rope_q_attn && c_->dt == VV_DTYPE_BF16 && !(rope_theta > 0.f)) ? 1 : 0) {}
    // once per call and lane: the row tables, the compact rope tables and (no mask) the first conditioning pack, every column
    int setup(Lane& L) const {
        // kv_len: the clamped lengths of the tables, both branches -- what attention and posconv run on (never the raw device lengths)
        KCHK(c, vvk_row_tables(L.seq_len, L.B, N, (int)L.Rc, L.tab, L.tab + 2 * L.B, L.tab + 2 * L.B + L.Rc, L.kv_len, L.st, &m__));
        KCHK(c, vvk_rope_compact(q.a.rope_cos_q, q.a.rope_sin_q, L.csq, N, L.st, &m__));
        KCHK(c, vvk_rope_compact(q.a.rope_cos_k, q.a.rope_sin_k, L.csk, N, L.st, &m__));
        if (q.guide) return 0;                            // N8: the row-gathered rope tables and the pack follow the evaluation's subset (guide_eval)
        if (c->rope_rows) {
            KCHK(c, vvk_rope_rows(L.csq, L.row_pos, L.csq_rows, (int)L.R, L.st, &m__));
            KCHK(c, vvk_rope_rows(L.csk, L.row_pos, L.csk_rows, (int)L.R, L.st, &m__));
        }
        Prof p(c, VV_PROF_ELEMWISE, 0, 4.0 * L.R * (M + CD) / 2 + (double)es * L.R * KP, L.st);
        KCHK(c, vvk_pack_cat(c->dt, L.x, L.cat, L.cat_drop, L.xcat, KP, (int)L.Rc, M, CD, 0, L.row_src, L.st, &m__));
        return 0;
    }
    // the state stage i >= 1 is evaluated at: under APG the stages alternate between two buffers (stage i - 1 wrote it, stage i reads it as x_e
    // while it writes the other one)
    float* stage_state(const Lane& L, int i) const { return (q.apg && !(i & 1)) ? L.xs2 : L.xs; }
    // the conditioning pack of stage i of step s (setup packed the call's first evaluation): the n_mel state columns, read from x or,
    // for a stage i > 0, from the stage state (packed rows, no row map)
    int pack(Lane& L, GuideState& G, int s, int i) const {
        if (q.guide) return guide_eval(L, G, i, s * ns + i);
        if (s == q.a.step0 && i == 0) return 0;
        Prof p(c, VV_PROF_ELEMWISE, 0, 4.0 * L.Rc * M + 2.0 * es * L.Rc * M, L.st);
        KCHK(c, vvk_pack_cat(c->dt, i ? stage_state(L, i) : L.x, L.cat, L.cat_drop, L.xcat, KP, (int)L.Rc, M, CD, 1, i ? nullptr : L.row_src, L.st, &m__));
        return 0;
    }
    // N8: evaluation e of a call with a mask -- the lane's guided subset, its tables when the subset differs from the previous evaluation's
    // (always at the call's first), and the pack: every column of the rows whose content moved (all rows at the call's first evaluation,
    // the unconditional rows after a change of subset), else the n_mel state columns alone, as the plain pack
    int guide_eval(Lane& L, GuideState& G, int i, int e) const {
        const uint8_t* row = q.guide + (size_t)e * q.ld_guide + L.b0;
        std::vector<uint8_t> f(L.B);
        size_t Ru = 0; int Bu = 0; double sq = 0;
        for (int b = 0; b < L.B; ++b) {
            f[b] = q.with_reuse ? row[b] == 1 : row[b] != 0;      // N21: only a COMPUTED item has unconditional rows; a reusing one is as an unguided one here
            if (f[b]) { Ru += hlen[L.b0 + b]; ++Bu; sq += (double)hlen[L.b0 + b] * hlen[L.b0 + b]; }
        }
        const bool first = G.flags.empty(), changed = first || f != G.flags;
        if (changed) {
            KCHK(c, vvk_guided_tables(L.seq_len, f.data(), L.B, N, (int)L.Rc, (int)Ru, L.g_row_start, L.g_rs_rel, L.g_kv_len, L.g_row_pos, L.u_src,
                                      L.u_crow, L.u_row, L.st, &m__));
            if (c->rope_rows) {
                KCHK(c, vvk_rope_rows(L.csq, L.g_row_pos, L.csq_rows, (int)(L.Rc + Ru), L.st, &m__));
                KCHK(c, vvk_rope_rows(L.csk, L.g_row_pos, L.csk_rows, (int)(L.Rc + Ru), L.st, &m__));
            }
            G.flags = f; G.Ru = Ru; G.Bu = Bu; G.sum_sq = sq;
        }
        const float* xin = i ? stage_state(L, i) : L.x;
        const int Rc = (int)L.Rc, R = (int)(L.Rc + Ru);
        auto rows = [&](int row0, int n_rows, int only_x) -> int {
            Prof p(c, VV_PROF_ELEMWISE, 0, only_x ? (4.0 + es) * n_rows * M : 4.0 * n_rows * (M + CD) + (double)es * n_rows * KP, L.st);
            KCHK(c, vvk_pack_cat_guided(c->dt, xin, L.cat, L.cat_drop, L.xcat, KP, Rc, row0, n_rows, M, CD, only_x, i ? 1 : 0, L.row_src, L.u_src,
                                        L.u_crow, L.st, &m__));
            return 0;
        };
        if (first || !changed) return rows(0, R, first ? 0 : 1);
        if (int r = rows(0, Rc, 1)) return r;
        return Ru ? rows(Rc, (int)Ru, 0) : 0;
    }
    // input embedding: proj, then conv position embedding (two grouped convs + Mish) + residual
    int step_head(Lane& L) const {
        const size_t R = L.R;
        Gemm proj = gemm_args(c, c->dt, c->dt, VV_EPI_STORE, VV_ACT_NONE_, L.xcat, KP, "input.proj.weight", KP, "input.proj.bias", L.h, D, (int)R, D, KP);
        if (int r = launch_gemm(c, proj, VV_PROF_GEMM, L.st, 2.0 * R * D * (M + CD))) return r;
        for (int j = 1; j <= 2; ++j) {
            vv_posconv_args a{};
            a.dtype = c->dt; a.out_dtype = (j == 1) ? c->dt : VV_DTYPE_F32; a.in = (j == 1) ? L.h : L.h2; a.ld_in = D;
            const std::string wn = "input.pos_conv" + std::to_string(j) + ".weight", bn = "input.pos_conv" + std::to_string(j) + ".bias";
            a.W = c->W(wn); a.bias = c->Wf(bn);
            a.out = (j == 1) ? (void*)L.h2 : (void*)L.xres; a.ld_out = D;
            a.resid = (j == 2) ? L.h : nullptr; a.ld_resid = D;
            a.n_seq = L.n_seq; a.seq_n = N; a.groups = g.pos_conv_groups; a.KW = g.pos_conv_k; a.B = L.n_seq; a.seq_len = L.kv_len; a.row_start = L.row_start;
            Prof p(c, VV_PROF_POSCONV, 2.0 * R * D * 64 * g.pos_conv_k, (double)es * R * D * 2 + (j == 2 ? 4.0 * R * D : 0), L.st);
            KCHK(c, vvk_posconv(&a, L.st, &m__));
        }
        L.pending = false;
        return 0;
    }
    // Residual stream protocol: a branch GEMM writes delta = gate * (out + bias) (operand dtype) and a LayerNorm kernel adds
    // it while it streams x anyway (no read-modify-write in a GEMM epilogue).  x is REWRITTEN ONCE PER BLOCK: the norm
    // before the MLP normalises x + d_attn without storing it (keep_x), the next block's first norm stores
    // (x + d_attn) + d_mlp -- the same additions in the same order, a third fewer bytes written by the norm kernels.
    // The residual LayerNorm behind a block (or, nothing pending, behind the step head): x + both deltas of that block -> L.h
    vv_ln_args residual_ln(const Lane& L, const float* scale, const float* shift, int keep_x) const {
        const bool pending = L.pending;
        vv_ln_args a{}; a.out_dtype = c->dt; a.x = L.xres; a.ldx = D; a.y = L.h; a.ldy = D; a.R = (int)L.R; a.D = D; a.add_one = 1; a.eps = 1e-6f;
        a.delta_dtype = c->dt; a.ld_delta = D; a.tail_row0 = L.tail_row0; a.delta_tail = L.h2_tail; a.delta2_tail = L.h3_tail;
        a.delta_tail_parts = pending ? L.tp_o : 0; a.delta2_tail_parts = pending ? L.tp_f : 0;
        a.w = scale; a.b = shift; a.keep_x = keep_x; a.delta = pending ? L.h2 : nullptr; a.delta2 = pending ? L.h3 : nullptr;
        return a;
    }
    // block l of evaluation e (= step * ns + stage, the row of the modulation tables)
    int block(Lane& L, int e, int l) const {
        const size_t R = L.R;
        const float* mod = c->modtab + ((size_t)l * S + e) * 6 * D;
        const std::string qkvw = blk(l, ".attn.qkv.weight"), qkvb = blk(l, ".attn.qkv.bias"), ow = blk(l, ".attn.out.weight"),
                          ob = blk(l, ".attn.out.bias"), f1w = blk(l, ".ff1.weight"), f1b = blk(l, ".ff1.bias"),
                          f2w = blk(l, ".ff2.weight"), f2b = blk(l, ".ff2.bias");
        vv_ln_args a = residual_ln(L, mod + D, mod, 0);  // scale_msa, shift_msa; x is stored
        { Prof p(c, VV_PROF_NORM, 0, (4.0 + es) * R * D + (L.pending ? (4.0 + 2.0 * es) * R * D : 0), L.st); KCHK(c, vvk_ln_mod(&a, L.st, &m__)); }
        Gemm qkv = gemm_args(c, c->dt, c->dt, VV_EPI_QKV_ROPE, VV_ACT_NONE_, L.h, D, qkvw.c_str(), D, qkvb.c_str(), L.qkv, 3 * D, (int)R, 3 * D, D);
        qkv.cos_q = q.a.rope_cos_q; qkv.sin_q = q.a.rope_sin_q; qkv.cos_k = q.a.rope_cos_k; qkv.sin_k = q.a.rope_sin_k;
        qkv.rope_cs_q = c->rope_rows ? L.csq_rows : L.csq; qkv.rope_cs_k = c->rope_rows ? L.csk_rows : L.csk; qkv.rope_by_row = c->rope_rows;
        qkv.seq_n = N; qkv.rope_dim = D; qkv.rope_pos = L.qkv_pos; qkv.rope_skip_q = q_rope_attn; qkv.rope_theta = rope_theta;
        if (int r = launch_gemm(c, qkv, VV_PROF_GEMM, L.st)) return r;
        {
            vv_attn_args t{}; t.dtype = c->dt; t.qkv = L.qkv; t.ld_qkv = 3 * D; t.out = L.att; t.ld_out = D; t.n_seq = L.n_seq; t.seq_n = N;
            t.heads = g.heads; t.dim = D; t.kv_len = L.kv_len; t.row_start = L.row_start; t.total_rows = (int)R;
            t.rope_cs_q = q_rope_attn ? L.csq : nullptr; t.q_scale = rope_theta > 0.f ? 1.0f / sqrtf((float)g.head_dim) : 0.f;
            Prof p(c, VV_PROF_ATTN, 4.0 * g.heads * L.sum_sq * 64, (double)es * R * 4 * D, L.st);
            KCHK(c, vvk_attention(&t, L.st, &m__));
        }
        Gemm out = gemm_args(c, c->dt, c->dt, VV_EPI_GATE_STORE, VV_ACT_NONE_, L.att, D, ow.c_str(), D, ob.c_str(), L.h2, D, (int)R, D, D);
        out.gate = mod + 2 * D;                         // gate_msa
        if (L.tp_o) { out.C_tail = L.h2_tail; out.tail_row0 = L.tail_row0; out.tail_parts = L.tp_o; }
        if (int r = launch_gemm(c, out, VV_PROF_GEMM, L.st)) return r;
        a.w = mod + 4 * D; a.b = mod + 3 * D;           // scale_mlp, shift_mlp
        a.delta = L.h2; a.delta2 = nullptr; a.keep_x = 1; a.delta_tail_parts = L.tp_o; a.delta2_tail_parts = 0;
        { Prof p(c, VV_PROF_NORM, 0, (4.0 + 2.0 * es) * R * D, L.st); KCHK(c, vvk_ln_mod(&a, L.st, &m__)); }
        if (int r = launch_gemm(c, gemm_args(c, c->dt, c->dt, VV_EPI_STORE, VV_ACT_GELU_TANH_, L.h, D, f1w.c_str(), D, f1b.c_str(), L.ffm, FF, (int)R, FF, D), VV_PROF_GEMM, L.st)) return r;
        Gemm ff2 = gemm_args(c, c->dt, c->dt, VV_EPI_GATE_STORE, VV_ACT_NONE_, L.ffm, FF, f2w.c_str(), FF, f2b.c_str(), L.h3, D, (int)R, D, FF);
        ff2.gate = mod + 5 * D;                         // gate_mlp
        if (L.tp_f) { ff2.C_tail = L.h3_tail; ff2.tail_row0 = L.tail_row0; ff2.tail_parts = L.tp_f; }
        if (int r = launch_gemm(c, ff2, VV_PROF_GEMM, L.st)) return r;
        L.pending = true;
        return 0;
    }
    // the final norm and projection of evaluation e
    int step_tail(Lane& L, int e) const {
        const size_t R = L.R;
        const float* fm = c->fintab + (size_t)e * 2 * D;
        vv_ln_args a = residual_ln(L, fm, fm + D, 1);        // scale, shift; x is re-initialised by the next step
        { Prof p(c, VV_PROF_NORM, 0, es * R * D + (L.pending ? (4.0 + 2.0 * es) * R * D : 4.0 * R * D), L.st); KCHK(c, vvk_ln_mod(&a, L.st, &m__)); }
        Gemm proj = gemm_args(c, c->dt, VV_DTYPE_F32, VV_EPI_STORE, VV_ACT_NONE_, L.h, D, "final.proj.weight", D, "final.proj.bias", L.pred, MP, (int)R, MP, D);
        proj.n_store = M;
        return launch_gemm(c, proj, VV_PROF_GEMM, L.st, 2.0 * R * D * M);
    }
    // the combine of stage i of step s.  !rk: exactly the Euler launch of the s = 1 plan (vvk_cfg_euler).  Else N7 -- CFG combine, slope
    // store, then the next stage's state or (last stage) x in place
    int combine(Lane& L, int s, int i) const {
        if (!q.rk) {
            Prof p(c, VV_PROF_ELEMWISE, 0, 16.0 * L.Rc * M, L.st);
            KCHK(c, vvk_cfg_euler(L.x, L.pred, MP, (int)L.Rc, M, g.cfg_strength, c->dt_host[s], L.row_src, L.st, &m__));
            return 0;
        }
        const vv_apg_args* apg = q.apg;
        const bool last = i == ns - 1;
        const double h = (double)c->dt_host[s];
        const int ring = ms_ring(c);
        vv_ode_stage_args a{};
        a.x = L.x; a.pred = L.pred; a.ldp = MP; a.Rc = (int)L.Rc; a.n_mel = M; a.n_prev = i;
        int n_read = 0;
        if (c->ms_q) {
            // N20: x += h (beta_0 f_s + beta_1 f_{s-1} + beta_2 f_{s-2}) in one launch of the stage kernel.  The call starts at step 0
            // (transformer_steps), so step s has s slopes behind it and reads nothing an earlier call left: the ring starts empty.
            const double* beta = c->ms_beta.data() + (size_t)s * c->ms_q;
            a.n_prev = std::min(c->ms_q - 1, s);
            for (int j = 1; j <= a.n_prev; ++j) {
                a.coef[j - 1] = (float)(h * beta[j]);
                if (a.coef[j - 1] != 0.f) { a.k_prev[j - 1] = L.hist[(s - j) % ring]; ++n_read; }
            }
            a.coef[a.n_prev] = (float)(h * beta[0]);
            a.k_out = (ring && (c->ode_report || s + 1 < c->n_steps)) ? L.hist[s % ring] : nullptr;     // the slot of the oldest slope read
        } else {
            for (int j = 0; j <= i; ++j) {
                a.coef[j] = (float)(h * (last ? c->ode_b[j] : c->ode_a[(i + 1) * 4 + j]));
                if (j < i && a.coef[j] != 0.f) { a.k_prev[j] = L.kbuf[c->ode_kslot[j]]; ++n_read; }
            }
            a.k_out = (!last && c->ode_kslot[i] >= 0) ? L.kbuf[c->ode_kslot[i]] : nullptr;
        }
        a.x_out = last ? nullptr : stage_state(L, i + 1);
        a.g = g.cfg_strength; a.g_item = q.a.cfg_item ? q.a.cfg_item + L.b0 : nullptr; a.seq_n = N; a.row_src = L.row_src;
        const int* u_row = q.guide ? L.u_row : nullptr;
        vv_apg_stage_args sa{};
        if (apg) {                                       // N11: the item sums of this evaluation, then their coefficients
            vv_apg_coef_args k{};
            k.pred = L.pred; k.ldp = MP; k.Rc = (int)L.Rc; k.n_mel = M; k.u_row = u_row;
            k.x_e = i ? stage_state(L, i) : L.x; k.row_src = i ? nullptr : L.row_src;
            k.B = L.B; k.n_tiles = (N + VV_APG_TILE - 1) / VV_APG_TILE; k.row_start = L.row_start; k.len = L.kv_len;
            k.t_e = apg->t_host[s * ns + i]; k.g = a.g; k.g_item = a.g_item;
            k.eta = apg->eta ? apg->eta + L.b0 : nullptr; k.norm_rms = apg->norm_rms ? apg->norm_rms + L.b0 : nullptr;
            k.partials = L.apg_part; k.coef = L.apg_coef;
            { Prof p(c, VV_PROF_ELEMWISE, 14.0 * L.Rc * M, 12.0 * L.Rc * M, L.st); KCHK(c, vvk_apg_coef(&k, 1, L.st, &m__)); }
            { Prof p(c, VV_PROF_ELEMWISE, 0, 24.0 * L.B * k.n_tiles, L.st); KCHK(c, vvk_apg_coef(&k, 2, L.st, &m__)); }
            sa.coef = L.apg_coef; sa.x_e = k.x_e; sa.x_e_packed = i ? 1 : 0; sa.t_e = k.t_e;
        }
        vv_reuse_stage_args ra{};
        if (q.with_reuse) {                              // N21: the items' modes at this evaluation; the drift sums before the stage kernel overwrites d_buf
            const int e = s * ns + i;
            const size_t at = (size_t)(e - q.a.step0 * ns) * q.a.B + L.b0;
            ra.d_buf = L.d_buf; ra.item_mode_host = q.ru_mode.data() + at; ra.n_items = L.B;
            if (q.with_drift) {
                vv_cfg_drift_args r{};
                r.pred = L.pred; r.ldp = MP; r.Rc = (int)L.Rc; r.n_mel = M; r.u_row = u_row; r.d_buf = L.d_buf; r.has_old_host = q.ru_old.data() + at;
                r.B = L.B; r.n_tiles = (N + VV_APG_TILE - 1) / VV_APG_TILE; r.row_start = L.row_start; r.len = L.kv_len;
                r.partials = L.drift_part; r.report = q.reuse->report + ((size_t)e * q.a.B + L.b0) * 2;
                { Prof p2(c, VV_PROF_ELEMWISE, 6.0 * L.Rc * M, 12.0 * L.Rc * M, L.st); KCHK(c, vvk_cfg_drift_reduce(&r, 1, L.st, &m__)); }
                { Prof p2(c, VV_PROF_ELEMWISE, 0, 16.0 * L.B * r.n_tiles, L.st); KCHK(c, vvk_cfg_drift_reduce(&r, 2, L.st, &m__)); }
            }
        }
        if (q.norm) {                                    // N24: the Gram sums of this evaluation, then the items' {s, f}
            vv_cfg_norm_coef_args k{};
            k.pred = L.pred; k.ldp = MP; k.Rc = (int)L.Rc; k.n_mel = M; k.u_row = u_row;
            k.B = L.B; k.n_tiles = (N + VV_APG_TILE - 1) / VV_APG_TILE; k.row_start = L.row_start; k.len = L.kv_len;
            k.g = a.g; k.g_item = a.g_item;
            k.star = q.norm->star ? q.norm->star + L.b0 : nullptr; k.rescale = q.norm->rescale ? q.norm->rescale + L.b0 : nullptr;
            k.partials = L.cn_part; k.coef = L.cn_coef;
            k.report = q.norm->report ? q.norm->report + ((size_t)(s * ns + i) * q.a.B + L.b0) * 2 : nullptr;
            { Prof p2(c, VV_PROF_ELEMWISE, 10.0 * L.Rc * M, 8.0 * L.Rc * M, L.st); KCHK(c, vvk_cfg_norm_coef(&k, 1, L.st, &m__)); }
            { Prof p2(c, VV_PROF_ELEMWISE, 0, 40.0 * L.B * k.n_tiles, L.st); KCHK(c, vvk_cfg_norm_coef(&k, 2, L.st, &m__)); }
        }
        Prof p(c, VV_PROF_ELEMWISE, 0, 4.0 * L.Rc * M * (4 + n_read + (a.k_out ? 1 : 0) + (apg ? 1 : 0) + (q.with_reuse ? 1 : 0)), L.st);
        KCHK(c, vvk_ode_stage(&a, u_row, apg ? &sa : nullptr, L.st, &m__, c->ms_q ? 1 : 0, q.with_reuse ? &ra : nullptr, q.norm ? L.cn_coef : nullptr));
        if (c->ms_q && c->ode_report) {                  // N20: the step report, from the slope just stored and the one before it
            vv_ode_diff_args r{};
            r.f = L.hist[s % ring]; r.f_prev = s ? L.hist[(s - 1) % ring] : nullptr; r.Rc = (int)L.Rc; r.n_mel = M;
            r.B = L.B; r.n_tiles = (N + VV_APG_TILE - 1) / VV_APG_TILE; r.row_start = L.row_start; r.len = L.kv_len;
            r.partials = L.rep_part; r.report = c->ode_report + ((size_t)s * q.a.B + L.b0) * 2;
            { Prof p2(c, VV_PROF_ELEMWISE, 6.0 * L.Rc * M, 8.0 * L.Rc * M, L.st); KCHK(c, vvk_ode_diff_reduce(&r, 1, L.st, &m__)); }
            { Prof p2(c, VV_PROF_ELEMWISE, 0, 16.0 * L.B * r.n_tiles, L.st); KCHK(c, vvk_ode_diff_reduce(&r, 2, L.st, &m__)); }
        }
        return 0;
    }
    // N23: one launch of the span kernel on a lane (or view) in front of a block or of the tail -- `which` plane takes X (MARK), becomes the
    // span's contribution (DIFF), or is added back (APPLY: x is rewritten and nothing is pending behind it)
    int span(Lane& L, int mode, int which) const {
        vv_block_span_args a{};
        a.mode = mode; a.delta_dtype = c->dt; a.x = L.xres; a.d1 = L.pending ? L.h2 : nullptr; a.d2 = L.pending ? L.h3 : nullptr;
        a.buf = L.bc_buf[which]; a.R = (int)L.R; a.D = D;
        {
            Prof p(c, VV_PROF_ELEMWISE, 0, (4.0 + (L.pending ? 2.0 * es : 0) + (mode == VV_SPAN_MARK ? 4.0 : 8.0)) * L.R * D, L.st);
            KCHK(c, vvk_block_span(&a, L.st, &m__));
        }
        if (mode == VV_SPAN_APPLY) L.pending = false;
        return 0;
    }
    // N23: the report rows of evaluation e for the sequences of a lane (both branches) or of branch view v: the sums of plane `which` against
    // the other one (with_prev) behind a DIFF, zeros (which < 0) at an evaluation that stores nothing
    int span_report(Lane& L, int v, int e, int which, bool with_prev) const {
        vv_block_drift_args r{};
        r.R = (int)L.R; r.D = D; r.n_seq = L.n_seq; r.n_items = L.B; r.branch0 = P.branch_lanes ? v : 0; r.n_tiles = (N + VV_APG_TILE - 1) / VV_APG_TILE;
        r.row_start = L.row_start; r.len = L.kv_len; r.partials = L.bc_part; r.report = q.bc->report + ((size_t)e * q.a.B + L.b0) * 4;
        if (which < 0) { Prof p(c, VV_PROF_ELEMWISE, 0, 16.0 * L.n_seq, L.st); KCHK(c, vvk_block_drift_reduce(&r, 4, L.st, &m__)); return 0; }
        r.d_new = L.bc_buf[which]; r.d_prev = with_prev ? L.bc_buf[which ^ 1] : nullptr;
        { Prof p(c, VV_PROF_ELEMWISE, 6.0 * L.R * D, (with_prev ? 8.0 : 4.0) * L.R * D, L.st); KCHK(c, vvk_block_drift_reduce(&r, 1, L.st, &m__)); }
        { Prof p(c, VV_PROF_ELEMWISE, 0, 16.0 * L.n_seq * r.n_tiles, L.st); KCHK(c, vvk_block_drift_reduce(&r, 2, L.st, &m__)); }
        return 0;
    }
    // What the block-level kernels (step_head, block, step_tail) run on: views of the lanes' buffers, two at the most; -> their number.
    // The schedule gives each its stream.  Branch lanes: view v is the conditional (0) or the unconditional (1) half of the one lane's rows.
    Lane branch_view(const Lane& L, int v) const {
        Lane V = L;
        const size_t r0 = v ? L.Rc : 0;                 // the unconditional branch's rows follow the conditional branch's
        V.R = L.Rc; V.n_seq = L.B; V.sum_sq = L.sum_sq / 2;
        V.xcat += r0 * KP * es; V.h += r0 * D * es; V.h2 += r0 * D * es; V.h3 += r0 * D * es; V.att += r0 * D * es;
        V.qkv += r0 * 3 * D * es; V.ffm += r0 * FF * es; V.xres += r0 * D; V.pred += r0 * MP;
        V.csq_rows += r0 * 64; V.csk_rows += r0 * 64;
        for (float*& b : V.bc_buf) if (b) b += r0 * D;                 // N23: the view's half of the planes and of the partial sums
        if (V.bc_part && v) V.bc_part += (size_t)L.B * ((N + VV_APG_TILE - 1) / VV_APG_TILE) * 2;
        // row_start / kv_len: the conditional branch's entries serve both views (same lengths, rows relative to the view's base);
        // row_pos: the first Rc entries (a row's position does not depend on its branch)
        return V;
    }
    // The views of one evaluation.  gstate == nullptr (no mask): the lanes themselves, or the two halves of the one lane.
    // N8, under a mask: Rc + Ru rows and B + Bu sequences on the subset's tables.  Branch lanes: the side stream's view is the Ru
    // compacted rows (sequence starts relative to the unconditional half); there is none when Ru = 0.
    int lane_views(const GuideState* gstate, Lane* views) const {
        const int n_views = !P.branch_lanes ? P.n_lanes : (gstate && !gstate[0].Ru) ? 1 : 2;
        for (int v = 0; v < n_views; ++v) {
            const Lane& L = P.lanes[P.branch_lanes ? 0 : v];
            Lane& V = views[v] = P.branch_lanes ? branch_view(L, v) : L;
            if (!gstate) continue;
            const GuideState& G = gstate[P.branch_lanes ? 0 : v];
            if (P.branch_lanes) {
                V.row_start = v ? L.g_rs_rel : L.g_row_start; V.kv_len = v ? L.g_kv_len + L.B : L.g_kv_len;
                V.qkv_pos = L.uniform ? nullptr : (v ? L.g_row_pos + L.Rc : L.g_row_pos);
                if (v) { V.R = G.Ru; V.n_seq = G.Bu; V.sum_sq = G.sum_sq; }
            } else {
                V.R = V.Rc + G.Ru; V.n_seq = V.B + G.Bu; V.sum_sq = V.sum_sq / 2 + G.sum_sq;
                V.row_start = V.g_row_start; V.kv_len = V.g_kv_len; V.qkv_pos = V.uniform ? nullptr : V.g_row_pos;
            }
        }
        return n_views;
    }
};

// The schedule of one call: order, streams (lane and view 0: the caller's, 1: the context's side stream, made on first use), forks, joins.
// Launch order: the lanes alternate block by block, so both streams always hold work and neither lane's enqueue waits for the
// other's queue to drain; the device orders each stream by itself.  Item lanes: lane 1 forks from the caller's stream once (what
// the caller enqueued before this call is visible to it) and joins back at the end (what the caller enqueues next sees both
// lanes).  Branch lanes: the same fork / join once per STEP, between the conditioning pack and the CFG combine.
int steps_schedule(const StepsRun& r, Lane* lanes, hipStream_t st) {
    vv_ctx* c = r.c;
    const int n_lanes = r.P.n_lanes, step0 = r.q.a.step0, n_steps = r.q.a.n_steps;
    const bool branch_lanes = r.P.branch_lanes, guide = r.q.guide != nullptr;
    if ((n_lanes > 1 || branch_lanes) && !c->side_stream[0]) {
        HIPCHK(c, hipStreamCreateWithFlags(&c->side_stream[0], hipStreamNonBlocking));
        HIPCHK(c, hipEventCreateWithFlags(&c->ev_join[0], hipEventDisableTiming));
    }
    if ((n_lanes > 1 || branch_lanes) && !c->ev_fork) HIPCHK(c, hipEventCreateWithFlags(&c->ev_fork, hipEventDisableTiming));
    const hipStream_t streams[2] = {st, c->side_stream[0]};
    auto fork = [&]() -> int {
        HIPCHK(c, hipEventRecord(c->ev_fork, st)); HIPCHK(c, hipStreamWaitEvent(c->side_stream[0], c->ev_fork, 0));
        return 0;
    };
    // always reached, also after a failed launch: the side stream must not outlive the call
    auto join = [&]() { hipEventRecord(c->ev_join[0], c->side_stream[0]); hipStreamWaitEvent(st, c->ev_join[0], 0); };
    Lane views[2]; GuideState gstate[2];
    auto make_views = [&](const GuideState* gs) {         // view v runs on stream v, as lane v does
        const int n = r.lane_views(gs, views);
        for (int v = 0; v < n; ++v) views[v].st = streams[v];
        return c->chip_share = n;
    };
    for (int li = 0; li < n_lanes; ++li) lanes[li].st = streams[li];
    int n_views = make_views(nullptr), rc = 0;
    // N23: the span, the modes, and where the latest stored contribution lives (plane `cur`; under a report the stores alternate)
    const vv_block_cache_args* bc = r.q.with_cache ? r.q.bc : nullptr;
    const bool bc_report = bc && r.q.with_cache_report;
    int bc_cur = 0; bool bc_stored = false;
    if (n_lanes > 1) rc = fork();
    for (int li = 0; li < n_lanes && !rc; ++li) rc = r.setup(lanes[li]);
    for (int s = step0; s < step0 + n_steps && !rc; ++s)
        for (int i = 0; i < r.ns && !rc; ++i) {           // the evaluations of one ODE step (one for Euler); branch lanes fork / join around each
            const int e = s * r.ns + i;
            for (int li = 0; li < n_lanes && !rc; ++li) rc = r.pack(lanes[li], gstate[li], s, i);
            if (guide) n_views = make_views(gstate);      // N8: the views follow the evaluation's guided subset
            const bool want_fork = branch_lanes && n_views == 2;   // N8: an evaluation without unconditional rows neither forks nor joins
            if (want_fork && !rc) rc = fork();
            const bool forked = want_fork && !rc;
            for (int v = 0; v < n_views && !rc; ++v) rc = r.step_head(views[v]);
            const int mode = bc ? bc->modes_host[e] : VV_BLOCK_FULL;
            if (mode == VV_BLOCK_STORE && bc_report && bc_stored) bc_cur ^= 1;
            for (int l = 0; l <= r.g.depth && !rc; ++l)   // l = depth: the tail
                for (int v = 0; v < n_views && !rc; ++v) {
                    Lane& V = views[v];
                    if (mode == VV_BLOCK_LIGHT && l >= bc->first && l < bc->last) {     // the span: its first block's place takes the APPLY, the rest launch nothing
                        if (l == bc->first) rc = r.span(V, VV_SPAN_APPLY, bc_cur);
                        continue;
                    }
                    if (mode == VV_BLOCK_STORE && l == bc->first) rc = r.span(V, VV_SPAN_MARK, bc_cur);
                    if (mode == VV_BLOCK_STORE && l == bc->last && !rc) {
                        rc = r.span(V, VV_SPAN_DIFF, bc_cur);
                        if (bc_report && !rc) rc = r.span_report(V, v, e, bc_cur, bc_stored);
                    }
                    if (bc_report && mode != VV_BLOCK_STORE && l == r.g.depth && !rc) rc = r.span_report(V, v, e, -1, false);
                    if (!rc) rc = l < r.g.depth ? r.block(V, e, l) : r.step_tail(V, e);
                }
            if (mode == VV_BLOCK_STORE) bc_stored = true;
            if (forked) join();
            for (int li = 0; li < n_lanes && !rc; ++li) rc = r.combine(lanes[li], s, i);
        }
    if (n_lanes > 1) join();
    c->chip_share = 1;
    return rc;
}
}  // namespace

// The stage: the checks every entry shares, the host lengths, the lane plan, the workspace, the schedule.
// q.a.ws != nullptr: the workspace is taken from that caller-owned block instead of the context's (what a captured hipGraph must point into).
static int transformer_steps(vv_ctx* c, StepsCall q, void* stream) {
    if (!c) return -22;
    const vv_steps_args& a = q.a;
    q.with_norm = q.norm != nullptr || q.ws_form == WS_NORM;
    if (q.norm && !q.ws_only && a.B > 0) {                // N24: no 2 in the mask (a reused item has no p_u to measure); no mask = one of ones
        const size_t E = (size_t)c->n_steps * c->ode_s;
        if (q.guide && q.ld_guide >= a.B)
            for (size_t e = 0; e < E; ++e)
                for (int b = 0; b < a.B; ++b)
                    if (q.guide[e * q.ld_guide + b] == 2)
                        return c->fail(-22, "vv_transformer_steps_norm: mask value 2 (guidance reuse) at evaluation %d, item %d: the item has no unconditional prediction to measure", (int)e, b);
        if (!q.guide) { q.all_guided.assign(E * a.B, 1); q.guide = q.all_guided.data(); q.ld_guide = a.B; }
    }
    q.with_apg = q.apg != nullptr || q.ws_form == WS_APG; q.guided = q.guide != nullptr || (q.ws_form != WS_PLAIN && q.ws_form != WS_CACHED && q.ws_form != WS_CACHED_REPORT) || q.with_apg;
    q.rk = c->ode_s > 1 || c->ms_q > 0 || a.cfg_item != nullptr || q.guide != nullptr || q.apg != nullptr;   // false: exactly the Euler launches (vvk_cfg_euler) and workspace of the s = 1 plan
    const int B = a.B, N = a.N;
    if (!c->finalized || !c->modtab) return c->fail(-1, "vv_transformer_steps: weights/time grid not ready");
    if (B < 1 || N < 1 || (!q.ws_only && (!a.seq_len || !a.x || !a.cat_mel_text || !a.cat_mel_text_drop || !a.rope_cos_q || !a.rope_sin_q || !a.rope_cos_k || !a.rope_sin_k)))
        return c->fail(-22, "vv_transformer_steps: bad arguments");
    if (a.step0 < 0 || a.n_steps < 0 || a.step0 + a.n_steps > c->n_steps) return c->fail(-22, "vv_transformer_steps: steps [%d,%d) outside the time grid (%d)", a.step0, a.step0 + a.n_steps, c->n_steps);
    if (c->ms_q && !q.ws_only && a.step0 != 0) return c->fail(-22, "vv_transformer_steps: under a multistep plan a call starts at step 0 (the kept slopes live for one call), got step0 = %d", a.step0);
    if (c->ms_q && c->ode_report && !q.ws_only && (c->report_B != B || c->report_steps != c->n_steps))
        return c->fail(-22, "vv_transformer_steps: the step report was set for %d steps of %d items, the call has %d of %d", c->report_steps, c->report_B, c->n_steps, B);
    if (q.guide && q.ld_guide < B) return c->fail(-22, "vv_transformer_steps_guided: ld_guide = %d < B = %d", q.ld_guide, B);
    if (q.guide && c->split_k_tail) return c->fail(-22, "vv_transformer_steps_guided: a guidance mask cannot be combined with option split_k_tail (its tail plan depends on the row count)");
    if (q.guided && B > VVK_GUIDE_MAX_ITEMS) return c->fail(-22, "vv_transformer_steps_guided: at most %d items per call", VVK_GUIDE_MAX_ITEMS);
    q.with_drift = q.ws_form == WS_REUSE_REPORT || (q.reuse && q.reuse->report); q.with_reuse = q.with_drift || q.ws_form == WS_REUSE;
    if (q.reuse_entry && !q.ws_only) {                    // N21: the mask's values, and what the stage kernel does for each item at each evaluation of the call
        const int E = c->n_steps * c->ode_s, ns = c->ode_s, e0 = a.step0 * ns, e1 = (a.step0 + a.n_steps) * ns;
        if (q.with_drift && !q.guide) return c->fail(-22, "vv_transformer_steps_reuse: the drift report needs a mask");
        if (q.with_drift && ((uintptr_t)q.reuse->report % 8 || q.reuse->report_B != B || q.reuse->report_evals != E))
            return c->fail(-22, "vv_transformer_steps_reuse: the report is float64 [%d evaluations of the plan][%d items][2], got [%d][%d][2]", E, B, q.reuse->report_evals, q.reuse->report_B);
        bool has2 = false;
        for (int e = 0; e < E && q.guide; ++e)
            for (int b = 0; b < B; ++b) {
                const uint8_t v = q.guide[(size_t)e * q.ld_guide + b];
                if (v > 2) return c->fail(-22, "vv_transformer_steps_reuse: mask value %d at evaluation %d, item %d (0 = not guided, 1 = computed, 2 = reused)", (int)v, e, b);
                has2 = has2 || v == 2;
            }
        if (has2 && a.step0 != 0) return c->fail(-22, "vv_transformer_steps_reuse: a call that reuses starts at step 0 (the stored differences live for one call), got step0 = %d", a.step0);
        q.with_reuse = q.with_reuse || has2;
        if (q.with_reuse) {
            q.ru_mode.assign((size_t)(e1 - e0) * B, 0); q.ru_old.assign((size_t)(e1 - e0) * B, 0);
            for (int b = 0; b < B; ++b) {
                bool seen = false, need = false;
                for (int e = e0; e < e1; ++e) {
                    const uint8_t v = q.guide[(size_t)e * q.ld_guide + b];
                    if (v == 2 && !seen) return c->fail(-22, "vv_transformer_steps_reuse: item %d reuses at evaluation %d with no computed evaluation before it in the call", b, e);
                    q.ru_old[(size_t)(e - e0) * B + b] = seen;
                    if (v == 2) q.ru_mode[(size_t)(e - e0) * B + b] = VV_REUSE_LOAD;
                    seen = seen || v == 1;
                }
                for (int e = e1 - 1; e >= e0; --e) {     // D is stored where a later evaluation reads it (at every computed one under a report)
                    const uint8_t v = q.guide[(size_t)e * q.ld_guide + b];
                    if (v == 2) need = true;
                    if (v == 1) { if (need || q.with_drift) q.ru_mode[(size_t)(e - e0) * B + b] = VV_REUSE_STORE; need = false; }
                }
            }
        }
    }
    q.with_cache_report = q.ws_form == WS_CACHED_REPORT || (q.bc && q.bc->report); q.with_cache = q.with_cache_report || q.ws_form == WS_CACHED || q.bc;
    if (q.with_cache && c->split_k_tail) return c->fail(-22, "vv_transformer_steps_cached: block caching cannot be combined with option split_k_tail (its tail rows keep fp32 parts instead of a delta)");
    if (q.bc) {                                           // N23: the span, the modes of the plan and what the call's own evaluations ask for
        const vv_block_cache_args& k = *q.bc;
        const int E = c->n_steps * c->ode_s, e0 = a.step0 * c->ode_s, e1 = (a.step0 + a.n_steps) * c->ode_s;
        if (k.first < 0 || k.first >= k.last || k.last > c->cfg.depth) return c->fail(-22, "vv_transformer_steps_cached: the span [%d, %d) is not inside the %d blocks", k.first, k.last, c->cfg.depth);
        if (!k.modes_host || k.n_modes != E) return c->fail(-22, "vv_transformer_steps_cached: one mode per evaluation of the plan (%d), got %d", E, k.n_modes);
        if (k.report && ((uintptr_t)k.report % 8 || k.report_B != B || k.report_evals != E))
            return c->fail(-22, "vv_transformer_steps_cached: the report is float64 [%d evaluations of the plan][%d items][2][2], got [%d][%d][2][2]", E, B, k.report_evals, k.report_B);
        if (k.report && B > VVK_GUIDE_MAX_ITEMS) return c->fail(-22, "vv_transformer_steps_cached: at most %d items per call with a report", VVK_GUIDE_MAX_ITEMS);
        for (int e = 0; e < E; ++e)
            if (k.modes_host[e] > VV_BLOCK_LIGHT) return c->fail(-22, "vv_transformer_steps_cached: mode %d at evaluation %d (0 = full, 1 = full and store, 2 = light)", (int)k.modes_host[e], e);
        bool stored = false;
        for (int e = e0; e < e1; ++e) {
            if (k.modes_host[e] == VV_BLOCK_LIGHT && a.step0 != 0)
                return c->fail(-22, "vv_transformer_steps_cached: a call with a light evaluation starts at step 0 (the stored contribution lives for one call), got step0 = %d", a.step0);
            if (k.modes_host[e] == VV_BLOCK_LIGHT && !stored) return c->fail(-22, "vv_transformer_steps_cached: evaluation %d is light with no storing evaluation before it in the call", e);
            stored = stored || k.modes_host[e] == VV_BLOCK_STORE;
        }
    }
    hipStream_t st = enter(c, stream);
    const vv_model_cfg& g = c->cfg;
    const StepDims d{g.dim, g.dim * g.ff_mult, g.n_mel, g.n_mel + g.text_dim, c->esz(), pad_to(2 * g.n_mel + g.text_dim, 64), pad_to(g.n_mel, 128)};
    if ((size_t)2 * B * N > (size_t)1 << 30) return c->fail(-22, "batch too large");
    // Ragged rows are PACKED: sequence (branch, b) owns rows [row_start, +len_b) of every activation buffer, the conditional
    // branch first, so GEMMs / norms / convs touch sum(len) rows instead of B x N_max.  The host needs the row count for the
    // launch shapes: the caller hands the lengths over on the host as well (vv_transformer_steps_h: no synchronisation at all,
    // the call can be captured into a hipGraph), or they are read back once (4*B bytes, one stream synchronisation).  The row
    // tables themselves are built on the device.  x, cat and cat_drop keep their padded [B][N] layout (row_src maps).
    std::vector<int> hlen(B);
    if (a.seq_len_host) std::copy(a.seq_len_host, a.seq_len_host + B, hlen.begin());
    else {
        HIPCHK(c, hipMemcpyAsync(hlen.data(), a.seq_len, sizeof(int) * B, hipMemcpyDeviceToHost, st));
        HIPCHK(c, hipStreamSynchronize(st));
    }
    size_t Rc_all = 0;
    for (int b = 0; b < B; ++b) {
        if (hlen[b] < 1 || hlen[b] > N) return c->fail(-22, "vv_transformer_steps: seq_len[%d] = %d outside [1, %d]", b, hlen[b], N);
        Rc_all += hlen[b];
    }
    if (2 * Rc_all * 3 * (size_t)d.D * d.es >= ((size_t)1 << 31))
        return c->fail(-22, "vv_transformer_steps: %zu packed rows make a %zu-byte qkv buffer; kernels address it with 32-bit byte offsets "
                            "(< 2 GiB) -- synthesise fewer units per call", 2 * Rc_all, 2 * Rc_all * 3 * (size_t)d.D * d.es);
    LanePlan P = lane_plan(c, d, hlen, N);
    auto bufs = [&](Arena& ar) { for (int li = 0; li < P.n_lanes; ++li) lane_bufs(ar, P.lanes[li], c, d, N, q.guided, q.with_apg, q.with_reuse, q.with_drift, q.with_cache, q.with_cache_report, q.with_norm); };
    if (q.ws_only) { *q.ws_only = (uint64_t)align_up(plan_bytes(bufs), 256); return 0; }
    if (int r = plan_ws(c, a.ws, (size_t)a.ws_bytes, bufs)) return r;
    for (int li = 0; li < P.n_lanes; ++li) {              // each lane's slice of the call's arrays
        Lane& L = P.lanes[li];
        L.seq_len = a.seq_len + L.b0; L.x = a.x + (size_t)L.b0 * N * d.M;
        L.cat = a.cat_mel_text + (size_t)L.b0 * N * d.CD; L.cat_drop = a.cat_mel_text_drop + (size_t)L.b0 * N * d.CD;
    }
    return steps_schedule(StepsRun(c, d, q, hlen, P), P.lanes, st);
}

// the arguments of the positional entries as the call the stage runs on
static StepsCall steps_call(int B, int N, const int32_t* seq_len, const int32_t* seq_len_host, float* x, const float* cat, const float* cat_drop,
                            const float* rope_cos_q, const float* rope_sin_q, const float* rope_cos_k, const float* rope_sin_k, int step0, int n_steps) {
    StepsCall q; vv_steps_args& a = q.a;
    a.B = B; a.N = N; a.seq_len = seq_len; a.seq_len_host = seq_len_host; a.x = x; a.cat_mel_text = cat; a.cat_mel_text_drop = cat_drop;
    a.rope_cos_q = rope_cos_q; a.rope_sin_q = rope_sin_q; a.rope_cos_k = rope_cos_k; a.rope_sin_k = rope_sin_k; a.step0 = step0; a.n_steps = n_steps;
    return q;
}
// the struct entries (_ex, _guided, _apg): what they check of their arguments, under the entry's name, and the call
static int steps_struct_call(vv_ctx* c, const char* entry, const vv_steps_args* a, const uint8_t* guide, int ld_guide, const vv_apg_args* apg, void* stream) {
    if (!c) return -22;
    if (!a) return c->fail(-22, "%s: null arguments", entry);
    if (a->ws && !a->seq_len_host) return c->fail(-22, "%s: a workspace block needs the host lengths", entry);
    if (a->cfg_item && (uintptr_t)a->cfg_item % 4) return c->fail(-22, "%s: cfg_item must be a float array", entry);
    if (apg && !apg->t_host) return c->fail(-22, "%s: the evaluation times t_host are required", entry);
    if (apg && ((uintptr_t)apg->eta | (uintptr_t)apg->norm_rms) % 4) return c->fail(-22, "%s: eta and norm_rms must be float arrays", entry);
    StepsCall q; q.a = *a; q.guide = guide; q.ld_guide = ld_guide; q.apg = apg;
    return transformer_steps(c, q, stream);
}
// the three size queries: nothing is launched, so no device pointer is needed
static int steps_ws_query(vv_ctx* c, const char* entry, WsForm form, int B, int N, const int32_t* seq_len_host, uint64_t* bytes) {
    if (c && (!seq_len_host || !bytes)) return c->fail(-22, "%s: bad arguments", entry);
    StepsCall q; q.a.B = B; q.a.N = N; q.a.seq_len_host = seq_len_host; q.ws_form = form; q.ws_only = bytes;
    return transformer_steps(c, q, nullptr);
}

int vv_transformer_steps(vv_ctx* c, int B, int N, const int32_t* seq_len, float* x, const float* cat, const float* cat_drop,
                         const float* rope_cos_q, const float* rope_sin_q, const float* rope_cos_k, const float* rope_sin_k,
                         int step0, int n_steps, void* stream) {
    return transformer_steps(c, steps_call(B, N, seq_len, nullptr, x, cat, cat_drop, rope_cos_q, rope_sin_q, rope_cos_k, rope_sin_k, step0, n_steps), stream);
}

// Same, with the per-item lengths ALSO given on the host (they must equal the device array): no read-back, no stream
// synchronisation anywhere in the call -- with a workspace that is already large enough it can be captured into a hipGraph.
int vv_transformer_steps_h(vv_ctx* c, int B, int N, const int32_t* seq_len, const int32_t* seq_len_host, float* x, const float* cat,
                           const float* cat_drop, const float* rope_cos_q, const float* rope_sin_q, const float* rope_cos_k,
                           const float* rope_sin_k, int step0, int n_steps, void* stream) {
    if (c && !seq_len_host) return c->fail(-22, "vv_transformer_steps_h: host lengths missing");
    return transformer_steps(c, steps_call(B, N, seq_len, seq_len_host, x, cat, cat_drop, rope_cos_q, rope_sin_q, rope_cos_k, rope_sin_k, step0, n_steps), stream);
}

// The same call with every intermediate taken from a CALLER-OWNED block (>= vv_transformer_ws_bytes for the same B, N and host
// lengths, 256-byte aligned): no allocation and no synchronisation anywhere in the call, and nothing it points at can move -- the
// form to capture into a hipGraph (all Euler steps of an utterance + vv_decode_into = one graph launch).
int vv_transformer_ws_bytes(vv_ctx* c, int B, int N, const int32_t* seq_len_host, uint64_t* bytes) {
    return steps_ws_query(c, "vv_transformer_ws_bytes", WS_PLAIN, B, N, seq_len_host, bytes);
}

int vv_transformer_steps_into(vv_ctx* c, int B, int N, const int32_t* seq_len, const int32_t* seq_len_host, float* x, const float* cat,
                              const float* cat_drop, const float* rope_cos_q, const float* rope_sin_q, const float* rope_cos_k,
                              const float* rope_sin_k, int step0, int n_steps, void* ws, uint64_t ws_bytes, void* stream) {
    if (c && (!seq_len_host || !ws)) return c->fail(-22, "vv_transformer_steps_into: host lengths and a workspace block are required");
    StepsCall q = steps_call(B, N, seq_len, seq_len_host, x, cat, cat_drop, rope_cos_q, rope_sin_q, rope_cos_k, rope_sin_k, step0, n_steps);
    q.a.ws = ws; q.a.ws_bytes = ws_bytes;
    return transformer_steps(c, q, stream);
}

// N7: the struct-argument form -- the arguments of the three entries above plus a guidance strength per item
int vv_transformer_steps_ex(vv_ctx* c, const vv_steps_args* a, void* stream) {
    return steps_struct_call(c, "vv_transformer_steps_ex", a, nullptr, 0, nullptr, stream);
}

// N8: a guidance mask on top of vv_transformer_steps_ex (include/vvtts.h)
int vv_transformer_steps_guided(vv_ctx* c, const vv_steps_args* a, const uint8_t* guide_host, int ld_guide, void* stream) {
    if (!guide_host) return vv_transformer_steps_ex(c, a, stream);
    return steps_struct_call(c, "vv_transformer_steps_guided", a, guide_host, ld_guide, nullptr, stream);
}

int vv_transformer_guided_ws_bytes(vv_ctx* c, int B, int N, const int32_t* seq_len_host, uint64_t* bytes) {
    return steps_ws_query(c, "vv_transformer_guided_ws_bytes", WS_GUIDED, B, N, seq_len_host, bytes);
}

// N11: projected guidance on top of vv_transformer_steps_guided (include/vvtts.h)
int vv_transformer_steps_apg(vv_ctx* c, const vv_steps_args* a, const uint8_t* guide_host, int ld_guide, const vv_apg_args* apg, void* stream) {
    if (!apg) return vv_transformer_steps_guided(c, a, guide_host, ld_guide, stream);
    return steps_struct_call(c, "vv_transformer_steps_apg", a, guide_host, ld_guide, apg, stream);
}

int vv_transformer_apg_ws_bytes(vv_ctx* c, int B, int N, const int32_t* seq_len_host, uint64_t* bytes) {
    return steps_ws_query(c, "vv_transformer_apg_ws_bytes", WS_APG, B, N, seq_len_host, bytes);
}

// N24: CFG-Zero* and guidance rescale on top of vv_transformer_steps_guided (include/vvtts.h)
int vv_transformer_steps_norm(vv_ctx* c, const vv_steps_args* a, const uint8_t* guide_host, int ld_guide, const vv_cfg_norm_args* norm, void* stream) {
    if (!norm) return vv_transformer_steps_guided(c, a, guide_host, ld_guide, stream);
    if (!c) return -22;
    if (!a) return c->fail(-22, "vv_transformer_steps_norm: null arguments");
    if (a->ws && !a->seq_len_host) return c->fail(-22, "vv_transformer_steps_norm: a workspace block needs the host lengths");
    if (a->cfg_item && (uintptr_t)a->cfg_item % 4) return c->fail(-22, "vv_transformer_steps_norm: cfg_item must be a float array");
    if (((uintptr_t)norm->star | (uintptr_t)norm->rescale) % 4 || (uintptr_t)norm->report % 8) return c->fail(-22, "vv_transformer_steps_norm: star and rescale must be float arrays, the report 8-byte aligned");
    StepsCall q; q.a = *a; q.guide = guide_host; q.ld_guide = ld_guide; q.norm = norm;
    return transformer_steps(c, q, stream);
}

int vv_transformer_norm_ws_bytes(vv_ctx* c, int B, int N, const int32_t* seq_len_host, uint64_t* bytes) {
    return steps_ws_query(c, "vv_transformer_norm_ws_bytes", WS_NORM, B, N, seq_len_host, bytes);
}

// N21: a third mask value on top of vv_transformer_steps_guided (include/vvtts.h)
int vv_transformer_steps_reuse(vv_ctx* c, const vv_steps_args* a, const uint8_t* guide_host, int ld_guide, const vv_reuse_args* reuse, void* stream) {
    if (!c) return -22;
    if (!a) return c->fail(-22, "vv_transformer_steps_reuse: null arguments");
    if (!guide_host && !(reuse && reuse->report)) return vv_transformer_steps_ex(c, a, stream);
    if (a->ws && !a->seq_len_host) return c->fail(-22, "vv_transformer_steps_reuse: a workspace block needs the host lengths");
    if (a->cfg_item && (uintptr_t)a->cfg_item % 4) return c->fail(-22, "vv_transformer_steps_reuse: cfg_item must be a float array");
    StepsCall q; q.a = *a; q.guide = guide_host; q.ld_guide = ld_guide; q.reuse_entry = true; q.reuse = reuse;
    return transformer_steps(c, q, stream);
}

int vv_transformer_reuse_ws_bytes(vv_ctx* c, int B, int N, const int32_t* seq_len_host, int with_report, uint64_t* bytes) {
    return steps_ws_query(c, "vv_transformer_reuse_ws_bytes", with_report ? WS_REUSE_REPORT : WS_REUSE, B, N, seq_len_host, bytes);
}

// N23: block caching on top of vv_transformer_steps_ex (include/vvtts.h)
int vv_transformer_steps_cached(vv_ctx* c, const vv_steps_args* a, const vv_block_cache_args* cache, void* stream) {
    if (!c) return -22;
    if (!a) return c->fail(-22, "vv_transformer_steps_cached: null arguments");
    if (!cache) return vv_transformer_steps_ex(c, a, stream);
    bool any = cache->report != nullptr;
    if (cache->modes_host && cache->n_modes == c->n_steps * c->ode_s && cache->first >= 0 && cache->first < cache->last && cache->last <= c->cfg.depth) {
        for (int e = 0; e < cache->n_modes; ++e) any = any || cache->modes_host[e] != VV_BLOCK_FULL;
        if (!any) return vv_transformer_steps_ex(c, a, stream);     // every evaluation full, no report: the plain call, launches and workspace
    }
    if (a->ws && !a->seq_len_host) return c->fail(-22, "vv_transformer_steps_cached: a workspace block needs the host lengths");
    if (a->cfg_item && (uintptr_t)a->cfg_item % 4) return c->fail(-22, "vv_transformer_steps_cached: cfg_item must be a float array");
    StepsCall q; q.a = *a; q.bc = cache;
    return transformer_steps(c, q, stream);
}

int vv_transformer_cached_ws_bytes(vv_ctx* c, int B, int N, const int32_t* seq_len_host, int with_report, uint64_t* bytes) {
    return steps_ws_query(c, "vv_transformer_cached_ws_bytes", with_report ? WS_CACHED_REPORT : WS_CACHED, B, N, seq_len_host, bytes);
}

// --------------------------------------------------------------------------------------- decode
static int vocos_wide(const vv_ctx* c) {
    const vv_vocos_cfg& v = c->vcfg;
    return std::max(std::max(pad_to(v.embed_k * c->cfg.n_mel, 32), v.intermediate), pad_to(v.n_fft + 2, 128));
}
// N6 Vocos: lens[B], three [B * T_max][dim] planes (residual stream, conv / norm outputs), one plane as wide as the widest GEMM
// operand (im2col, intermediate, head, frames), the spectrum operand [B * T_max][n_fft]
struct VocosBufs { int* lens; float *res, *t, *hn, *big, *spec; };
static VocosBufs vocos_bufs(Arena& a, const vv_ctx* c, int B, int T_max) {
    const size_t R = (size_t)B * T_max, V = c->vcfg.dim;
    VocosBufs w;
    w.lens = a.take<int>(B);
    w.res = a.take<float>(R * V); w.t = a.take<float>(R * V); w.hn = a.take<float>(R * V);
    w.big = a.take<float>(R * vocos_wide(c)); w.spec = a.take<float>(R * c->vcfg.n_fft);
    return w;
}
// HiFi-GAN: frames and channels per level (0 = conv_pre's output, s + 1 = after upsampler s) and the largest [C][T] plane
struct HifiPlan { int Ts[VV_MAX_UP + 1], Cs[VV_MAX_UP + 1]; size_t big; };
static HifiPlan hifi_plan(const vv_model_cfg& g, int t_gen_max) {
    HifiPlan p;
    p.Ts[0] = t_gen_max; p.Cs[0] = g.voc_pre_ch; p.big = (size_t)p.Cs[0] * p.Ts[0];
    for (int s = 0; s < g.voc_n_up; ++s) { p.Ts[s + 1] = p.Ts[s] * g.voc_up_rates[s]; p.Cs[s + 1] = p.Cs[s] / 2; p.big = std::max(p.big, (size_t)p.Cs[s + 1] * p.Ts[s + 1]); }
    return p;
}
// the mel slice, five rotating [B][big] planes, the lengths of every level
struct HifiBufs { float *v0, *buf[5]; int* lens; };
static HifiBufs hifi_bufs(Arena& a, const vv_model_cfg& g, const HifiPlan& p, int B) {
    HifiBufs w{a.take<float>((size_t)B * g.n_mel * p.Ts[0])};
    for (float*& b : w.buf) b = a.take<float>((size_t)B * p.big);
    w.lens = a.take<int>((size_t)(g.voc_n_up + 1) * B);
    return w;
}

int vv_decode_ws_bytes(vv_ctx* c, int B, int t_gen_max, uint64_t* bytes) {
    if (!c || !bytes || B < 1 || t_gen_max < 1) return c ? c->fail(-22, "vv_decode_ws_bytes: bad arguments") : -22;
    Arena dry;
    if (c->vocos) vocos_bufs(dry, c, B, t_gen_max); else hifi_bufs(dry, c->cfg, hifi_plan(c->cfg, t_gen_max), B);
    *bytes = (uint64_t)align_up(dry.off, 256);
    return 0;
}

uint64_t vv_ws_generation(const vv_ctx* c) { return c ? c->ws_generation : 0; }

// ---- N6 Vocos.  Every GEMM is fp32 on the pinned 128 x 128 tiling: a row's arithmetic is then the same whatever
// the batch (M) it shares a launch with.
static Gemm vocos_gemm(const vv_ctx* c, int mode, int act, const float* A, int lda, const char* wn, const char* bn, float* C, int ldc, int M, int N, int K) {
    Gemm g = gemm_args(c, VV_DTYPE_F32, VV_DTYPE_F32, mode, act, A, lda, wn, K, bn, C, ldc, M, N, K);
    g.tile = 128; g.chip_share = 1;
    return g;
}

static int vocos_ln(vv_ctx* c, const float* x, float* y, int R, const std::string& n, hipStream_t st) {
    vv_ln_args a{};
    a.out_dtype = VV_DTYPE_F32; a.x = x; a.ldx = c->vcfg.dim; a.y = y; a.ldy = c->vcfg.dim; a.R = R; a.D = c->vcfg.dim;
    a.w = c->Wf(n + ".weight"); a.b = c->Wf(n + ".bias"); a.add_one = 0; a.eps = c->vcfg.ln_eps;
    Prof p(c, VV_PROF_VOC_CONV, 0, 8.0 * R * c->vcfg.dim, st);
    KCHK(c, vvk_ln_mod(&a, st, &m__));
    return 0;
}

// The ISTFT head after the head GEMM: head [B * T_max][ld_head] -> spectrum operand -> windowed frames (one K = n_fft GEMM against
// const.istft_basis) -> overlap-add / envelope / trim / int16.  spec and frames: [B * T_max][n_fft] scratch.
static int vocos_istft(vv_ctx* c, int B, int T_max, const float* head, int ld_head, const int* lens, int16_t* pcm, int ld_pcm, int32_t* pcm_len,
                       float* wave, float* spec, float* frames, hipStream_t st) {
    const int n = c->vcfg.n_fft, hop = c->vcfg.hop_length, R = B * T_max;
    {
        Prof p(c, VV_PROF_VOC_POST, 0, 4.0 * R * ((double)n + 2 + n), st);
        KCHK(c, vvk_vocos_spectrum(head, ld_head, R, n, spec, st, &m__));
    }
    if (int r = launch_gemm(c, vocos_gemm(c, VV_EPI_STORE, VV_ACT_NONE_, spec, n, "const.istft_basis", nullptr, frames, n, R, n, n), VV_PROF_VOC_POST, st)) return r;
    Prof p(c, VV_PROF_VOC_POST, 0, 4.0 * R * (double)n + 6.0 * B * (double)T_max * hop, st);
    KCHK(c, vvk_vocos_ola(frames, n, B, T_max, lens, c->Wf("const.window"), n, hop, pcm, ld_pcm, pcm_len, wave, T_max * hop, st, &m__));
    return 0;
}

static int decode_vocos(vv_ctx* c, int B, int N, const float* x, const int32_t* ref_len, const int32_t* seq_len, int T_max, int16_t* pcm,
                        int ld_pcm, int32_t* pcm_len, float* wave_f32, void* ext_ws, uint64_t ext_bytes, hipStream_t st) {
    const vv_vocos_cfg& v = c->vcfg;
    const int M = c->cfg.n_mel, V = v.dim, I = v.intermediate, KE = pad_to(v.embed_k * M, 32), HP = pad_to(v.n_fft + 2, 128);
    if ((size_t)B * T_max * vocos_wide(c) * 4 >= ((size_t)1 << 31)) return c->fail(-22, "vv_decode: a Vocos plane of 2 GiB or more (split the batch)");
    const int R = B * T_max;
    VocosBufs w;
    if (int r = plan_ws(c, ext_ws, (size_t)ext_bytes, [&](Arena& a) { w = vocos_bufs(a, c, B, T_max); })) return r;
    auto [lens, res, t, hn, big, spec] = w;
    KCHK(c, vvk_vocos_lens(seq_len, ref_len, lens, B, N, T_max, st, &m__));
    {
        Prof p(c, VV_PROF_VOC_CONV, 0, 4.0 * R * ((double)M + KE), st);
        KCHK(c, vvk_vocos_im2col(x, B, N, M, ref_len, seq_len, T_max, v.embed_k, big, KE, st, &m__));
    }
    if (int r = launch_gemm(c, vocos_gemm(c, VV_EPI_STORE, VV_ACT_NONE_, big, KE, "voc.embed.weight", "voc.embed.bias", t, V, R, V, KE), VV_PROF_VOC_CONV, st)) return r;
    if (int r = vocos_ln(c, t, res, R, "voc.norm", st)) return r;
    for (int i = 0; i < v.layers; ++i) {
        const std::string p = "voc.blocks." + std::to_string(i);
        {
            Prof pr(c, VV_PROF_VOC_CONV, 2.0 * R * (double)V * v.dw_k, 8.0 * R * V, st);
            KCHK(c, vvk_dwconv(res, t, c->Wf(p + ".dwconv.weight"), c->Wf(p + ".dwconv.bias"), lens, B, B, T_max, V, v.dw_k, st, &m__));
        }
        if (int r = vocos_ln(c, t, hn, R, p + ".norm", st)) return r;
        const std::string w1 = p + ".pwconv1.weight", b1 = p + ".pwconv1.bias", w2 = p + ".pwconv2.weight", b2 = p + ".pwconv2.bias";
        if (int r = launch_gemm(c, vocos_gemm(c, VV_EPI_STORE, VV_ACT_GELU_ERF_, hn, V, w1.c_str(), b1.c_str(), big, I, R, I, V), VV_PROF_VOC_CONV, st)) return r;
        Gemm g2 = vocos_gemm(c, VV_EPI_GATE_RES, VV_ACT_NONE_, big, I, w2.c_str(), b2.c_str(), res, V, R, V, I);
        g2.gate = c->Wf(p + ".gamma");
        if (int r = launch_gemm(c, g2, VV_PROF_VOC_CONV, st)) return r;
    }
    if (int r = vocos_ln(c, res, hn, R, "voc.final_norm", st)) return r;
    Gemm head = vocos_gemm(c, VV_EPI_STORE, VV_ACT_NONE_, hn, V, "voc.head.weight", "voc.head.bias", big, HP, R, HP, V);
    head.n_store = v.n_fft + 2;
    if (int r = launch_gemm(c, head, VV_PROF_VOC_POST, st)) return r;
    return vocos_istft(c, B, T_max, big, HP, lens, pcm, ld_pcm, pcm_len, wave_f32, spec, big, st);
}

static int decode_impl(vv_ctx* c, int B, int N, const float* x, const int32_t* ref_len, const int32_t* seq_len, int t_gen_max, int16_t* pcm,
                       int ld_pcm, int32_t* pcm_len, float* wave_f32, void* ext_ws, uint64_t ext_bytes, void* stream) {
    if (!c) return -22;
    if (!c->finalized) return c->fail(-1, "vv_decode: weights not finalized");
    if (B < 1 || N < 1 || !x || !ref_len || !seq_len || !pcm || !pcm_len || t_gen_max < 1 || t_gen_max > N)
        return c->fail(-22, "vv_decode: bad arguments");
    const vv_model_cfg& g = c->cfg;
    if (ld_pcm < t_gen_max * g.hop_length) return c->fail(-22, "vv_decode: ld_pcm too small");
    hipSetDevice(c->device);
    hipStream_t st = (hipStream_t)stream;
    if (c->vocos) return decode_vocos(c, B, N, x, ref_len, seq_len, t_gen_max, pcm, ld_pcm, pcm_len, wave_f32, ext_ws, ext_bytes, st);
    const int M = g.n_mel, nu = g.voc_n_up;
    const HifiPlan plan = hifi_plan(g, t_gen_max);
    const int *Ts = plan.Ts, *Cs = plan.Cs;
    HifiBufs w;
    if (int r = plan_ws(c, ext_ws, (size_t)ext_bytes, [&](Arena& a) { w = hifi_bufs(a, g, plan, B); })) return r;
    auto [v0, buf, lens] = w;

    KCHK(c, vvk_decode_len(seq_len, ref_len, lens, B, nu + 1, c->d_mult, N, Ts[0], st, &m__));
    HIPCHK(c, hipMemcpyAsync(pcm_len, lens + (size_t)nu * B, sizeof(int) * B, hipMemcpyDeviceToDevice, st));
    {
        Prof p(c, VV_PROF_ELEMWISE, 0, 8.0 * B * M * Ts[0], st);
        KCHK(c, vvk_mel_slice(x, B, N, M, ref_len, seq_len, v0, Ts[0], st, &m__));
    }
    const bool x3 = c->voc_x3 == 1 || (c->voc_x3 < 0 && c->dt == VV_DTYPE_BF16);
    auto conv = [&](const float* in, const std::string& name, float* out, const float* resid, int Cin, int Cout, int T_in, int T_out, int KW,
                    int dil, int up, float pre_slope, float scale, int accumulate, const int* len_in, int stage_cls) -> int {
        vv_conv_args a{};
        a.in = in; a.W = c->Wf(name + ".weight"); a.bias = c->Wf(name + ".bias"); a.out = out; a.resid = resid;
        if (x3) {
            auto it = c->x3_w.find(name + ".weight");
            if (it == c->x3_w.end()) return c->fail(-2, "split weights of %s missing", name.c_str());
            a.W_x3 = it->second; a.wg_rows = c->voc_x3_rows;
        }
        a.B = B; a.Cin = Cin; a.Cout = Cout; a.T_in = T_in; a.T_out = T_out; a.KW = KW; a.dil = dil; a.transposed = up > 0; a.up = up;
        a.rows_total = up > 0 ? Cout * up : Cout; a.rows_pad = pad_to(a.rows_total, 64); a.accumulate = accumulate;
        a.pre_slope = pre_slope; a.out_scale = scale; a.len_in = len_in;
        const double taps = up > 0 ? 2.0 : (double)KW;
        Prof p(c, VV_PROF_VOC_CONV, 2.0 * B * (double)T_out * Cout * Cin * taps,
               4.0 * B * ((double)Cin * T_in + (double)Cout * T_out * (1 + (resid ? 1 : 0) + (accumulate ? 1 : 0))), st, stage_cls);
        const char* m = "";
        int r = vvk_conv(&a, st, &m);
        if (r) return c->fail(r, "%s (%s)", m, name.c_str());
        return 0;
    };
    if (int r = conv(v0, "voc.pre", buf[0], nullptr, M, Cs[0], Ts[0], Ts[0], g.voc_pre_k, 1, 0, 1.0f, 1.0f, 0, lens, VV_PROF_VOC_PRE)) return r;
    float* cur = buf[0];
    float* up_out = buf[1];
    for (int s = 0; s < nu; ++s) {
        const int C = Cs[s + 1], T = Ts[s + 1];
        const int* len_s = lens + (size_t)(s + 1) * B;
        if (int r = conv(cur, "voc.up." + std::to_string(s), up_out, nullptr, Cs[s], C, Ts[s], T, 2, 1, g.voc_up_rates[s], g.voc_lrelu, 1.0f, 0, lens + (size_t)s * B,
                         s < 4 ? VV_PROF_VOC_UP0 + s : -1)) return r;
        // MRF: acc = (1/n_res) * sum_a resblock_a(up_out)
        float* acc = cur;                                   // the previous stage's input is dead now: the sum lands there and is the next stage's input
        float* t1 = (up_out == buf[1]) ? buf[2] : buf[1];
        float* ya = buf[3];
        float* yb = buf[4];
        const float inv = 1.0f / (float)g.voc_n_res;
        const int mrf_cls = s < 4 ? VV_PROF_VOC_MRF0 + s : -1;
        for (int a = 0; a < g.voc_n_res; ++a) {
            const float* y = up_out;
            for (int b = 0; b < g.voc_n_dil; ++b) {
                const std::string q = "voc.res." + std::to_string(s) + "." + std::to_string(a) + "." + std::to_string(b);
                const bool last = b == g.voc_n_dil - 1;
                float* dst = last ? acc : ((y == ya) ? yb : ya);
                const int kw = g.voc_res_kernels[a], dil = g.voc_res_dilations[b];
                // (the fused pair exists on the f32 instruction only: with x3 products the two x3 launches are taken unless fusion is forced)
                if ((c->fuse_mrf == 1 || (c->fuse_mrf == 2 && B <= 8 && !x3)) && (C == 32 || C == 64) && (kw == 3 || kw == 7 || kw == 11)) {
                    // K12 fused through LDS: the intermediate of the pair never reaches HBM (bit-identical to the two launches below)
                    vv_mrf_args m{};
                    m.y = y; m.W1 = c->Wf(q + ".conv1.weight"); m.b1 = c->Wf(q + ".conv1.bias"); m.W2 = c->Wf(q + ".conv2.weight"); m.b2 = c->Wf(q + ".conv2.bias");
                    m.out = dst; m.B = B; m.C = C; m.T = T; m.KW = kw; m.dil = dil; m.rows_pad = 64; m.accumulate = last && a > 0;
                    m.slope = g.voc_lrelu; m.out_scale = last ? inv : 1.0f; m.len_in = len_s;
                    Prof p(c, VV_PROF_VOC_CONV, 2.0 * 2.0 * B * (double)T * C * C * kw, 4.0 * B * (double)C * T * (2 + (m.accumulate ? 1 : 0)), st, mrf_cls);
                    const char* em = "";
                    if (int r = vvk_mrf_pair(&m, st, &em)) return c->fail(r, "%s (%s)", em, q.c_str());
                } else {
                    if (int r = conv(y, q + ".conv1", t1, nullptr, C, C, T, T, kw, dil, 0, g.voc_lrelu, 1.0f, 0, len_s, mrf_cls)) return r;
                    if (int r = conv(t1, q + ".conv2", dst, y, C, C, T, T, kw, 1, 0, g.voc_lrelu, last ? inv : 1.0f, last && a > 0, len_s, mrf_cls)) return r;
                }
                y = dst;
            }
        }
    }
    {
        const int C = Cs[nu], T = Ts[nu];
        Prof p(c, VV_PROF_VOC_POST, 2.0 * B * (double)T * C * g.voc_post_k, 4.0 * B * (double)C * T + 2.0 * B * T, st);
        KCHK(c, vvk_conv_post(cur, c->Wf("voc.post.weight"), c->post_bias, pcm, ld_pcm, wave_f32, B, C, T, g.voc_post_k, 0.01f,
                              lens + (size_t)nu * B, st, &m__));
    }
    return 0;
}

int vv_set_rope_theta(vv_ctx* c, float theta) {
    if (!c) return -22;
    if (theta != 0.f && !(theta > 1.f)) return c->fail(-22, "vv_set_rope_theta: the base must be > 1 (0 = read the tables)");
    c->rope_theta = theta;
    return 0;
}

int vv_set_option(vv_ctx* c, const char* name, int value) {
    if (!c || !name) return -22;
    if (!strcmp(name, "rope_rows")) { c->rope_rows = value != 0; return 0; }
    if (!strcmp(name, "rope_q_attn")) { c->rope_q_attn = value != 0; return 0; }
    if (!strcmp(name, "voc_x3_rows")) {
        if (value != 0 && value != 128) return c->fail(-22, "vv_set_option: voc_x3_rows takes 0 (64-row workgroups) or 128");
        c->voc_x3_rows = value; return 0;
    }
    if (!strcmp(name, "voc_x3")) {
        if (value < -1 || value > 1) return c->fail(-22, "vv_set_option: voc_x3 takes -1 (by acoustic dtype), 0 (f32 MFMA) or 1 (3-way bf16 split)");
        c->voc_x3 = value; return 0;
    }
    if (!strcmp(name, "split_k_tail")) {
        if (value < 0 || value > 2) return c->fail(-22, "vv_set_option: split_k_tail takes 0 (off), 1 (out-projection and FF2) or 2 (FF2 only)");
        c->split_k_tail = value; return 0;
    }
    if (!strcmp(name, "ring_tiles")) { c->ring_tiles = value != 0; if (value > 1) c->ring_tiles_max = value; return 0; }
    if (!strcmp(name, "pp_min_tiles")) {
        if (value < -1) return c->fail(-22, "vv_set_option: pp_min_tiles takes -1 (the launcher's rule) or a 256-tile count >= 0");
        c->pp_min_tiles = value; return 0;
    }
    if (!strcmp(name, "lanes")) {
        if (value < 0 || value > 2) return c->fail(-22, "vv_set_option: lanes takes 0 (auto), 1 (one lane) or 2 (two lanes whenever the batch has two items)");
        c->lanes = value; return 0;
    }
    if (!strcmp(name, "fuse_mrf")) {
        if (value < 0 || value > 2) return c->fail(-22, "vv_set_option: fuse_mrf takes 0 (off), 1 (on) or 2 (auto)");
        c->fuse_mrf = value; return 0;
    }
    return c->fail(-22, "vv_set_option: unknown option '%s'", name);
}

int vv_decode(vv_ctx* c, int B, int N, const float* x, const int32_t* ref_len, const int32_t* seq_len, int t_gen_max, int16_t* pcm,
              int ld_pcm, int32_t* pcm_len, float* wave_f32, void* stream) {
    return decode_impl(c, B, N, x, ref_len, seq_len, t_gen_max, pcm, ld_pcm, pcm_len, wave_f32, nullptr, 0, stream);
}

// Same stage with every intermediate in a CALLER-OWNED block of vv_decode_ws_bytes() bytes: nothing the launches point at can
// be moved by a later call that grows the context arena, so the launch sequence may be captured into a hipGraph and replayed
// for the lifetime of that block (reference has no counterpart; BASELINE.json configs[4] "hipGraph-captured vocoder step").
int vv_decode_into(vv_ctx* c, int B, int N, const float* x, const int32_t* ref_len, const int32_t* seq_len, int t_gen_max, int16_t* pcm,
                   int ld_pcm, int32_t* pcm_len, float* wave_f32, void* ws, uint64_t ws_bytes, void* stream) {
    if (!c) return -22;
    if (!ws) return c->fail(-22, "vv_decode_into: null workspace block");
    return decode_impl(c, B, N, x, ref_len, seq_len, t_gen_max, pcm, ld_pcm, pcm_len, wave_f32, ws, ws_bytes, stream);
}

// ------------------------------------------------------------------------------------ profiling
int vv_prof_enable(vv_ctx* c, int on) {
    if (!c) return -22;
    c->prof = on != 0;
    return 0;
}
int vv_prof_collect(vv_ctx* c, int64_t* launches, double* ms, double* flops, double* bytes) {
    if (!c) return -22;
    hipSetDevice(c->device);
    HIPCHK(c, hipDeviceSynchronize());
    for (auto& r : c->recs) {
        float t = 0.f;
        if (hipEventElapsedTime(&t, r.a, r.b) == hipSuccess) { c->p_ms[r.cls] += t; if (r.sub >= 0) c->p_ms[r.sub] += t; }
        c->pool.push_back(r.a); c->pool.push_back(r.b);
    }
    c->recs.clear();
    for (int i = 0; i < VV_PROF_NCLASS; ++i) {
        if (launches) launches[i] = c->p_launch[i];
        if (ms) ms[i] = c->p_ms[i];
        if (flops) flops[i] = c->p_flops[i];
        if (bytes) bytes[i] = c->p_bytes[i];
        c->p_launch[i] = 0; c->p_ms[i] = 0; c->p_flops[i] = 0; c->p_bytes[i] = 0;
    }
    return 0;
}

// ----------------------------------------------------------------------- single-kernel entries
#define SINGLE(ctx, call)                                     \
    do {                                                      \
        if (!(ctx)) return -22;                               \
        hipSetDevice((ctx)->device);                          \
        const char* m__ = "";                                 \
        int r__ = (call);                                     \
        if (r__) return (ctx)->fail(r__, "%s", m__);          \
        return 0;                                             \
    } while (0)

int vv_gemm(vv_ctx* c, const vv_gemm_args* a, void* st) { SINGLE(c, vvk_gemm(a, (hipStream_t)st, &m__)); }
int vv_gemm_tail_plan(vv_ctx* c, int32_t M, int32_t N, int32_t K, int32_t* row0, int32_t* parts) {
    // ctx may be NULL: the plan for the process's current device (256 CUs when there is none), so that planner / launcher
    // consistency can be checked without a GPU.  Operands are taken as contiguous (lda = ldw = K, ldc = N).
    if (!row0 || !parts || M < 1 || N < 1 || K < 1) return c ? c->fail(-22, "vv_gemm_tail_plan: bad arguments") : -22;
    if (c) HIPCHK(c, hipSetDevice(c->device));
    vvk_gemm_tail_plan(M, N, K, K, K, N, row0, parts);
    return 0;
}
int vv_attention(vv_ctx* c, const vv_attn_args* a, void* st) { SINGLE(c, vvk_attention(a, (hipStream_t)st, &m__)); }
int vv_layernorm(vv_ctx* c, const vv_ln_args* a, void* st) { SINGLE(c, vvk_ln_mod(a, (hipStream_t)st, &m__)); }
int vv_posconv(vv_ctx* c, const vv_posconv_args* a, void* st) { SINGLE(c, vvk_posconv(a, (hipStream_t)st, &m__)); }
int vv_conv1d(vv_ctx* c, const vv_conv_args* a, void* st) { SINGLE(c, vvk_conv(a, (hipStream_t)st, &m__)); }
uint64_t vv_conv_split_bytes(int32_t Cin_pad, int32_t KW, int32_t rows_pad) {
    return (Cin_pad < 1 || KW < 1 || rows_pad < 1) ? 0 : (uint64_t)vvk_conv_split_bytes(Cin_pad, KW, rows_pad);
}
int vv_conv_split_weights(vv_ctx* c, const float* W, int32_t Cin_pad, int32_t KW, int32_t rows_pad, void* out, void* st) {
    SINGLE(c, vvk_conv_split_weights(W, Cin_pad, KW, rows_pad, out, (hipStream_t)st, &m__));
}
int vv_mrf_resblock(vv_ctx* c, const vv_mrf_args* a, void* st) { SINGLE(c, vvk_mrf_pair(a, (hipStream_t)st, &m__)); }
int vv_conv_post(vv_ctx* c, const float* in, const float* w, float bias, int16_t* pcm, int ld_pcm, float* wave_f32, int B, int C, int T,
                 int KW, float pre_slope, const int32_t* len_in, void* st) {
    SINGLE(c, vvk_conv_post(in, w, bias, pcm, ld_pcm, wave_f32, B, C, T, KW, pre_slope, len_in, (hipStream_t)st, &m__));
}
int vv_mel(vv_ctx* c, const int16_t* audio, int ld_audio, const int32_t* audio_len, float* mel, int B, int F_max, void* st) {
    if (!c) return -22;
    if (!c->W("const.window") || !c->W("const.tw_cos") || !c->W("const.tw_sin") || !c->W("const.mel_fb"))
        return c->fail(-2, "vv_mel: constant tables not bound");
    SINGLE(c, vvk_mel(audio, ld_audio, audio_len, c->Wf("const.window"), c->Wf("const.tw_cos"), c->Wf("const.tw_sin"), c->Wf("const.mel_fb"),
                      mel, B, F_max, c->cfg.n_fft, c->cfg.hop_length, c->cfg.n_mel, (hipStream_t)st, &m__));
}
int vv_groupnorm(vv_ctx* c, const float* x, float* y, const float* gamma, const float* beta, int B, int C, int T, int G, float eps, int act, void* st) {
    SINGLE(c, vvk_groupnorm(x, y, gamma, beta, B, C, T, G, eps, act, (hipStream_t)st, &m__));
}
int vv_rope_rows(vv_ctx* c, const float* compact, const int32_t* pos, float* out, int rows, void* st) {
    SINGLE(c, vvk_rope_rows(compact, pos, out, rows, (hipStream_t)st, &m__));
}
int vv_rope_compact(vv_ctx* c, const float* cos_t, const float* sin_t, float* out, int n, void* st) {
    SINGLE(c, vvk_rope_compact(cos_t, sin_t, out, n, (hipStream_t)st, &m__));
}
int vv_resample_poly(vv_ctx* c, const float* x, int n_in, const double* taps, int n_taps, int up, int down, int skip, float* y, int n_out, void* st) {
    SINGLE(c, vvk_resample_poly(x, n_in, taps, n_taps, up, down, skip, y, n_out, (hipStream_t)st, &m__));
}
int vv_ingest_pcm(vv_ctx* c, const void* pcm, const int64_t* desc, int n_clips, int64_t max_out, float* out, void* st) {
    SINGLE(c, vvk_ingest_pcm(pcm, (const long long*)desc, n_clips, (long long)max_out, out, (hipStream_t)st, &m__));
}
size_t vv_normalize_scratch_bytes(int n_clips, int64_t total_len) { return vvk_normalize_scratch_bytes(n_clips, (long long)total_len); }
int vv_normalize_clips(vv_ctx* c, const float* x, const int64_t* offsets, int n_clips, int64_t max_len, void* scratch, int16_t* out, void* st) {
    SINGLE(c, vvk_normalize_clips(x, (const long long*)offsets, n_clips, (long long)max_len, scratch, out, (hipStream_t)st, &m__));
}
int vv_vocos_im2col(vv_ctx* c, const float* x, int B, int N, const int32_t* ref_len, const int32_t* seq_len, int T_max, float* out, int ld_out,
                    void* st) {
    if (c && !c->vocos) return c->fail(-22, "vv_vocos_im2col: not a Vocos context (vv_set_vocos)");
    SINGLE(c, vvk_vocos_im2col(x, B, N, c->cfg.n_mel, ref_len, seq_len, T_max, c->vcfg.embed_k, out, ld_out, (hipStream_t)st, &m__));
}
int vv_istft_head(vv_ctx* c, int B, int T_max, const float* head, int ld_head, const int32_t* n_frames, int16_t* pcm, int ld_pcm, int32_t* pcm_len,
                  float* wave_f32, void* stream) {
    if (!c) return -22;
    if (!c->vocos || !c->finalized) return c->fail(-22, "vv_istft_head: needs a finalized Vocos context");
    if (B < 1 || T_max < 1 || !head || !n_frames || !pcm || ld_head < c->vcfg.n_fft + 2 || ld_pcm < T_max * c->vcfg.hop_length)
        return c->fail(-22, "vv_istft_head: bad arguments (ld_head >= n_fft + 2, ld_pcm >= T_max * hop)");
    if ((size_t)B * T_max * c->vcfg.n_fft * 4 >= ((size_t)1 << 31)) return c->fail(-22, "vv_istft_head: a plane of 2 GiB or more");
    hipSetDevice(c->device);
    const size_t R = (size_t)B * T_max;
    float *spec, *frames;                                // the spectrum operand and the windowed frames, [B * T_max][n_fft] each
    if (int r = plan_ws(c, nullptr, 0, [&](Arena& a) { spec = a.take<float>(R * c->vcfg.n_fft); frames = a.take<float>(R * c->vcfg.n_fft); })) return r;
    return vocos_istft(c, B, T_max, head, ld_head, n_frames, pcm, ld_pcm, pcm_len, wave_f32, spec, frames, (hipStream_t)stream);
}
int vv_ode_stage(vv_ctx* c, const vv_ode_stage_args* a, void* st) {
    if (!c || !a) return c ? c->fail(-22, "vv_ode_stage: null arguments") : -22;
    SINGLE(c, vvk_ode_stage(a, nullptr, nullptr, (hipStream_t)st, &m__));
}
int vv_ode_stage_guided(vv_ctx* c, const vv_ode_stage_args* a, const int32_t* u_row, void* st) {
    if (!c || !a) return c ? c->fail(-22, "vv_ode_stage_guided: null arguments") : -22;
    if ((uintptr_t)u_row % 4) return c->fail(-22, "vv_ode_stage_guided: u_row must be an int32 array");
    SINGLE(c, vvk_ode_stage(a, u_row, nullptr, (hipStream_t)st, &m__));
}
int vv_ode_stage_apg(vv_ctx* c, const vv_ode_stage_args* a, const int32_t* u_row, const vv_apg_stage_args* apg, void* st) {
    if (!apg) return vv_ode_stage_guided(c, a, u_row, st);
    if (!c || !a) return c ? c->fail(-22, "vv_ode_stage_apg: null arguments") : -22;
    if ((uintptr_t)u_row % 4) return c->fail(-22, "vv_ode_stage_apg: u_row must be an int32 array");
    SINGLE(c, vvk_ode_stage(a, u_row, apg, (hipStream_t)st, &m__));
}
int vv_ode_stage_reuse(vv_ctx* c, const vv_ode_stage_args* a, const int32_t* u_row, const vv_reuse_stage_args* reuse, void* st) {
    if (!reuse) return vv_ode_stage_guided(c, a, u_row, st);
    if (!c || !a) return c ? c->fail(-22, "vv_ode_stage_reuse: null arguments") : -22;
    if ((uintptr_t)u_row % 4) return c->fail(-22, "vv_ode_stage_reuse: u_row must be an int32 array");
    SINGLE(c, vvk_ode_stage(a, u_row, nullptr, (hipStream_t)st, &m__, 0, reuse));
}
int vv_block_span(vv_ctx* c, const vv_block_span_args* a, void* st) {
    if (!c || !a) return c ? c->fail(-22, "vv_block_span: null arguments") : -22;
    SINGLE(c, vvk_block_span(a, (hipStream_t)st, &m__));
}
int vv_block_drift_reduce(vv_ctx* c, const vv_block_drift_args* a, void* st) {
    if (!c || !a) return c ? c->fail(-22, "vv_block_drift_reduce: null arguments") : -22;
    SINGLE(c, vvk_block_drift_reduce(a, 3, (hipStream_t)st, &m__));
}
int vv_cfg_drift_reduce(vv_ctx* c, const vv_cfg_drift_args* a, void* st) {
    if (!c || !a) return c ? c->fail(-22, "vv_cfg_drift_reduce: null arguments") : -22;
    if (((uintptr_t)a->u_row | (uintptr_t)a->row_start | (uintptr_t)a->len) % 4) return c->fail(-22, "vv_cfg_drift_reduce: the index arrays must be 4-byte aligned");
    SINGLE(c, vvk_cfg_drift_reduce(a, 3, (hipStream_t)st, &m__));
}
int vv_ode_diff_reduce(vv_ctx* c, const vv_ode_diff_args* a, void* st) {
    if (!c || !a) return c ? c->fail(-22, "vv_ode_diff_reduce: null arguments") : -22;
    if (((uintptr_t)a->row_start | (uintptr_t)a->len) % 4) return c->fail(-22, "vv_ode_diff_reduce: the index arrays must be 4-byte aligned");
    SINGLE(c, vvk_ode_diff_reduce(a, 3, (hipStream_t)st, &m__));
}
int vv_apg_coef(vv_ctx* c, const vv_apg_coef_args* a, void* st) {
    if (!c || !a) return c ? c->fail(-22, "vv_apg_coef: null arguments") : -22;
    if (((uintptr_t)a->u_row | (uintptr_t)a->row_src | (uintptr_t)a->row_start | (uintptr_t)a->len | (uintptr_t)a->g_item | (uintptr_t)a->eta |
         (uintptr_t)a->norm_rms) % 4)
        return c->fail(-22, "vv_apg_coef: the index and item arrays must be 4-byte aligned");
    SINGLE(c, vvk_apg_coef(a, 3, (hipStream_t)st, &m__));
}
int vv_cfg_norm_coef(vv_ctx* c, const vv_cfg_norm_coef_args* a, void* st) {
    if (!c || !a) return c ? c->fail(-22, "vv_cfg_norm_coef: null arguments") : -22;
    if (((uintptr_t)a->u_row | (uintptr_t)a->row_start | (uintptr_t)a->len | (uintptr_t)a->g_item | (uintptr_t)a->star | (uintptr_t)a->rescale) % 4)
        return c->fail(-22, "vv_cfg_norm_coef: the index and item arrays must be 4-byte aligned");
    SINGLE(c, vvk_cfg_norm_coef(a, 3, (hipStream_t)st, &m__));
}
int vv_ode_stage_norm(vv_ctx* c, const vv_ode_stage_args* a, const int32_t* u_row, const float* coef, void* st) {
    if (!coef) return vv_ode_stage_guided(c, a, u_row, st);
    if (!c || !a) return c ? c->fail(-22, "vv_ode_stage_norm: null arguments") : -22;
    if ((uintptr_t)u_row % 4) return c->fail(-22, "vv_ode_stage_norm: u_row must be an int32 array");
    SINGLE(c, vvk_ode_stage(a, u_row, nullptr, (hipStream_t)st, &m__, 0, nullptr, coef));
}
// single-kernel entries (unit parity) of the text stack: the checks live here, the stages call the launchers with operands they own
int vv_text_embed(vv_ctx* c, const int32_t* ids, int ld_ids, const int32_t* text_len, const float* emb, const float* pos, int vocab_rows,
                  float* out, int B, int N, int Dt, void* st) {
    if (!c) return -22;
    if (!ids || !text_len || !emb || !pos || !out || B < 1 || N < 1 || ld_ids < 1 || vocab_rows < 1 || Dt < 4 || Dt % 4)
        return c->fail(-22, "vv_text_embed: bad arguments (B, N, ld_ids, vocab_rows >= 1, Dt a multiple of 4)");
    if (((uintptr_t)emb | (uintptr_t)pos | (uintptr_t)out) % 16 || ((uintptr_t)ids | (uintptr_t)text_len) % 4)
        return c->fail(-22, "vv_text_embed: emb, pos and out must be 16-byte aligned, ids and text_len 4-byte");
    SINGLE(c, vvk_text_embed(ids, ld_ids, text_len, emb, pos, out, B, N, Dt, vocab_rows, (hipStream_t)st, &m__));
}
int vv_dwconv(vv_ctx* c, const float* in, float* out, const float* w, const float* bias, const int32_t* seq_len, int B, int n_seq, int N, int C,
              int KW, void* st) {
    if (!c) return -22;
    if (!in || !out || !w || !bias || in == out || n_seq < 1 || N < 1 || C < 4 || C % 4 || KW < 1 || !(KW & 1) || (seq_len && B < 1))
        return c->fail(-22, "vv_dwconv: bad arguments (out a buffer of its own, C a multiple of 4, KW odd, B >= 1 with seq_len)");
    if (((uintptr_t)in | (uintptr_t)out | (uintptr_t)bias) % 16 || ((uintptr_t)w | (uintptr_t)seq_len) % 4)
        return c->fail(-22, "vv_dwconv: in, out and bias must be 16-byte aligned, w and seq_len 4-byte");
    SINGLE(c, vvk_dwconv(in, out, w, bias, seq_len, seq_len ? B : 1, n_seq, N, C, KW, (hipStream_t)st, &m__));
}
int vv_grn(vv_ctx* c, int dtype, void* x, float* sumsq, const float* gamma, const float* beta, const int32_t* seq_len, int B, int n_seq, int N,
           int C, void* st) {
    if (!c) return -22;
    if ((dtype != VV_DTYPE_F32 && dtype != VV_DTYPE_BF16) || !x || !sumsq || !gamma || !beta || n_seq < 1 || N < 1 || C < 64 || C % 64 || C > 8192 ||
        (seq_len && B < 1))
        return c->fail(-22, "vv_grn: bad arguments (dtype f32 / bf16, C a multiple of 64 up to 8192, B >= 1 with seq_len)");
    if ((uintptr_t)x % (dtype == VV_DTYPE_BF16 ? 8 : 16) || (uintptr_t)beta % 16 || ((uintptr_t)sumsq | (uintptr_t)gamma | (uintptr_t)seq_len) % 4)
        return c->fail(-22, "vv_grn: x must be aligned to 4 elements, beta to 16 bytes, sumsq, gamma and seq_len to 4");
    SINGLE(c, vvk_grn(dtype, x, sumsq, gamma, beta, seq_len, seq_len ? B : 1, n_seq, N, C, (hipStream_t)st, &m__));
}
int vv_cfg_euler(vv_ctx* c, float* x, const float* pred, int ldp, int BN, int n_mel, float cfg, float dt, void* st) {
    SINGLE(c, vvk_cfg_euler(x, pred, ldp, BN, n_mel, cfg, dt, nullptr, (hipStream_t)st, &m__));
}
// single-kernel entries (unit parity) of the sampler, pack and waveform-head kernels: the launchers hold the checks the stages also pass;
// what only a caller from outside can get wrong (an array that is not 4-byte aligned, a dtype code) is checked here
#define ALIGN4(ctx, name, ptrs)                                                                                   \
    do {                                                                                                              \
        if (!(ctx)) return -22;                                                                                       \
        if ((ptrs) % 4) return (ctx)->fail(-22, name ": every array must be 4-byte aligned");                    \
    } while (0)
int vv_cfg_euler_rows(vv_ctx* c, float* x, const float* pred, int ldp, int BN, int n_mel, float cfg, float dt, const int32_t* row_src, void* st) {
    ALIGN4(c, "vv_cfg_euler_rows", (uintptr_t)row_src);
    SINGLE(c, vvk_cfg_euler(x, pred, ldp, BN, n_mel, cfg, dt, row_src, (hipStream_t)st, &m__));
}
int vv_pack_cat(vv_ctx* c, int dtype, const float* x, const float* cat, const float* cat_drop, void* out, int ldo, int BN, int n_mel, int cond_dim,
                int only_x, const int32_t* row_src, void* st) {
    ALIGN4(c, "vv_pack_cat", (uintptr_t)row_src);
    if (dtype != VV_DTYPE_F32 && dtype != VV_DTYPE_BF16) return c->fail(-22, "vv_pack_cat: dtype must be VV_DTYPE_F32 or VV_DTYPE_BF16");
    SINGLE(c, vvk_pack_cat(dtype, x, cat, cat_drop, out, ldo, BN, n_mel, cond_dim, only_x, row_src, (hipStream_t)st, &m__));
}
int vv_pack_cat_guided(vv_ctx* c, int dtype, const float* x, const float* cat, const float* cat_drop, void* out, int ldo, int Rc, int row0,
                       int n_rows, int n_mel, int cond_dim, int only_x, int x_packed, const int32_t* row_src, const int32_t* u_src,
                       const int32_t* u_crow, void* st) {
    ALIGN4(c, "vv_pack_cat_guided", (uintptr_t)row_src | (uintptr_t)u_src | (uintptr_t)u_crow);
    if (dtype != VV_DTYPE_F32 && dtype != VV_DTYPE_BF16) return c->fail(-22, "vv_pack_cat_guided: dtype must be VV_DTYPE_F32 or VV_DTYPE_BF16");
    SINGLE(c, vvk_pack_cat_guided(dtype, x, cat, cat_drop, out, ldo, Rc, row0, n_rows, n_mel, cond_dim, only_x, x_packed, row_src, u_src, u_crow,
                                  (hipStream_t)st, &m__));
}
int vv_row_tables(vv_ctx* c, const int32_t* seq_len, int B, int N, int Rc, int32_t* row_start, int32_t* row_src, int32_t* row_pos, int32_t* kv_len,
                  void* st) {
    ALIGN4(c, "vv_row_tables", (uintptr_t)seq_len | (uintptr_t)row_start | (uintptr_t)row_src | (uintptr_t)row_pos | (uintptr_t)kv_len);
    if (!seq_len || !row_start || !row_src || !row_pos || !kv_len) return c->fail(-22, "vv_row_tables: seq_len and the four tables are required");
    if ((long long)B * N >= (1ll << 31)) return c->fail(-22, "vv_row_tables: B * N must stay below 2^31 (row_src holds b * N + t)");
    SINGLE(c, vvk_row_tables(seq_len, B, N, Rc, row_start, row_src, row_pos, kv_len, (hipStream_t)st, &m__));
}
int vv_guided_tables(vv_ctx* c, const int32_t* seq_len, const uint8_t* guided, int B, int N, int Rc, int Ru, int32_t* row_start, int32_t* rs_rel,
                     int32_t* kv_len, int32_t* row_pos, int32_t* u_src, int32_t* u_crow, int32_t* u_row, void* st) {
    ALIGN4(c, "vv_guided_tables", (uintptr_t)seq_len | (uintptr_t)row_start | (uintptr_t)rs_rel | (uintptr_t)kv_len | (uintptr_t)row_pos |
                                          (uintptr_t)u_src | (uintptr_t)u_crow | (uintptr_t)u_row);
    if (!seq_len || !row_start || !rs_rel || !kv_len || !row_pos || !u_src || !u_crow || !u_row)
        return c->fail(-22, "vv_guided_tables: seq_len and the seven tables are required");
    if ((long long)B * N >= (1ll << 31)) return c->fail(-22, "vv_guided_tables: B * N must stay below 2^31 (u_src holds b * N + t)");
    SINGLE(c, vvk_guided_tables(seq_len, guided, B, N, Rc, Ru, row_start, rs_rel, kv_len, row_pos, u_src, u_crow, u_row, (hipStream_t)st, &m__));
}
int vv_ref_len(vv_ctx* c, const int32_t* audio_len, int32_t* ref_len, int B, int hop, void* st) {
    ALIGN4(c, "vv_ref_len", (uintptr_t)audio_len | (uintptr_t)ref_len);
    SINGLE(c, vvk_ref_len(audio_len, ref_len, B, hop, (hipStream_t)st, &m__));
}
int vv_decode_len(vv_ctx* c, const int32_t* seq_len, const int32_t* ref_len, int32_t* lens, int B, int n_levels, const int32_t* mult, int N, int T_max,
                  void* st) {
    ALIGN4(c, "vv_decode_len", (uintptr_t)seq_len | (uintptr_t)ref_len | (uintptr_t)lens | (uintptr_t)mult);
    SINGLE(c, vvk_decode_len(seq_len, ref_len, lens, B, n_levels, mult, N, T_max, (hipStream_t)st, &m__));
}
int vv_vocos_lens(vv_ctx* c, const int32_t* seq_len, const int32_t* ref_len, int32_t* lens, int B, int N, int T_max, void* st) {
    ALIGN4(c, "vv_vocos_lens", (uintptr_t)seq_len | (uintptr_t)ref_len | (uintptr_t)lens);
    SINGLE(c, vvk_vocos_lens(seq_len, ref_len, lens, B, N, T_max, (hipStream_t)st, &m__));
}
int vv_mel_slice(vv_ctx* c, const float* x, int B, int N, int n_mel, const int32_t* ref_len, const int32_t* seq_len, float* out, int T, void* st) {
    ALIGN4(c, "vv_mel_slice", (uintptr_t)ref_len | (uintptr_t)seq_len | (uintptr_t)x | (uintptr_t)out);
    SINGLE(c, vvk_mel_slice(x, B, N, n_mel, ref_len, seq_len, out, T, (hipStream_t)st, &m__));
}
int vv_vocos_im2col_ex(vv_ctx* c, const float* x, int B, int N, int n_mel, const int32_t* ref_len, const int32_t* seq_len, int T_max, int k, float* out,
                       int ld_out, void* st) {
    ALIGN4(c, "vv_vocos_im2col_ex", (uintptr_t)ref_len | (uintptr_t)seq_len);
    SINGLE(c, vvk_vocos_im2col(x, B, N, n_mel, ref_len, seq_len, T_max, k, out, ld_out, (hipStream_t)st, &m__));
}
int vv_vocos_spectrum(vv_ctx* c, const float* head, int ld_head, int R, int n_fft, float* out, void* st) {
    if (!c) return -22;
    if (((uintptr_t)head | (uintptr_t)out) % 4) return c->fail(-22, "vv_vocos_spectrum: head and out must be 4-byte aligned");
    SINGLE(c, vvk_vocos_spectrum(head, ld_head, R, n_fft, out, (hipStream_t)st, &m__));
}
int vv_vocos_ola(vv_ctx* c, const float* frames, int ld_f, int B, int T_max, const int32_t* lens, const float* window, int n_fft, int hop,
                 int16_t* pcm, int ld_pcm, int32_t* pcm_len, float* wave, int ld_wave, void* st) {
    ALIGN4(c, "vv_vocos_ola", (uintptr_t)lens | (uintptr_t)pcm_len | (uintptr_t)frames | (uintptr_t)window | (uintptr_t)wave);
    if ((uintptr_t)pcm % 2) return c->fail(-22, "vv_vocos_ola: pcm must be 2-byte aligned");
    if (n_fft < 2 || n_fft % 2) return c->fail(-22, "vv_vocos_ola: n_fft must be even and at least 2");
    SINGLE(c, vvk_vocos_ola(frames, ld_f, B, T_max, lens, window, n_fft, hop, pcm, ld_pcm, pcm_len, wave, ld_wave, (hipStream_t)st, &m__));
}
#undef ALIGN4

}  // extern "C"
