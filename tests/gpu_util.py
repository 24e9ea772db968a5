"""Helpers for the -m gpu parity tests: call single kernels through the C ABI."""
import copy
import ctypes as C
import dataclasses
import math

import torch

from vietvoice_tts_amd import runtime as rt

DEV = "cuda:0"


def stream():
    return torch.cuda.current_stream().cuda_stream


def check(eng, rc):
    assert rc == 0, eng.lib.vv_last_error(eng.ctx).decode()


def rel_err(got: torch.Tensor, ref: torch.Tensor) -> float:
    got, ref = got.detach().float().cpu(), ref.detach().float().cpu()
    return float((got - ref).abs().max() / (ref.abs().max() + 1e-12))


def gemm_tail_plan(eng, M, N, K):
    row0, parts = C.c_int32(0), C.c_int32(0)
    check(eng, eng.lib.vv_gemm_tail_plan(eng.ctx, M, N, K, C.byref(row0), C.byref(parts)))
    return row0.value, parts.value


def gemm(eng, A, W, bias=None, mode=0, act=0, out_dtype=None, gate=None, C_io=None, ropes=None, seq_n=0, rope_dim=0, n_store=0, tile=0,
         rope_pos=None, rope_by_row=0, tail=None, c_fill=0.0, rope_skip_q=0, rope_theta=0.0, chip_share=0):
    """A [M,K], W [N,K] on device, same dtype (bf16 or f32).  tail = (fp32 C_tail tensor [parts][M - row0][N], row0, parts): the
    split-K tail request.  c_fill: what a fresh output buffer holds before the launch (shows rows the kernel leaves unwritten)."""
    dt = rt.VV_BF16 if A.dtype == torch.bfloat16 else rt.VV_F32
    od = dt if out_dtype is None else out_dtype
    M, K = A.shape
    N = W.shape[0]
    if C_io is None:
        C_io = torch.full((M, N), c_fill, dtype=torch.bfloat16 if od == rt.VV_BF16 else torch.float32, device=DEV)
    a = rt.vv_gemm_args()
    a.dtype, a.out_dtype, a.mode, a.act = dt, od, mode, act
    a.A, a.lda, a.W, a.ldw, a.C, a.ldc = A.data_ptr(), A.stride(0), W.data_ptr(), W.stride(0), C_io.data_ptr(), C_io.stride(0)
    a.M, a.N, a.K = M, N, K
    a.bias = None if bias is None else bias.data_ptr()
    a.gate = None if gate is None else gate.data_ptr()
    if ropes is not None:
        a.cos_q, a.sin_q, a.cos_k, a.sin_k = [t.data_ptr() for t in ropes[:4]]
        if len(ropes) == 6:
            a.rope_cs_q, a.rope_cs_k = ropes[4].data_ptr(), ropes[5].data_ptr()
    a.n_store, a.seq_n, a.rope_dim, a.tile = n_store, seq_n, rope_dim, tile
    a.rope_pos = None if rope_pos is None else rope_pos.data_ptr()
    a.rope_by_row = rope_by_row
    a.rope_skip_q = rope_skip_q
    a.chip_share = chip_share
    a.rope_theta = rope_theta
    if tail is not None:
        a.C_tail, a.tail_row0, a.tail_parts = tail[0].data_ptr(), tail[1], tail[2]
    check(eng, eng.lib.vv_gemm(eng.ctx, C.byref(a), stream()))
    torch.cuda.synchronize()
    return C_io


# ------------------------------------------------------------------------------------ attention: wrapper, float64 reference, cases
LOG2E_F32 = 1.4426950408889634          # the kernel's constant (rounded to fp32 where it is used)
LN2_F32 = float(torch.tensor(math.log(2.0), dtype=torch.float32))       # q_scale of the level families: LOG2E x LN2_F32 == 1.0f exactly
TOL_F32 = 2e-4
TOL_BF16 = 1.5e-2
BF16_STEP = 2.0 ** -8                   # one bf16 output step at full range


def _i32(v):
    return None if v is None else torch.tensor(list(v), dtype=torch.int32, device=DEV)


def attention(eng, qkv, *, n_seq, seq_n, heads, dtype=None, kv_len=None, row_start=None, total_rows=0, q_scale=0.0, rope_cs_q=None,
              ld_qkv=None, ld_out=None, sentinel_rows=0, fill=7.0, expect_error=False):
    """vv_attention on qkv [rows][ld_qkv] (device, bf16 or f32; dtype defaults to the tensor's).  kv_len / row_start: lists or None;
    rope_cs_q: device fp32 [seq_n][64] or None.  Returns the WHOLE output buffer [rows + sentinel_rows][ld_out], which held `fill`
    everywhere before the launch -- padding columns and sentinel rows included.  expect_error: returns (rc, message) instead."""
    tdt = qkv.dtype if dtype is None else dtype
    dim = heads * 64
    ld_qkv = qkv.stride(0) if ld_qkv is None else ld_qkv
    ld_out = dim if ld_out is None else ld_out
    rows = total_rows if total_rows > 0 else n_seq * seq_n
    out = torch.full((rows + sentinel_rows, ld_out), fill, dtype=tdt, device=DEV)
    kv, rs = _i32(kv_len), _i32(row_start)
    a = rt.vv_attn_args()
    a.dtype = rt.VV_BF16 if tdt == torch.bfloat16 else rt.VV_F32
    a.qkv, a.ld_qkv, a.out, a.ld_out = qkv.data_ptr(), ld_qkv, out.data_ptr(), ld_out
    a.n_seq, a.seq_n, a.heads, a.dim = n_seq, seq_n, heads, dim
    a.kv_len = None if kv is None else kv.data_ptr()
    a.row_start = None if rs is None else rs.data_ptr()
    a.total_rows, a.q_scale = total_rows, q_scale
    a.rope_cs_q = None if rope_cs_q is None else rope_cs_q.data_ptr()
    rc = eng.lib.vv_attention(eng.ctx, C.byref(a), stream())
    torch.cuda.synchronize()
    if expect_error:
        return rc, eng.lib.vv_last_error(eng.ctx)
    check(eng, rc)
    return out


def bf16r(x):
    """Round a float64 tensor onto the bf16 grid (through fp32: the second rounding moves a tie by 2^-29 relative at most)."""
    return x.float().bfloat16().double()


def rope_cs_table(seq_n, scale, theta=10000.0):
    """float64 [seq_n][64] compact (cos, sin) pair table of the query side: pair i at columns 2i, 2i + 1, the softmax scale folded in."""
    pos = torch.arange(seq_n, dtype=torch.float64)[:, None]
    ang = pos * theta ** (-torch.arange(32, dtype=torch.float64)[None, :] * 2.0 / 64.0)
    t = torch.empty(seq_n, 64, dtype=torch.float64)
    t[:, 0::2], t[:, 1::2] = torch.cos(ang) * scale, torch.sin(ang) * scale
    return t


def _seq_operands(qkv, r0, L, heads, rope_cs_q):
    dim = heads * 64
    blk = qkv[r0:r0 + L, :3 * dim].double()
    q, k, v = (blk[:, i * dim:(i + 1) * dim].reshape(L, heads, 64) for i in range(3))
    if rope_cs_q is not None:           # position = row inside the sequence; interleaved pairs
        cs = rope_cs_q[:L].double()
        c, s = cs[:, None, 0::2], cs[:, None, 1::2]
        a, b = q[..., 0::2], q[..., 1::2]
        q = torch.stack([a * c - b * s, b * c + a * s], dim=-1).reshape(L, heads, 64)
    return q, k, v


def _seq_rows(n_seq, seq_n, lens, starts):
    lens = [seq_n] * n_seq if lens is None else [max(1, min(int(L), seq_n)) for L in lens]
    return [((s * seq_n) if starts is None else int(starts[s]), lens[s]) for s in range(n_seq)]


def attention_ref(qkv, *, n_seq, seq_n, heads, lens=None, starts=None, q_scale=1.0, rope_cs_q=None, base2=False):
    """float64 softmax(q_scale q.k) v per (sequence, head) of the operands AS GIVEN (CPU tensor [rows][>= 3 dim]); query rows [0, len).
    base2: the weights are 2^(q.k) (the level families, q_scale ignored).  With rope_cs_q (float64 table) q is roped first and carries
    its scale.  Returns a list over sequences of (ref [len][heads][64], vmax [heads] = max |V| over the head's valid keys)."""
    res = []
    for r0, L in _seq_rows(n_seq, seq_n, lens, starts):
        q, k, v = _seq_operands(qkv, r0, L, heads, rope_cs_q)
        sc = torch.einsum("qhd,khd->hqk", q, k)
        sc = sc * (math.log(2.0) if base2 else (1.0 if rope_cs_q is not None else q_scale))
        res.append((torch.einsum("hqk,khd->qhd", torch.softmax(sc, -1), v), v.abs().amax(dim=(0, 2))))
    return res


def attention_model_bf16(qkv, *, n_seq, seq_n, heads, lens=None, starts=None, q_scale=1.0, rope_cs_q=None, base2=False):
    """float64 ROUNDING MODEL of a bf16 attention (a yardstick for the bound, not an emulation of the kernel's control flow): Q x log2e x
    q_scale rounded to bf16, float64 scores, p = 2^(s - rowmax) rounded to bf16 for the PV product with the row sum taken unrounded,
    the output rounded to bf16.  Same return as attention_ref."""
    q_mul = 1.0 if base2 else float(torch.tensor(LOG2E_F32, dtype=torch.float32) * torch.tensor(1.0 if rope_cs_q is not None else q_scale, dtype=torch.float32))
    res = []
    for r0, L in _seq_rows(n_seq, seq_n, lens, starts):
        q, k, v = _seq_operands(qkv, r0, L, heads, rope_cs_q)
        sc = torch.einsum("qhd,khd->hqk", bf16r(q * q_mul), k)
        p = torch.exp2(sc - sc.amax(-1, keepdim=True))
        o = torch.einsum("hqk,khd->qhd", bf16r(p), v) / p.sum(-1).t()[:, :, None]
        res.append((bf16r(o), v.abs().amax(dim=(0, 2))))
    return res


def attention_errs(got, refs, *, n_seq, seq_n, heads, lens=None, starts=None):
    """Per (sequence, head, query row): max_d |got - ref| / max |V| of that head's valid keys.  got: the output buffer (any device) or a
    list shaped like refs.  Returns (worst, (sequence, head, row))."""
    worst, where = -1.0, None
    for s, (r0, L) in enumerate(_seq_rows(n_seq, seq_n, lens, starts)):
        ref, vmax = refs[s]
        g = got[s][0] if isinstance(got, list) else got[r0:r0 + L, :heads * 64].detach().cpu().double().reshape(L, heads, 64)
        e = (g - ref).abs().amax(-1) / vmax[None, :]
        e = torch.where(torch.isfinite(e), e, torch.full_like(e, float("inf")))
        m = float(e.max())
        if m > worst:
            row, h = divmod(int(e.argmax()), heads)
            worst, where = m, (s, h, row)
    return worst, where


class AttnCase:
    """One problem of the attention parity grid: master operands [n_seq][seq_n][3 dim] fp32 (padded), valid lengths, how q is scaled."""

    def __init__(self, name, family, master, lens, heads, q_scale=1.0, rope=False, base2=False, pad_qkv=0, pad_out=0, layouts=("full", "ragged", "packed")):
        self.name, self.family, self.master, self.lens, self.heads = name, family, master, list(lens), heads
        self.n_seq, self.seq_n = master.shape[0], master.shape[1]
        self.q_scale, self.rope, self.base2, self.pad_qkv, self.pad_out, self.layouts = q_scale, rope, base2, pad_qkv, pad_out, layouts
        self.dim = heads * 64

    def dtypes(self):
        return (torch.bfloat16,) if self.rope else (torch.float32, torch.bfloat16)       # the fp32 kernel takes no query-side rope table

    def rope_table(self):
        return rope_cs_table(self.seq_n, 0.125) if self.rope else None

    def operands(self, dtype):
        """-> (operands [n_seq][seq_n][3 dim] in dtype as the kernel receives them, q_scale argument of the launch, reference keywords).
        The fp32 kernel has no q_scale: q carries the factor (ln 2 for the level families), the reference is natural on what is stored."""
        m = self.master.clone()
        if dtype == torch.bfloat16:
            kw = dict(q_scale=LN2_F32 if self.base2 else self.q_scale, base2=self.base2, rope_cs_q=self.rope_table())
            return m.to(dtype), (LN2_F32 if self.base2 else (0.0 if self.q_scale == 1.0 else self.q_scale)), kw
        m[..., :self.dim] *= torch.tensor(LN2_F32 if self.base2 else self.q_scale, dtype=torch.float32)
        return m, 0.0, dict(q_scale=1.0, base2=False, rope_cs_q=None)

    def layout(self, ops, which):
        """-> (qkv CPU [rows][3 dim + pad_qkv], lens or None, starts or None, total_rows).  'full': padded, every key valid, no length
        array; 'ragged': padded with the case's lengths; 'packed': the valid rows back to back with gaps of rows nobody owns (s % 3
        after sequence s, 2 at the end; finite values)."""
        n_seq, seq_n, w = self.n_seq, self.seq_n, 3 * self.dim
        g = torch.Generator().manual_seed(977 + n_seq * seq_n)
        if which in ("full", "ragged"):
            body, lens, starts = ops.reshape(n_seq * seq_n, w), (None if which == "full" else self.lens), None
        else:
            lens, starts, parts, r = self.lens, [], [], 0
            for s, L in enumerate(lens):
                gap = s % 3 if s + 1 < n_seq else 2
                starts.append(r)
                parts += [ops[s, :L], torch.randn(gap, w, generator=g).to(ops.dtype)]
                r += L + gap
            body = torch.cat(parts, 0)
        qkv = torch.full((body.shape[0], w + self.pad_qkv), 1.0e4, dtype=ops.dtype)      # padding columns: finite, and wrong if read
        qkv[:, :w] = body
        return qkv, lens, starts, body.shape[0]

    def lens_of(self, which):
        return None if which == "full" else self.lens


def _generic_master(n_seq, seq_n, heads, seed, q_std=0.35):
    g = torch.Generator().manual_seed(seed)
    m = torch.randn(n_seq, seq_n, 3 * heads * 64, generator=g)
    m[..., :heads * 64] *= q_std
    return m


def _edge_lens(seq_n):
    """1, seq_n and b - 1, b, b + 1 around every multiple b of 32 (so of 64 and 128 too) below seq_n."""
    v = {1, seq_n}
    for b in range(32, seq_n, 32):
        v |= {x for x in (b - 1, b, b + 1) if 1 <= x <= seq_n}
    return sorted(v)


def attn_edge_cases():
    """Section 2 of the grid: lengths at the tile edges, (sequence, head) pair counts {1, 6, 8, 9, 48} among them, padded leading
    dimensions, q_scale != 1 and the query-side rope in ragged and packed rows."""
    cases = []
    for i, seq_n in enumerate([1, 31, 32, 33, 64, 65, 127, 128, 129, 257, 640]):
        lens = _edge_lens(seq_n)
        heads = 1 if seq_n in (1, 640) else 2
        qs = 0.125 if i % 2 else 1.0
        cases.append(AttnCase(f"seq_n{seq_n}", "edge", _generic_master(len(lens), seq_n, heads, 100 + seq_n, 0.35 / qs), lens, heads, q_scale=qs,
                              pad_qkv=8 if i % 2 == 0 else 0, pad_out=4 if i % 3 != 1 else 0))
    for name, heads, seq_n, lens, qs in [("pairs6", 2, 65, [65, 64, 1], 0.125), ("pairs9", 3, 130, [129, 33, 130], 1.0),
                                         ("pairs48", 16, 129, [129, 128, 31], 0.125)]:
        cases.append(AttnCase(name, "edge", _generic_master(len(lens), seq_n, heads, 300 + heads, 0.35 / qs), lens, heads, q_scale=qs, pad_qkv=8, pad_out=4))
    cases.append(AttnCase("rope_ragged", "edge", _generic_master(4, 257, 2, 401, 2.8), [257, 100, 33, 1], 2, rope=True, pad_qkv=8, pad_out=4))
    return cases


LEVEL_SEQ_N = 320                       # 5 tiles of 64 keys
SPIKE_POS = [(0, 3, 4), (7, 8, 31), (32, 35, 63)]


def _level_master(levels, qsign, heads, seed):
    """levels [n_seq][heads][seq_n] (log2 units; level / 8 must be exact in bf16), qsign [seq_n]: q[0] = 8 qsign, k[j][0] = level_j / 8;
    the other 63 dims small random (q std 0.25, k std 0.5: about one log2 unit of score noise); v std 1."""
    n_seq, _, seq_n = levels.shape
    g = torch.Generator().manual_seed(seed)
    q = torch.randn(n_seq, seq_n, heads, 64, generator=g) * 0.25
    k = torch.randn(n_seq, seq_n, heads, 64, generator=g) * 0.5
    v = torch.randn(n_seq, seq_n, heads, 64, generator=g)
    q[..., 0] = 8.0 * qsign[None, :, None]
    k[..., 0] = levels.permute(0, 2, 1) / 8.0
    return torch.cat([t.reshape(n_seq, seq_n, heads * 64) for t in (q, k, v)], -1)


def attn_level_cases():
    """Section 3: scores placed around the speculative softmax's decision edges (half-row sum 2^64, first-tile row sum 2^-64)."""
    N, heads = LEVEL_SEQ_N, 2
    ones = torch.ones(N)
    tiles = lambda vals: torch.tensor(vals, dtype=torch.float32).repeat_interleave(64)
    cases, seed = [], [700]

    def add(name, family, tile_levels, lens=(320, 290, 65), qsign=ones, extra=None):
        lv = tiles(tile_levels)[None, None, :].repeat(3, heads, 1)
        for key, val in (extra or []):
            lv[:, :, key] = val
        seed[0] += 1
        cases.append(AttnCase(name, family, _level_master(lv, qsign, heads, seed[0]), lens, heads, base2=True))

    for lvl in (-62, -64, -70):
        add(f"flat{lvl}", "flat_tiny_edge", [lvl] * 5)
    for lvl in (-66, -63, -60):
        add(f"first{lvl}", "first_tile_low", [lvl, 0, 0, 0, 0])
    add("ramp_up30", "ramp_up", [0, 30, 60, 90, 120])
    add("ramp_down58", "ramp_down", [58, 28, -2, -32, -62])
    add("flat58", "flat_high", [58] * 5)
    add("flat63", "flat_high", [63] * 5)
    add("two_refs", "two_refs", [0] * 5, lens=(320, 233, 70), extra=[(64 + 5, 100.0), (192 + 40, 200.0)])
    mixed = torch.zeros(N)
    mixed[5::32], mixed[20::32] = 1.0, -1.0         # per wave: row 5 sees the levels, row 20 their negatives, the others noise only
    add("mixed_first_tile", "mixed_wave", [70, 0, 0, 0, 0], qsign=mixed)
    add("mixed_down_then_up", "mixed_wave", [-70, 90, 0, 0, 0], qsign=mixed)
    for mag in (70, 200, 576):          # one spike per (sequence, head): tile t = s // 3, key position SPIKE_POS[s % 3][head]
        lv, lens = torch.zeros(15, 3, N), []
        for s in range(15):
            t, grp = s // 3, SPIKE_POS[s % 3]
            for h in range(3):
                lv[s, h, 64 * t + grp[h]] = float(mag)
            lens.append(64 * t + max(grp) + 1)      # ragged / packed: the sequence ends inside the spiked tile, head 2's spike is its last key
        seed[0] += 1
        cases.append(AttnCase(f"spike{mag}", "spike", _level_master(lv, ones, 3, seed[0]), lens, 3, base2=True))
    return cases


def attn_cases():
    return attn_edge_cases() + attn_level_cases()


# Families in which ONE key holds all of a row's weight (the next one stands 2^-60 or less below it) and that key sits far from zero.
# The model centres a row on its maximum: that key's p is exactly 1, the row is v itself, the model's figure is 0 and says nothing.
# A kernel whose reference must be bf16-representable (it rides through the MFMA) has p = 2^(s - bf16(max)), any number of a binade,
# rounds it for the PV product and divides by the unrounded sum: the row is bf16(v x bf16(p) / p) -- two roundings of <= 2^-8 relative
# each, |v (1 + d1)(1 + d2) - v| <= |v| (2^-7 + 2^-16).  So these families get two bf16 steps where the others get one.
ATTN_DOMINATED_FAMILIES = ("two_refs", "spike")


def attn_case_bound(case, dtype, model_err):
    """fp32: TOL_F32.  bf16: min(TOL_BF16, 3 x the rounding model's own error on this case + one bf16 output step), two steps for the
    single-key-dominated families (above)."""
    if dtype == torch.float32:
        return TOL_F32
    steps = BF16_STEP * (2.0 + BF16_STEP) if case.family in ATTN_DOMINATED_FAMILIES else BF16_STEP
    return min(TOL_BF16, 3.0 * model_err + steps)


def attn_case_max_log2_score(case):
    """Largest |score| in the bf16 kernel's log2 domain over EVERY (query, key) pair of a sequence's seq_n padded rows."""
    ops, _, kw = case.operands(torch.bfloat16)
    q_mul = 1.0 if kw["base2"] else LOG2E_F32 * (1.0 if kw["rope_cs_q"] is not None else kw["q_scale"])
    worst = 0.0
    for s in range(case.n_seq):
        q, k, _ = _seq_operands(ops[s], 0, case.seq_n, case.heads, kw["rope_cs_q"])
        worst = max(worst, float((torch.einsum("qhd,khd->hqk", q, k) * q_mul).abs().max()))
    return worst


def attn_case_refs(case, dtype, which):
    """-> (refs, model_err or None): the float64 reference of the case in one layout's lengths, and (bf16) the model's worst error."""
    ops, _, kw = case.operands(dtype)
    shp = dict(n_seq=case.n_seq, seq_n=case.seq_n, heads=case.heads, lens=case.lens_of(which))
    flat = ops.reshape(case.n_seq * case.seq_n, -1)
    refs = attention_ref(flat, **shp, **kw)
    if dtype != torch.bfloat16:
        return refs, None
    model = attention_model_bf16(flat, **shp, **kw)
    return refs, attention_errs(model, refs, **shp)[0]


# ------------------------------------------------------------------------------------ convolutions: wrappers, float64 references, metric
import torch.nn.functional as F  # noqa: E402

NAN = float("nan")
CONV_FILL = 7.0                         # what guard bands, padding columns and sentinel rows hold before a launch
CONV_GUARD = 64                         # guard elements in front of and behind a conv output (a multiple of 4: out stays 16-byte aligned)
EPS24 = 2.0 ** -24
X3_DROPPED = 2.0 ** -23                 # m.l + l.m + l.l of the six-product form (top of vv_vocoder_x3.hip), per term, so per A_e
# Round-to-nearest store of a bf16 output.  bf16 keeps 8 significant bits: the spacing in [2^e, 2^(e+1)) is 2^(e-7), half of it is
# 2^(e-8) -- 2^-9 of the binade's TOP but up to 2^-8 of an element at its bottom (1.004 stores as 1.0078: off by 2^-8 x 1.004).  The term
# per element is therefore 2^-8 |ref_e|; 2^-9 |ref_e| is what a float64 value rounded to bf16 already exceeds (the tests print both the
# device's figure and that store-only model under the 2^-9 term: profiles/conv_parity/notes.md).
BF16_STORE = 2.0 ** -8
BF16_STORE_HALF = 2.0 ** -9


def pack_conv(w):         # torch [Cout][Cin][KW] -> [Cin_pad8][KW][Cout_pad64]
    cout, cin, kw = w.shape
    t = torch.zeros(((cin + 7) // 8 * 8, kw, (cout + 63) // 64 * 64))
    t[:cin, :, :cout] = w.permute(1, 2, 0)
    return t


def conv_transpose_pack(w, up):
    """torch ConvTranspose1d weight [Cin][Cout][2 up] -> the polyphase slab [Cin_pad8][2][rows_pad64]: row = co * up + phase, tap j of
    that row = w[ci][co][phase + j up]  (out time q up + phase - up / 2 reads in[q - j])."""
    cin, cout, k = w.shape
    assert k == 2 * up
    rows = cout * up
    t = torch.zeros(((cin + 7) // 8 * 8, 2, (rows + 63) // 64 * 64))
    t[:cin, :, :rows] = w.reshape(cin, cout, 2, up).permute(0, 2, 1, 3).reshape(cin, 2, rows)
    return t


def split_conv_weights(eng, dw):
    """vv_conv_split_weights on a packed fp32 slab [Cin_pad][KW][rows_pad] (device) -> the x3 slab (device uint16 tensor)."""
    cin_pad, kw, rows_pad = dw.shape
    nbytes = int(eng.lib.vv_conv_split_bytes(cin_pad, kw, rows_pad))
    assert nbytes == (cin_pad + 15) // 16 * kw * 3 * rows_pad * 16 * 2
    wb = torch.zeros(nbytes // 2, dtype=torch.int16, device=DEV)
    check(eng, eng.lib.vv_conv_split_weights(eng.ctx, dw.data_ptr(), cin_pad, kw, rows_pad, wb.data_ptr(), stream()))
    torch.cuda.synchronize()
    return wb


def _guarded(shape, guard, fill, init=None, dtype=torch.float32):
    """-> (whole flat buffer, view of `shape` that starts `guard` elements in).  The view holds init (or zeros), the bands hold fill."""
    n = int(math.prod(shape))
    buf = torch.full((n + 2 * guard,), fill, dtype=dtype, device=DEV)
    view = buf[guard:guard + n].view(*shape)
    if init is None:
        view.zero_()
    else:
        view.copy_(init.to(DEV))
    return buf, view


def _bands_intact(buf, guard, fill, what):
    if guard:
        assert bool((buf[:guard] == fill).all()), f"{what}: the guard band in front of out was written"
        assert bool((buf[-guard:] == fill).all()), f"{what}: the guard band behind out was written"


def _offset_input(x, in_offset, in_tail):
    """x on the device, in_offset elements into an allocation whose head and tail (in_tail elements) hold NaN -> (keep-alive, pointer)."""
    if not in_offset and not in_tail:
        dx = x.to(DEV).contiguous()
        return dx, dx.data_ptr()
    flat = torch.full((in_offset + x.numel() + in_tail,), NAN, dtype=x.dtype, device=DEV)
    flat[in_offset:in_offset + x.numel()] = x.reshape(-1).to(DEV)
    return flat, flat.data_ptr() + in_offset * x.element_size()


def conv1d(eng, x, wp, bias, cout, T_out, KW, dil, up, resid=None, pre_slope=1.0, scale=1.0, accumulate=0, out0=None, lens=None, x3=False,
           guard=0, fill=CONV_FILL, in_offset=0, in_tail=0, expect_error=False):
    """vv_conv1d on x [B][Cin][T_in] (CPU) with the packed slab wp.  up = 0: conv; up >= 2: polyphase ConvTranspose.  x3: False = the f32
    MFMA kernel; True = x3 with wg_rows 0; an int = x3 with that wg_rows (128: 8-wave workgroups, -1: never the streaming up-sampler).
    guard: fp32 elements of `fill` in front of and behind out, checked after the launch.  in_offset / in_tail: the input pointer stands
    that many elements into a larger allocation whose head / tail hold NaN.  Returns out [B][cout][T_out] (device)."""
    B, cin, T_in = x.shape
    assert guard % 4 == 0
    buf, out = _guarded((B, cout, T_out), guard, fill, out0)
    keep, in_ptr = _offset_input(x, in_offset, in_tail)
    db = bias.to(DEV)
    if guard:                           # eight more channels of NaN behind the slab: a chunk that runs past Cin_pad8 would show
        wflat = torch.full((wp.numel() + 8 * wp.shape[1] * wp.shape[2],), NAN, device=DEV)
        dw = wflat[:wp.numel()].view(wp.shape)
        dw.copy_(wp.to(DEV))
    else:
        dw = wp.to(DEV)
    dr = resid.to(DEV) if resid is not None else None
    dl = torch.tensor(lens, dtype=torch.int32, device=DEV) if lens is not None else None
    a = rt.vv_conv_args()
    a.in_, a.W, a.bias, a.out = in_ptr, dw.data_ptr(), db.data_ptr(), out.data_ptr()
    a.resid = dr.data_ptr() if dr is not None else None
    a.B, a.Cin, a.Cout, a.T_in, a.T_out, a.KW, a.dil = B, cin, cout, T_in, T_out, KW, dil
    a.transposed, a.up = (1 if up else 0), up
    a.rows_total = cout * up if up else cout
    a.rows_pad = (a.rows_total + 63) // 64 * 64
    a.accumulate, a.pre_slope, a.out_scale = accumulate, pre_slope, scale
    a.len_in = dl.data_ptr() if dl is not None else None
    if x3:
        wb = split_conv_weights(eng, dw)
        a.W_x3 = wb.data_ptr()
        a.wg_rows = x3 if (isinstance(x3, int) and not isinstance(x3, bool)) else 0
    rc = eng.lib.vv_conv1d(eng.ctx, C.byref(a), stream())
    torch.cuda.synchronize()
    if expect_error:
        return rc, eng.lib.vv_last_error(eng.ctx)
    check(eng, rc)
    _bands_intact(buf, guard, fill, "vv_conv1d")
    del keep
    return out


def mrf_resblock(eng, y, p1, b1, p2, b2, KW, dil, lens=None, slope=0.1, scale=1.0, accumulate=0, out0=None, guard=0, fill=CONV_FILL,
                 in_offset=0, in_tail=0, expect_error=False):
    """vv_mrf_resblock on y [B][C][T] (CPU), packed slabs p1 / p2 [C_pad8][KW][64].  Guard band and input offset as in conv1d."""
    B, C_, T = y.shape
    assert guard % 4 == 0
    buf, out = _guarded((B, C_, T), guard, fill, out0)
    keep, in_ptr = _offset_input(y, in_offset, in_tail)
    dev = [t.to(DEV) for t in (p1, b1, p2, b2)]
    dl = torch.tensor(lens, dtype=torch.int32, device=DEV) if lens is not None else None
    a = rt.vv_mrf_args()
    a.y = in_ptr
    a.W1, a.b1, a.W2, a.b2 = [t.data_ptr() for t in dev]
    a.out = out.data_ptr()
    a.B, a.C, a.T, a.KW, a.dil, a.rows_pad, a.accumulate, a.slope, a.out_scale = B, C_, T, KW, dil, 64, accumulate, slope, scale
    a.len_in = dl.data_ptr() if dl is not None else None
    rc = eng.lib.vv_mrf_resblock(eng.ctx, C.byref(a), stream())
    torch.cuda.synchronize()
    if expect_error:
        return rc, eng.lib.vv_last_error(eng.ctx)
    check(eng, rc)
    _bands_intact(buf, guard, fill, "vv_mrf_resblock")
    del keep
    return out


def _lrelu(x, slope):
    """LeakyReLU with the slope the kernel is given: the fp32 value of `slope`."""
    return torch.where(x >= 0, x, x * float(torch.tensor(slope, dtype=torch.float32)))


def _zero_outside(x, lens):
    """x [B][C][T] with columns outside [0, len_b) set to zero (whatever they held: NaN too)."""
    if lens is None:
        return x
    t = torch.arange(x.shape[-1])
    keep = t[None, :] < torch.tensor([max(0, min(int(L), x.shape[-1])) for L in lens])[:, None]
    return torch.where(keep[:, None, :], x, torch.zeros((), dtype=x.dtype))


def _conv_taps(a, w, dil):
    """Plain sum over taps: a [B][Cin][T], w [Cout][Cin][KW] -> [B][Cout][T], 'same' padding dil (KW - 1) / 2 (no library convolution)."""
    KW, T = w.shape[2], a.shape[2]
    left = dil * (KW - 1) // 2
    ap = F.pad(a, (left, dil * (KW - 1) - left))
    y = torch.zeros(a.shape[0], w.shape[0], T, dtype=a.dtype)
    for k in range(KW):
        y += torch.einsum("oc,bct->bot", w[:, :, k], ap[:, :, k * dil:k * dil + T])
    return y


def _conv_transpose_taps(a, w, up):
    """Plain scatter form of ConvTranspose1d (stride up, kernel 2 up, padding up / 2): a [B][Cin][T], w [Cin][Cout][2 up] -> [B][Cout][T up]."""
    B, _, T = a.shape
    full = torch.zeros(B, w.shape[1], (T - 1) * up + 2 * up, dtype=a.dtype)
    for k in range(2 * up):
        full[:, :, k:k + (T - 1) * up + 1:up] += torch.einsum("co,bct->bot", w[:, :, k], a)
    return full[:, :, up // 2:up // 2 + T * up]


def conv_ref(x, w, bias, *, dil=1, up=0, lens=None, slope=1.0, resid=None, scale=1.0, prev=None, mode="f64"):
    """out = (conv(lrelu(x zero-filled outside [0, len))) + bias [+ resid as given]) * scale [+ previous out], every column of the output.
    x [B][Cin][T]; w in torch layout ([Cout][Cin][KW], or [Cin][Cout][2 up] for the transposed form); all operands as the kernel gets them.
    mode 'f64': the float64 reference (plain tap sums).  'abs': the per-element scale A_e, the same expression with every operand replaced
    by its absolute value.  'f32': the yardstick, the CPU library in fp32 on the same operands."""
    if mode == "f32":
        a = F.leaky_relu(_zero_outside(x.float(), lens), slope)
        w32, b32 = w.float(), bias.float()
        y = F.conv_transpose1d(a, w32, b32, stride=up, padding=up // 2) if up else F.conv1d(a, w32, b32, dilation=dil, padding=dil * (w.shape[2] - 1) // 2)
        if resid is not None:
            y = y + resid.float()
        y = y * torch.tensor(scale, dtype=torch.float32)
        return y + prev.float() if prev is not None else y
    pos = (lambda t: t.double().abs()) if mode == "abs" else (lambda t: t.double())
    a = pos(_lrelu(_zero_outside(x.double(), lens), slope))
    y = _conv_transpose_taps(a, pos(w), up) if up else _conv_taps(a, pos(w), dil)
    y = y + pos(bias)[None, :, None]
    if resid is not None:
        y = y + pos(resid)
    y = y * pos(torch.tensor(scale, dtype=torch.float32))       # the kernel multiplies by the fp32 scale it is given
    return y + pos(prev) if prev is not None else y


def mrf_ref(y, w1, b1, w2, b2, *, dil, lens=None, slope=0.1, scale=1.0, prev=None, mode="f64"):
    """conv1 (dilated) + b1, zeroed outside [0, len), LeakyReLU, conv2 (undilated) + b2 + y AS GIVEN, times scale [+ previous out]."""
    if mode == "f32":
        t1 = F.conv1d(F.leaky_relu(_zero_outside(y.float(), lens), slope), w1.float(), b1.float(), dilation=dil, padding=dil * (w1.shape[2] - 1) // 2)
        o = F.conv1d(F.leaky_relu(_zero_outside(t1, lens), slope), w2.float(), b2.float(), padding=(w2.shape[2] - 1) // 2) + y.float()
        o = o * torch.tensor(scale, dtype=torch.float32)
        return o + prev.float() if prev is not None else o
    pos = (lambda t: t.double().abs()) if mode == "abs" else (lambda t: t.double())
    t1 = _conv_taps(pos(_lrelu(_zero_outside(y.double(), lens), slope)), pos(w1), dil) + pos(b1)[None, :, None]
    t1 = pos(_lrelu(_zero_outside(t1, lens), slope))
    o = _conv_taps(t1, pos(w2), 1) + pos(b2)[None, :, None] + pos(y)
    o = o * pos(torch.tensor(scale, dtype=torch.float32))
    return o + pos(prev) if prev is not None else o


def parity_err(got, ref, A, allow=None):
    """max_e (|got_e - ref_e| - allow_e) / A_e and the index of the worst element; a non-finite element counts as infinite.  allow: an
    absolute per-element allowance that is not part of the accumulation error (the bf16 store rounding)."""
    d = (got.detach().cpu().double() - ref).abs()
    if allow is not None:
        d = (d - allow).clamp_min(0.0)
    e = d / A
    e = torch.where(torch.isfinite(e), e, torch.full_like(e, float("inf")))
    i = int(e.argmax())
    where = tuple(int(v) for v in torch.unravel_index(torch.tensor(i), e.shape)) if e.dim() > 1 else (i,)
    return float(e.reshape(-1)[i]), where


def conv_bound(yardstick, x3=False):
    """fp32 forms: max(8 x 2^-24, 4 x yardstick).  Floor: one product rounding plus at most four epilogue roundings (bias, residual,
    scale, accumulate), each <= 2^-24 A_e, with room for the bias add.  4: the kernel sums one fp32 chain of Cin_pad x KW steps per
    element, the CPU library sums in vector lanes (the project grants 2 between its own two orders).  x3: + 2^-23, the dropped piece
    products.  Never fitted to a measurement: profiles/conv_parity/notes.md."""
    return max(8.0 * EPS24, 4.0 * yardstick) + (X3_DROPPED if x3 else 0.0)


# ---- posconv
def posconv_pack(w, groups, dtype):
    """torch grouped-conv weight [G 64][64][KW] -> bf16: [G][KW][64 co][64 ci]; f32: [G][KW][64 ci][64 co]."""
    kw = w.shape[2]
    w4 = w.reshape(groups, 64, 64, kw)
    return (w4.permute(0, 3, 1, 2) if dtype == torch.bfloat16 else w4.permute(0, 3, 2, 1)).contiguous()


def posconv(eng, x, w, bias, *, n_seq, seq_n, groups, resid=None, lens=None, B=None, starts=None, out_dtype=None, pad_in=0, pad_out=0,
            pad_resid=0, sentinel_rows=0, fill=CONV_FILL, tweak=None, expect_error=False):
    """vv_posconv on x [rows][groups 64] (CPU, bf16 or f32: picks the kernel) with the torch-layout weight w [D][64][KW] (same dtype).
    lens: list of B lengths indexed seq % B (B defaults to len(lens)); starts: packed rows.  The leading dimensions are padded by pad_*
    elements; padding columns of in / resid hold 1e4 (finite, wrong if read), those of out and the sentinel rows hold `fill`.  tweak(a)
    may edit the argument struct before the call.  Returns the WHOLE out buffer [rows + sentinel_rows][D + pad_out] (device)."""
    D, rows, dt = groups * 64, x.shape[0], x.dtype
    odt = dt if out_dtype is None else out_dtype
    din = torch.full((rows, D + pad_in), 1.0e4, dtype=dt, device=DEV)
    din[:, :D] = x.to(DEV)
    out = torch.full((rows + sentinel_rows, D + pad_out), fill, dtype=odt, device=DEV)
    dw, db = posconv_pack(w, groups, dt).to(DEV), bias.float().to(DEV)
    dr = None
    if resid is not None:
        dr = torch.full((rows, D + pad_resid), 1.0e4, dtype=dt, device=DEV)
        dr[:, :D] = resid.to(DEV)
    sl, rs = _i32(lens), _i32(starts)
    a = rt.vv_posconv_args()
    a.dtype = rt.VV_BF16 if dt == torch.bfloat16 else rt.VV_F32
    a.out_dtype = rt.VV_BF16 if odt == torch.bfloat16 else rt.VV_F32
    a.in_, a.ld_in, a.W, a.bias, a.out, a.ld_out = din.data_ptr(), D + pad_in, dw.data_ptr(), db.data_ptr(), out.data_ptr(), D + pad_out
    a.resid, a.ld_resid = (None if dr is None else dr.data_ptr()), D + pad_resid
    a.n_seq, a.seq_n, a.groups, a.KW = n_seq, seq_n, groups, w.shape[2]
    a.B = (len(lens) if lens is not None else n_seq) if B is None else B
    a.seq_len = None if sl is None else sl.data_ptr()
    a.row_start = None if rs is None else rs.data_ptr()
    if tweak is not None:
        tweak(a)
    rc = eng.lib.vv_posconv(eng.ctx, C.byref(a), stream())
    torch.cuda.synchronize()
    if expect_error:
        return rc, eng.lib.vv_last_error(eng.ctx)
    check(eng, rc)
    return out


def posconv_rows(n_seq, seq_n, lens=None, starts=None):
    """-> per sequence (first row, rows the kernel writes, valid length): padded layout every row < seq_n; packed rows [0, len) only."""
    res = []
    for s in range(n_seq):
        L = seq_n if lens is None else max(0, min(int(lens[s % len(lens)]), seq_n))
        res.append((s * seq_n, seq_n, L) if starts is None else (int(starts[s]), L, L))
    return res


def posconv_ref(x, w, bias, resid, *, n_seq, seq_n, groups, lens=None, starts=None, mode="f64"):
    """mish(conv(x zero-filled outside [0, len)) + bias) + resid on the operands as given, for every row the kernel writes.  Returns a
    list over sequences of (first row, ref [rows][D]).  Modes as in conv_ref ('f32': F.conv1d + F.mish in fp32)."""
    D, KW = groups * 64, w.shape[2]
    pad = KW // 2
    res = []
    for r0, n, L in posconv_rows(n_seq, seq_n, lens, starts):
        if n == 0:
            res.append((r0, torch.zeros(0, D, dtype=torch.float32 if mode == "f32" else torch.float64)))
            continue
        rz = None if resid is None else resid[r0:r0 + n]
        if mode == "f32":
            xs = x[r0:r0 + n].float().clone()
            xs[L:] = 0
            o = F.mish(F.conv1d(xs.t().unsqueeze(0), w.float(), bias.float(), padding=pad, groups=groups)).squeeze(0).t()
            res.append((r0, o + rz.float() if rz is not None else o))
            continue
        pos = (lambda t: t.double().abs()) if mode == "abs" else (lambda t: t.double())
        xs = pos(x[r0:r0 + n]).clone()
        xs[L:] = 0
        xp = F.pad(xs, (0, 0, pad, pad)).reshape(n + 2 * pad, groups, 64)
        wg = pos(w).reshape(groups, 64, 64, KW)
        z = torch.zeros(n, groups, 64, dtype=torch.float64)
        for k in range(KW):
            z += torch.einsum("tgc,goc->tgo", xp[k:k + n], wg[:, :, :, k])
        o = F.mish(z.reshape(n, D) + pos(bias)[None, :])
        res.append((r0, o + pos(rz) if rz is not None else o))
    return res


# ---- the conv parity grid (tests/test_conv_gpu.py runs it, tests/test_conv_ref_cpu.py checks the claims made here)
# forms -> the x3 argument of conv1d.  'stream' is x3 with wg_rows 0 on a shape the streaming up-sampler takes, 'generic' its twin.
CONV_FORMS = {"f32": False, "x3": True, "x3w": 128, "stream": True, "generic": -1}
# conv_x3_kernel<KW, TR, RT, TG, NWV, OCC> instantiations and the two up2_stream_x3_kernel widths, by the names used in the claims
NARROW, R64, K11, WIDE = "<KW,1,2,4,3>", "<KW,2,2,4,3>", "<11,2,4,4,2>", "<KW,2,2,8,2>"
T_NARROW, T_R64, T_WIDE, STREAM4, STREAM8 = "T<2,1,2,4,3>", "T<2,2,2,4,3>", "T<2,2,2,8,2>", "up2_stream<4>", "up2_stream<8>"
X3_REQUIRED = (NARROW, R64, K11, WIDE, T_R64, T_WIDE, STREAM4, STREAM8)
MRF_VT2 = {3: 124, 7: 120, 11: 116}     # output columns per mrf_pair_kernel workgroup: 128 - ((KW - 1 + 3) & ~3)


class _Ops:
    pass


class ConvCase:
    """One problem of the conv grid.  kind 'conv' / 'tconv' (polyphase ConvTranspose, T = T_in) / 'mrf' (cin = cout = C).  variants:
    'plain' = conv + bias; 'conv2' = the decode's second-conv form (resid, out_scale 1/3, accumulate onto a previous out; mrf: scale 1/3 +
    accumulate).  reach: form -> the x3 instantiation the case claims to reach; claims: form -> (n_win, n_rt) of the 1-D window walk."""

    def __init__(self, name, section, kind, *, B, cin, cout, T, KW=2, dil=1, up=0, lens=None, variants=("plain",), forms=("f32", "x3", "x3w"),
                 reach=None, claims=None, in_offset=0, fallback=False):
        self.name, self.section, self.kind = name, section, kind
        self.B, self.cin, self.cout, self.T, self.KW, self.dil, self.up = B, cin, cout, T, KW, dil, up
        self.lens, self.variants, self.forms, self.reach, self.claims = lens, variants, forms, reach or {}, claims or {}
        self.in_offset, self.fallback = in_offset, fallback
        self.T_out = T * up if up else T
        self.rows_total = cout * up if up else cout
        self.rows_pad = (self.rows_total + 63) // 64 * 64
        self._ops, self._refs = None, {}

    def forms_of(self, variant):
        """The streaming kernel takes no residual and no accumulate: in the conv2 variant 'stream' would be the generic kernel again."""
        return tuple(f for f in self.forms if not (variant == "conv2" and f == "stream"))

    def ops(self):
        if self._ops is None:
            g = torch.Generator().manual_seed(sum(ord(ch) * (i + 1) for i, ch in enumerate(self.name)) % 100003)
            o, B, T = _Ops(), self.B, self.T
            o.x = torch.randn(B, self.cin, T, generator=g)
            if self.kind == "mrf":
                o.w = torch.randn(self.cout, self.cin, self.KW, generator=g) * 1.4 / math.sqrt(self.cin * self.KW)
                o.w2 = torch.randn(self.cout, self.cin, self.KW, generator=g) * 0.45 / math.sqrt(self.cin * self.KW)
                o.bias2 = torch.randn(self.cout, generator=g) * 0.1
                o.wp, o.wp2 = pack_conv(o.w), pack_conv(o.w2)
            elif self.up:
                o.w = torch.randn(self.cin, self.cout, 2 * self.up, generator=g) / math.sqrt(2 * self.cin)
                o.wp = conv_transpose_pack(o.w, self.up)
            else:
                o.w = torch.randn(self.cout, self.cin, self.KW, generator=g) / math.sqrt(self.cin * self.KW)
                o.wp = pack_conv(o.w)
            o.bias = torch.randn(self.cout, generator=g) * 0.1
            o.resid = torch.randn(B, self.cout, self.T_out, generator=g)
            o.prev = torch.randn(B, self.cout, self.T_out, generator=g)
            self._ops = o
        return self._ops

    def item(self, i):
        """The operands of item i alone (B = 1), weights shared."""
        o, s = self.ops(), _Ops()
        s.__dict__.update(o.__dict__)
        s.x, s.resid, s.prev = o.x[i:i + 1], o.resid[i:i + 1], o.prev[i:i + 1]
        return s

    def ref_kw(self, variant, o=None, lens="case"):
        o = self.ops() if o is None else o
        lens = self.lens if lens == "case" else lens
        c2 = variant == "conv2"
        if self.kind == "mrf":
            return dict(dil=self.dil, lens=lens, slope=0.1, scale=1.0 / 3.0 if c2 else 1.0, prev=o.prev if c2 else None)
        return dict(dil=self.dil, up=self.up, lens=lens, slope=0.1, resid=o.resid if c2 else None, scale=1.0 / 3.0 if c2 else 1.0,
                    prev=o.prev if c2 else None)

    def compute(self, variant, mode, o=None, lens="case"):
        o = self.ops() if o is None else o
        kw = self.ref_kw(variant, o, lens)
        if self.kind == "mrf":
            return mrf_ref(o.x, o.w, o.bias, o.w2, o.bias2, mode=mode, **kw)
        return conv_ref(o.x, o.w, o.bias, mode=mode, **kw)

    def refs(self, variant):
        """-> (float64 reference, A_e, the fp32 CPU yardstick's err in the same metric); computed once per (case, variant)."""
        if variant not in self._refs:
            ref, A = self.compute(variant, "f64"), self.compute(variant, "abs")
            self._refs[variant] = (ref, A, parity_err(self.compute(variant, "f32"), ref, A)[0])
        return self._refs[variant]


def _x3_walk(B, q_total, rows_total, vr):
    return (B * ((q_total + 255) // 256), (rows_total + vr - 1) // vr)


def conv_cases():
    cs = []
    # ---- taps: every (kernel, dilation) the ABI takes.  Cout = 64: rows_pad = 64 is no multiple of 128, so wg_rows = 128 falls back to the
    # 64-row forms -- k = 3 / 7 reach <KW,2,2,4,3>, k = 11 reaches <11,2,4,4,2> in both x3 forms
    for KW in (3, 7, 11):
        for d in (1, 2, 3, 4, 5):
            r = K11 if KW == 11 else R64
            cs.append(ConvCase(f"taps_k{KW}d{d}", "taps", "conv", B=2, cin=24, cout=64, T=300, KW=KW, dil=d, reach={"x3": r, "x3w": r}))
            for C_ in (32, 64):
                cs.append(ConvCase(f"taps_mrf_k{KW}d{d}_c{C_}", "taps", "mrf", B=2, cin=C_, cout=C_, T=300, KW=KW, dil=d, variants=("plain", "conv2"), forms=("mrf",)))
    # ---- time seams.  conv: Cout = 24 <= 32 rows: <KW,1,2,4,3> for every k (wg_rows is not looked at)
    for KW, d in ((3, 1), (7, 5), (11, 5)):
        for T in (1, 2, 3, 255, 256, 257, 513):
            cs.append(ConvCase(f"seam_k{KW}d{d}_T{T}", "seams", "conv", B=2, cin=20, cout=24, T=T, KW=KW, dil=d, variants=("plain", "conv2"),
                               reach={"x3": NARROW, "x3w": NARROW}))
        for i, T in enumerate((1, MRF_VT2[KW] - 1, MRF_VT2[KW], MRF_VT2[KW] + 1, 2 * MRF_VT2[KW] + 1)):
            C_ = 64 if (i + KW) % 2 else 32
            cs.append(ConvCase(f"seam_mrf_k{KW}d{d}_T{T}_c{C_}", "seams", "mrf", B=2, cin=C_, cout=C_, T=T, KW=KW, dil=d, variants=("plain", "conv2"), forms=("mrf",)))
    # transposed: the window walk runs over q in [0, T_in]: T_in = 255 is one full window, 256 opens a second one for a single column.
    # up 8, 32 -> 16: 128 rows = rows_pad: 64-row T<2,2,2,4,3> by default, wide T<2,2,2,8,2> with wg_rows = 128.  up 2, 64 -> 32: 64 rows:
    # the streaming kernel up2_stream<4> unless wg_rows = -1, then T<2,2,2,4,3>
    for T in (1, 255, 256, 257):
        cs.append(ConvCase(f"seam_up8_T{T}", "seams", "tconv", B=2, cin=32, cout=16, T=T, up=8, reach={"x3": T_R64, "x3w": T_WIDE}))
        cs.append(ConvCase(f"seam_up2_T{T}", "seams", "tconv", B=2, cin=64, cout=32, T=T, up=2, forms=("f32", "stream", "generic"),
                           reach={"stream": STREAM4, "generic": T_R64}))
    # ---- valid lengths on every form, plain and in the conv2 form.  Seam = 256 (window) / VT2 (mrf); T % 4 == 0, so the f32 kernels stage
    # float4s that straddle a length.  Cout = 65: rows_pad 128: <KW,2,2,4,3> with two row tiles, and the 128-row <KW,2,2,8,2>
    both = ("plain", "conv2")
    cl = lambda seam, T: [-3, 0, 1, seam - 1, seam, seam + 1, T]
    cs.append(ConvCase("len_k7d3", "lengths", "conv", B=7, cin=20, cout=65, T=300, KW=7, dil=3, lens=cl(256, 300), variants=both, reach={"x3": R64, "x3w": WIDE}))
    cs.append(ConvCase("len_k11d5_narrow", "lengths", "conv", B=7, cin=20, cout=24, T=300, KW=11, dil=5, lens=cl(256, 300), variants=both, forms=("f32", "x3"),
                       reach={"x3": NARROW}))
    cs.append(ConvCase("len_k11d3_wide", "lengths", "conv", B=7, cin=20, cout=128, T=300, KW=11, dil=3, lens=cl(256, 300), variants=both, reach={"x3": K11, "x3w": WIDE}))
    cs.append(ConvCase("len_up8", "lengths", "tconv", B=7, cin=32, cout=16, T=300, up=8, lens=cl(256, 300), variants=both, reach={"x3": T_R64, "x3w": T_WIDE}))
    cs.append(ConvCase("len_up8_512rows", "lengths", "tconv", B=7, cin=64, cout=64, T=260, up=8, lens=cl(256, 260), variants=both, reach={"x3": T_R64, "x3w": T_WIDE}))
    cs.append(ConvCase("len_up2_c64", "lengths", "tconv", B=7, cin=64, cout=32, T=300, up=2, lens=cl(256, 300), variants=both, forms=("f32", "stream", "generic"),
                       reach={"stream": STREAM4, "generic": T_R64}))
    cs.append(ConvCase("len_up2_c128", "lengths", "tconv", B=7, cin=128, cout=64, T=300, up=2, lens=cl(256, 300), variants=both, forms=("f32", "stream", "generic"),
                       reach={"stream": STREAM8, "generic": T_R64}))
    for KW, d, C_ in ((3, 3, 64), (7, 5, 32), (11, 3, 64)):
        T = MRF_VT2[KW] + 44
        cs.append(ConvCase(f"len_mrf_k{KW}d{d}_c{C_}", "lengths", "mrf", B=7, cin=C_, cout=C_, T=T, KW=KW, dil=d, lens=cl(MRF_VT2[KW], T), variants=both, forms=("mrf",)))
    # ---- channels: chunk edges of the f32 kernel (8 channels per chunk at k = 3, 4 at k = 7 / 11) and of x3 (16).  Cout = 33: 64-row forms
    for cin in (1, 7, 8, 9, 15, 16, 17, 100):
        cs.append(ConvCase(f"cin{cin}_k3", "channels", "conv", B=2, cin=cin, cout=33, T=70, KW=3, dil=1, forms=("f32", "x3"), reach={"x3": R64}))
        cs.append(ConvCase(f"cin{cin}_k11", "channels", "conv", B=2, cin=cin, cout=33, T=70, KW=11, dil=2, forms=("f32", "x3"), reach={"x3": K11}))
    cs.append(ConvCase("cin512_k3", "channels", "conv", B=2, cin=512, cout=64, T=40, KW=3, dil=1, variants=both, reach={"x3": R64, "x3w": R64}))
    cs.append(ConvCase("cin512_k7_wide", "channels", "conv", B=1, cin=512, cout=128, T=40, KW=7, dil=1, reach={"x3": R64, "x3w": WIDE}))
    # ---- rows: n_rt 1, 2, 3, 4 of the 64-row forms, pad rows (24, 33, 65), and rows_pad = 192, where wg_rows = 128 must fall back
    for cout in (24, 32, 33, 64, 65, 128, 192, 256):
        for KW, d in ((7, 3), (11, 1)):
            small = NARROW if cout <= 32 else (K11 if KW == 11 else R64)
            big = WIDE if cout in (65, 128, 256) else small
            cs.append(ConvCase(f"cout{cout}_k{KW}", "rows", "conv", B=2, cin=20, cout=cout, T=70, KW=KW, dil=d, variants=both, reach={"x3": small, "x3w": big},
                               fallback=cout == 192))
    # transposed shapes: (16, 8, 2): 16 rows: T<2,1,2,4,3>; (32, 16, 8): 128 rows; (64, 32, 8): 256 rows; the two x2 up-samplers stream
    cs.append(ConvCase("t_16_8_up2", "rows", "tconv", B=2, cin=16, cout=8, T=41, up=2, variants=both, reach={"x3": T_NARROW, "x3w": T_NARROW}))
    cs.append(ConvCase("t_32_16_up8", "rows", "tconv", B=2, cin=32, cout=16, T=41, up=8, variants=both, reach={"x3": T_R64, "x3w": T_WIDE}))
    cs.append(ConvCase("t_64_32_up8", "rows", "tconv", B=2, cin=64, cout=32, T=41, up=8, variants=both, reach={"x3": T_R64, "x3w": T_WIDE}))
    cs.append(ConvCase("t_64_32_up2", "rows", "tconv", B=2, cin=64, cout=32, T=41, up=2, variants=both, forms=("f32", "stream", "generic"), reach={"stream": STREAM4, "generic": T_R64}))
    cs.append(ConvCase("t_128_64_up2", "rows", "tconv", B=2, cin=128, cout=64, T=41, up=2, variants=both, forms=("f32", "stream", "generic"), reach={"stream": STREAM8, "generic": T_R64}))
    # ---- windows: the 1-D walk win = (jj / n_rt) * 8 + xcd of conv_x3_kernel.  n_win in {1, 7, 8, 9, 12, 17}; Cout 64 / 128 / 256 / 512 gives
    # n_rt 1 / 2 / 4 / 8 in the 64-row form and 1 / 1 / 2 / 4 in the 128-row form (Cout = 64: rows_pad 64, falls back to 64 rows)
    for B, T, n_win in ((1, 40, 1), (7, 8, 7), (8, 8, 8), (9, 40, 9), (3, 769, 12), (17, 8, 17)):
        for cout, rt64, rt128 in ((64, 1, 1), (128, 2, 1), (256, 4, 2), (512, 8, 4)):
            cs.append(ConvCase(f"win{n_win}_cout{cout}", "windows", "conv", B=B, cin=8, cout=cout, T=T, KW=3, dil=1, forms=("x3", "x3w"),
                               reach={"x3": R64, "x3w": R64 if cout == 64 else WIDE}, claims={"x3": (n_win, rt64), "x3w": (n_win, rt128)}))
    cs.append(ConvCase("win9_up8", "windows", "tconv", B=3, cin=16, cout=32, T=513, up=8, forms=("x3", "x3w"), reach={"x3": T_R64, "x3w": T_WIDE},
                       claims={"x3": (9, 4), "x3w": (9, 2)}))
    # ---- alignment: T % 4 == 0 with the input pointer one element into its allocation: vec_ok false by address, scalar staging
    cs.append(ConvCase("off1_k7d3", "alignment", "conv", B=2, cin=20, cout=33, T=300, KW=7, dil=3, variants=both, forms=("f32", "x3"), reach={"x3": R64}, in_offset=1))
    cs.append(ConvCase("off1_k3d2", "alignment", "conv", B=2, cin=20, cout=33, T=300, KW=3, dil=2, forms=("f32", "x3"), reach={"x3": R64}, in_offset=1))
    cs.append(ConvCase("off1_up8", "alignment", "tconv", B=2, cin=32, cout=16, T=60, up=8, forms=("f32", "x3"), reach={"x3": T_R64}, in_offset=1))
    cs.append(ConvCase("off1_up2", "alignment", "tconv", B=2, cin=64, cout=32, T=60, up=2, forms=("f32", "stream", "generic"), reach={"stream": STREAM4, "generic": T_R64}, in_offset=1))
    cs.append(ConvCase("off1_mrf_k7d3_c32", "alignment", "mrf", B=2, cin=32, cout=32, T=300, KW=7, dil=3, variants=both, forms=("mrf",), in_offset=1))
    cs.append(ConvCase("off1_mrf_k3d1_c64", "alignment", "mrf", B=2, cin=64, cout=64, T=300, KW=3, dil=1, lens=[300, 123], forms=("mrf",), in_offset=1))
    cs.append(ConvCase("odd_T301_k7d3", "alignment", "conv", B=2, cin=20, cout=33, T=301, KW=7, dil=3, lens=[301, 130], forms=("f32", "x3"), reach={"x3": R64}))
    cs.append(ConvCase("odd_T301_mrf_k11d1", "alignment", "mrf", B=2, cin=32, cout=32, T=301, KW=11, dil=1, lens=[301, 130], forms=("mrf",)))
    # ---- neighbours: the last channel chunk has pad channels (Cin 20 / 100 at 8 and 16 per chunk, 18 at 4 per chunk); in memory they are the
    # next item's first channels
    for cin in (18, 20, 100):
        cs.append(ConvCase(f"nb_cin{cin}_k3", "neighbours", "conv", B=3, cin=cin, cout=33, T=70, KW=3, dil=1, forms=("f32", "x3"), reach={"x3": R64}))
        cs.append(ConvCase(f"nb_cin{cin}_k7", "neighbours", "conv", B=3, cin=cin, cout=128, T=70, KW=7, dil=1, reach={"x3": R64, "x3w": WIDE}))
    # transposed: the f32 kernel walks 16 channels per chunk over a slab padded to 8 (Cin 20 -> 24, 8 -> 8: its last chunk ends past the slab)
    cs.append(ConvCase("nb_cin20_up8", "neighbours", "tconv", B=3, cin=20, cout=16, T=70, up=8, reach={"x3": T_R64, "x3w": T_WIDE}))
    cs.append(ConvCase("nb_cin8_up2", "neighbours", "tconv", B=3, cin=8, cout=4, T=70, up=2, forms=("f32", "x3"), reach={"x3": T_NARROW}))
    assert len({c.name for c in cs}) == len(cs)
    return cs


class PosCase:
    """One posconv problem: n_seq sequences of seq_n rows, lengths lens[seq % B] (None: no length array), KW = 31."""

    def __init__(self, name, seq_n, groups, lens, n_seq=None, resid=True, pad=8):
        self.name, self.seq_n, self.groups, self.lens, self.resid, self.pad = name, seq_n, groups, lens, resid, pad
        self.n_seq = n_seq if n_seq is not None else (len(lens) if lens else 2)
        self.D, self.KW = groups * 64, 31
        self._ops, self._refs = {}, {}

    def ops(self, dtype):
        """x [n_seq seq_n][D], w [D][64][KW], resid in dtype (the kernel's operands), bias fp32."""
        if dtype not in self._ops:
            g = torch.Generator().manual_seed(5000 + self.seq_n * 17 + self.groups)
            o = _Ops()
            o.x = torch.randn(self.n_seq * self.seq_n, self.D, generator=g).to(dtype)
            o.w = (torch.randn(self.D, 64, self.KW, generator=g) / math.sqrt(64 * self.KW)).to(dtype)
            o.bias = torch.randn(self.D, generator=g) * 0.1
            o.resid = torch.randn(self.n_seq * self.seq_n, self.D, generator=g).to(dtype) if self.resid else None
            self._ops[dtype] = o
        return self._ops[dtype]

    def packed(self, dtype):
        """-> (x, resid, starts, total_rows): rows [0, len) of every sequence back to back, s % 3 rows nobody owns behind sequence s (2 at the
        end; finite values)."""
        o, rows = self.ops(dtype), posconv_rows(self.n_seq, self.seq_n, self.lens)
        g = torch.Generator().manual_seed(77)
        xs, rs, starts, r = [], [], [], 0
        for s, (r0, _, L) in enumerate(rows):
            gap = s % 3 if s + 1 < self.n_seq else 2
            starts.append(r)
            xs += [o.x[r0:r0 + L], torch.randn(gap, self.D, generator=g).to(dtype)]
            if o.resid is not None:
                rs += [o.resid[r0:r0 + L], torch.randn(gap, self.D, generator=g).to(dtype)]
            r += L + gap
        return torch.cat(xs, 0), (torch.cat(rs, 0) if rs else None), starts, r

    def refs(self, dtype, layout):
        """-> (refs, As, yardstick) for the operands of dtype in the padded or packed layout; lists over sequences of (first row, tensor)."""
        key = (dtype, layout)
        if key not in self._refs:
            o = self.ops(dtype)
            x, resid, starts = o.x, o.resid, None
            if layout == "packed":
                x, resid, starts, _ = self.packed(dtype)
            kw = dict(n_seq=self.n_seq, seq_n=self.seq_n, groups=self.groups, lens=self.lens, starts=starts)
            ref, A, y32 = (posconv_ref(x, o.w, o.bias, resid, mode=m, **kw) for m in ("f64", "abs", "f32"))
            yard = max([parity_err(y[1], r[1], a[1])[0] for y, r, a in zip(y32, ref, A) if r[1].numel()] or [0.0])
            self._refs[key] = (ref, A, yard)
        return self._refs[key]


def posconv_cases():
    """seq_n at the edges of the f32 kernel's 64-token and the bf16 kernel's 256-token workgroups; lengths 1, seam +- 1 and seq_n, a zero and a
    negative one; n_seq = 2 B (lengths indexed seq % B) where the case has a length array; 16 groups at seq_n = 257."""
    cs = []
    for i, seq_n in enumerate((1, 15, 16, 17, 63, 64, 65, 255, 256, 257, 513)):
        lens = sorted({L for L in (1, 63, 65, 255, 257, seq_n) if L <= seq_n}) + [0, -2]
        groups = 16 if seq_n == 257 else (1 if seq_n in (1, 16, 64, 513) else 2)
        if seq_n == 257:
            lens = [257, 255, 1, 0]
        cs.append(PosCase(f"seq_n{seq_n}", seq_n, groups, lens, n_seq=2 * len(lens), resid=i % 2 == 0, pad=0 if i % 4 == 3 else 8))
    cs.append(PosCase("full_seq_n300", 300, 2, None, n_seq=3, resid=True, pad=8))
    return cs


# ------------------------------------------------------------------------------------ GEMM: float64 reference, launch wrapper, cases
# (tests/test_gemm_gpu.py runs the grid, tests/test_gemm_ref_cpu.py checks the claims made here; profiles/gemm_parity/notes.md)
MODE_STORE, MODE_QKV_ROPE, MODE_GATE_RES, MODE_GATE_STORE = 0, 1, 2, 3
ACT_NONE, ACT_GELU_TANH, ACT_GELU_ERF, ACT_SILU = 0, 1, 2, 3
ACT_SLOPE = 1.13                        # bounds |f'| of tanh-GELU (1.129), erf-GELU (1.129) and SiLU (1.100)
ACT_ALLOW = 8.0 * EPS24                 # x |z_e|: the epilogue's own roundings of f(z) (profiles/gemm_parity/notes.md; checked without a device)
ROPE_FACTOR = 4.0                       # between two fp32 evaluations of one formula
ROPE_THETA = 10000.0
Q_SCALE = 0.125                         # the q tables carry the softmax scale: a q column roped with the k table shows
# the kernels by the names used in the claims: gemm_kernel<T, CFG> and the persistent kernel's two store paths
K_F32_128, K_F32_256 = "gemm_kernel<f32,0>", "gemm_kernel<f32,2>"
K_BF16_128, K_BF16_64, K_BF16_RING, K_BF16_W16 = "gemm_kernel<bf16,0>", "gemm_kernel<bf16,3>", "gemm_kernel<bf16,4>", "gemm_kernel<bf16,2>"
K_PP_STAGED, K_PP_PLAIN = "gemm_pp_kernel/staged", "gemm_pp_kernel/plain"
# form -> (operand dtype, tile argument, rows per tile, BK)
GEMM_FORMS = {"f32_128": (torch.float32, 128, 128, 32), "f32_256": (torch.float32, 256, 256, 32), "bf16_64": (torch.bfloat16, 64, 64, 64),
              "bf16_128": (torch.bfloat16, 128, 128, 64), "bf16_6464": (torch.bfloat16, 6464, 64, 64), "pp": (torch.bfloat16, 256, 256, 64),
              "w16": (torch.bfloat16, 256, 256, 64)}
_FORM_KERNEL = {"f32_128": K_F32_128, "f32_256": K_F32_256, "bf16_64": K_BF16_64, "bf16_128": K_BF16_128, "bf16_6464": K_BF16_RING, "w16": K_BF16_W16}


def gemm_act(z, act):
    """Exact activation of a float64 (or, for the yardstick, fp32) tensor."""
    if act == ACT_GELU_TANH:
        return F.gelu(z, approximate="tanh")
    if act == ACT_GELU_ERF:
        return F.gelu(z)
    if act == ACT_SILU:
        return F.silu(z)
    return z


def rope_angles(pos, theta=ROPE_THETA):
    """float64 [len(pos)][32]: pos x theta^(-2i/64)."""
    return pos.double()[:, None] * theta ** (-torch.arange(32, dtype=torch.float64)[None, :] * 2.0 / 64.0)


def rope_full_tables(seq_n, theta=ROPE_THETA):
    """The four fp32 pair-duplicated tables [seq_n][64] (cos_q, sin_q, cos_k, sin_k); the q tables carry Q_SCALE."""
    ang = torch.repeat_interleave(rope_angles(torch.arange(seq_n), theta), 2, dim=1)
    c, s = ang.cos(), ang.sin()
    return [(c * Q_SCALE).float(), (s * Q_SCALE).float(), c.float(), s.float()]


def rope_compact(cos, sin):
    """[pos][64] (cos, sin) per pair from two pair-duplicated tables: what vv_rope_compact writes."""
    t = torch.empty_like(cos)
    t[:, 0::2], t[:, 1::2] = cos[:, 0::2], sin[:, 0::2]
    return t


def rope_computed_emulation(pos, theta=ROPE_THETA):
    """fp32 emulation of rope_pair_computed's steps up to the argument of v_cos / v_sin -> the angle it stands for, float64 rad in
    [0, 2 pi), [len(pos)][32].  k1 = log2f(theta) / 32 and k0 = fp32(log2(2 pi)) as vvk_gemm sets them; the fma rounds once."""
    f32 = torch.float32
    k1 = (torch.log2(torch.tensor(theta, dtype=f32)) / 32.0).double()
    k0 = torch.tensor(2.6514961294723187, dtype=f32).double()
    ex = -(torch.arange(32, dtype=torch.float64) * k1 + k0).to(f32)             # one rounding: the product is exact in float64
    rev = pos.to(f32)[:, None] * torch.exp2(ex)[None, :]                        # v_exp_f32, then one fp32 product
    fr = rev - torch.floor(rev)                                                 # v_fract_f32: exact
    return fr.double() * (2.0 * math.pi)


_ROPE_MODEL = {}


def rope_angle_model(theta=ROPE_THETA, n_pos=4096):
    """-> (kappa, theta0) of  |angle error| <= kappa 2^-24 angle + theta0, MEASURED on the CPU: the emulation above against the float64
    angle at positions 0 .. n_pos - 1 and all 32 pairs.  kappa: the worst relative figure where the angle is at least one radian (the
    error is a relative one there: roundings of the exponent and the product); theta0: what is left over that line anywhere."""
    if (theta, n_pos) not in _ROPE_MODEL:
        pos = torch.arange(n_pos)
        true = rope_angles(pos, theta)
        d = rope_computed_emulation(pos, theta) - torch.remainder(true, 2.0 * math.pi)
        d = (torch.remainder(d + math.pi, 2.0 * math.pi) - math.pi).abs()
        big = true >= 1.0
        kappa = float((d[big] / (EPS24 * true[big])).max())
        theta0 = float((d - kappa * EPS24 * true).clamp_min(0.0).max())
        _ROPE_MODEL[(theta, n_pos)] = (kappa, theta0)
    return _ROPE_MODEL[(theta, n_pos)]


def gemm_dispatch(bf16_in, out_bytes, M, N, K, lda, ldw, ldc, act, tile, cus=256, chip_share=0):
    """launch() of vv_gemm.hip restated for a chip of `cus` CUs -> the kernel a launch reaches."""
    T = "bf16" if bf16_in else "f32"
    big = tile == 256 or (tile == 0 and M >= 4096 and N % 256 == 0)
    share = 2 if chip_share == 2 else 1
    if bf16_in:
        if tile == 0 and big and N < 3072 and ((M + 255) // 256) * (N // 256) < cus // share:
            big = False
        fits = K >= 128 and act != ACT_GELU_ERF and M * lda * 2 < 2 ** 31 and N * ldw * 2 < 2 ** 31 and M * ldc * out_bytes < 2 ** 31 - 256
        if big and fits:
            return K_PP_STAGED if out_bytes == 2 else K_PP_PLAIN
    if big:
        return f"gemm_kernel<{T},2>"
    if bf16_in:
        if tile == 6464 and M * lda * 2 < 2 ** 31 and N * ldw * 2 < 2 ** 31:
            return K_BF16_RING
        t64 = tile == 64
        if tile == 0:
            t, c = ((M + 127) // 128) * (N // 128), cus // share
            t64 = t <= 3 * c and (2 * t + 3 * c - 1) // (3 * c) <= (t + 2 * c - 1) // (2 * c)
        if t64:
            return K_BF16_64
    return f"gemm_kernel<{T},0>"


_TILE_OF_KERNEL = {K_F32_128: 128, K_F32_256: 256, K_BF16_128: 128, K_BF16_64: 64, K_BF16_RING: 6464, K_BF16_W16: 256, K_PP_STAGED: 256, K_PP_PLAIN: 256}


class GemmCase:
    """One problem of the GEMM grid.  form: key of GEMM_FORMS (the tile argument and the operand dtype); kernel: the kernel the case
    CLAIMS to reach (checked against gemm_dispatch).  rope: None / 'tables' / 'compact' / 'by_row' / 'computed'.  tile: overrides the
    form's tile argument (0 = automatic; the case is then also compared bit for bit with the forced tile the rule names).  twins: more
    tile arguments whose output must be bit-identical."""

    def __init__(self, name, section, form, *, M, N, K, mode=MODE_STORE, act=ACT_NONE, out_f32=False, gated=True, rope=None, seq_n=0, rope_dim=0,
                 use_pos=False, skip_q=False, n_store=0, tile=None, twins=(), kernel=None):
        self.name, self.section, self.form = name, section, form
        self.dtype, form_tile, self.rows_per_tile, self.BK = GEMM_FORMS[form]
        self.tile = form_tile if tile is None else tile
        self.M, self.N, self.K, self.mode, self.act, self.gated = M, N, K, mode, act, gated
        self.bf16_in = self.dtype == torch.bfloat16
        self.out_f32 = out_f32 or not self.bf16_in or mode == MODE_GATE_RES
        self.out_dtype = torch.float32 if self.out_f32 else torch.bfloat16
        self.rope, self.seq_n, self.rope_dim, self.use_pos, self.skip_q, self.n_store, self.twins = rope, seq_n, rope_dim, use_pos, skip_q, n_store, tuple(twins)
        self.kernel = kernel or (_FORM_KERNEL[form] if form != "pp" else (K_PP_PLAIN if self.out_f32 else K_PP_STAGED))
        self.m_tiles = (M + self.rows_per_tile - 1) // self.rows_per_tile
        self._ops, self._refs = None, None

    def store_quantum(self):
        return 4 if self.out_f32 else 8

    def ld(self, padded):
        """-> (lda, ldw, ldc) of the contiguous or the padded launch."""
        return (self.K + 8, self.K + 16, self.N + self.store_quantum()) if padded else (self.K, self.K, self.N)

    def reached(self, padded, tile=None):
        lda, ldw, ldc = self.ld(padded)
        return gemm_dispatch(self.bf16_in, 4 if self.out_f32 else 2, self.M, self.N, self.K, lda, ldw, ldc, self.act, self.tile if tile is None else tile)

    def positions(self):
        """Rope position of every row: a table that is NOT row % seq_n when the case passes one."""
        m = torch.arange(self.M)
        return ((m * 11 + 3) % self.seq_n) if self.use_pos else (m % self.seq_n)

    def ops(self):
        """Operands as the kernel gets them: A [M][K], W [N][K] in the operand dtype (randn, W / sqrt(K)); bias, gate fp32 of UNIT scale;
        x0 fp32 [M][N] (the residual stream); the four rope tables."""
        if self._ops is None:
            g = torch.Generator().manual_seed(sum(ord(ch) * (i + 1) for i, ch in enumerate(self.name)) % 100003)
            o = _Ops()
            o.A = torch.randn(self.M, self.K, generator=g).to(self.dtype)
            o.W = (torch.randn(self.N, self.K, generator=g) / math.sqrt(self.K)).to(self.dtype)
            o.bias, o.gate = torch.randn(self.N, generator=g), torch.randn(self.N, generator=g)
            o.x0 = torch.randn(self.M, self.N, generator=g) if self.mode == MODE_GATE_RES else None
            o.tables = rope_full_tables(self.seq_n) if self.mode == MODE_QKV_ROPE else None
            o.pos = self.positions() if self.mode == MODE_QKV_ROPE else None
            self._ops = o
        return self._ops

    def refs(self):
        """-> the float64 reference of the case (gemm_ref), computed once."""
        if self._refs is None:
            self._refs = gemm_ref(self)
        return self._refs


def _rope_cs(case, o, mode):
    """-> (c, s), each [M][2 rope_dim]: cos and sin per COLUMN of the q and k blocks (pair-duplicated), float64 (fp32 for the yardstick)."""
    D = case.rope_dim
    if case.rope == "computed":
        ang = torch.repeat_interleave(rope_angles(o.pos), 2, dim=1)             # [M][64]
        c, s = ang.cos(), ang.sin()
        if mode == "f32":
            c, s = c.float(), s.float()
        reps = 2 * D // 64
        return c.repeat(1, reps), s.repeat(1, reps)
    conv = (lambda t: t) if mode == "f32" else (lambda t: t.double())
    cq, sq, ck, sk = (conv(t[o.pos]) for t in o.tables)
    h = D // 64
    return torch.cat([cq.repeat(1, h), ck.repeat(1, h)], 1), torch.cat([sq.repeat(1, h), sk.repeat(1, h)], 1)


def gemm_eval(case, o, mode, act=None):
    """The case's expression on operands o.  mode 'f64': the float64 reference; 'abs': A_e, the same expression with every operand
    replaced by its absolute value (an activation: 1.13 A_z); 'f32': the yardstick, the CPU library in fp32.  -> (out, z)."""
    act = case.act if act is None else act
    if mode == "f32":
        pos = lambda t: t.float()
    elif mode == "abs":
        pos = lambda t: t.double().abs()
    else:
        pos = lambda t: t.double()
    z = pos(o.A) @ pos(o.W).t() + pos(o.bias)[None, :]
    if case.mode == MODE_STORE:
        if act == ACT_NONE:
            return z, z
        return (ACT_SLOPE * z if mode == "abs" else gemm_act(z, act)), z
    if case.mode == MODE_GATE_STORE:
        return pos(o.gate)[None, :] * z, z
    if case.mode == MODE_GATE_RES:
        return (pos(o.x0) + (pos(o.gate)[None, :] * z if case.gated else z)), z
    D, lo = case.rope_dim, (case.rope_dim if case.skip_q else 0)
    c, s = _rope_cs(case, o, mode)
    if mode == "abs":
        c, s = c.abs(), s.abs()
    out = z.clone()
    a, b = z[:, lo:2 * D:2], z[:, lo + 1:2 * D:2]
    cc, ss = c[:, lo:2 * D:2], s[:, lo:2 * D:2]
    if mode == "abs":
        out[:, lo:2 * D:2], out[:, lo + 1:2 * D:2] = a * cc + b * ss, b * cc + a * ss
    else:
        out[:, lo:2 * D:2], out[:, lo + 1:2 * D:2] = a * cc - b * ss, b * cc + a * ss
    return out, z


def gemm_allow(case, ref, z, o, bf16_out=None):
    """The per-element allowances on top of the accumulation bound: the bf16 store, the activation's own roundings, the fp32 angle of the
    computed rope."""
    bf16_out = (not case.out_f32) if bf16_out is None else bf16_out
    allow = torch.zeros_like(ref)
    if bf16_out:
        allow += BF16_STORE * ref.abs()
    if case.mode == MODE_STORE and case.act != ACT_NONE:
        allow += ACT_ALLOW * z.abs()
    if case.mode == MODE_QKV_ROPE and case.rope == "computed":
        kappa, theta0 = rope_angle_model()
        dth = torch.repeat_interleave(kappa * EPS24 * rope_angles(o.pos) + theta0, 2, dim=1)        # [M][64], per column
        D, lo = case.rope_dim, (case.rope_dim if case.skip_q else 0)
        dth = dth.repeat(1, 2 * D // 64)
        pair = z[:, 0:2 * D:2].abs() + z[:, 1:2 * D:2].abs()
        add = ROPE_FACTOR * dth[:, :2 * D] * torch.repeat_interleave(pair, 2, dim=1)
        allow[:, lo:2 * D] += add[:, lo:]
    return allow


def gemm_ref(case, o=None):
    """-> an object with ref (float64 [M][N]), A (the scale A_e), z (float64 A W^T + bias), allow (gemm_allow), yard (the fp32 CPU library's
    err under the metric, no allowance) and bound."""
    o = case.ops() if o is None else o
    r = _Ops()
    r.ref, r.z = gemm_eval(case, o, "f64")
    r.A, _ = gemm_eval(case, o, "abs")
    r.f32, _ = gemm_eval(case, o, "f32")
    r.allow = gemm_allow(case, r.ref, r.z, o)
    r.yard = parity_err(r.f32, r.ref, r.A)[0]
    r.bound = gemm_bound(r.yard)
    return r


def gemm_bound(yardstick):
    """max(8 x 2^-24, 4 x yardstick): conv_bound's rule, for its reasons -- the floor is one product rounding plus the epilogue's few
    (bias, gate, residual / the rope pair's products), the 4 stands between the kernel's one chain of K / 32 MFMA steps per element and
    the CPU library's vector lanes.  Never fitted to a measurement; tests/test_gemm_ref_cpu.py holds it under (K + 8) 2^-24."""
    return max(8.0 * EPS24, 4.0 * yardstick)


def gemm_written_cols(case):
    """-> (columns below this are compared, columns from this on must keep the fill): n_store, and n_store rounded up to the store quantum."""
    if not case.n_store:
        return case.N, case.N
    q = case.store_quantum()
    return case.n_store, min(case.N, (case.n_store + q - 1) // q * q)


def gemm_launch(eng, case, *, padded, tile=None, o=None, tail=None):
    """One launch of a case -> the M x N view of C on the CPU.  C is a view inside a larger buffer of CONV_FILL: CONV_GUARD rows in front
    and behind, and (padded) 8 / 4 padding columns for bf16 / fp32 output; A and W are views with lda = K + 8 / ldw = K + 16 (padded)
    whose padding columns and two more rows hold NaN; bias and gate are followed by NaN.  The guard rows and padding columns are checked
    after the launch.  Fresh rows of C hold the fill (the residual stream x0 in MODE_GATE_RES)."""
    o = case.ops() if o is None else o
    M, N, K, G = case.M, case.N, case.K, CONV_GUARD
    lda, ldw, ldc = case.ld(padded)
    Ab = torch.full((M + 2, lda), NAN, dtype=case.dtype, device=DEV)
    Wb = torch.full((N + 2, ldw), NAN, dtype=case.dtype, device=DEV)
    Ab[:M, :K], Wb[:N, :K] = o.A.to(DEV), o.W.to(DEV)
    vecs = []
    for v in (o.bias, o.gate):
        t = torch.full((N + 4,), NAN, device=DEV)
        t[:N] = v.to(DEV)
        vecs.append(t[:N])
    Cb = torch.full((G + M + G, ldc), CONV_FILL, dtype=case.out_dtype, device=DEV)
    Cv = Cb[G:G + M, :N]
    if case.mode == MODE_GATE_RES:
        Cv.copy_(o.x0.to(DEV))
    kw = dict(mode=case.mode, act=case.act, out_dtype=rt.VV_F32 if case.out_f32 else rt.VV_BF16, n_store=case.n_store,
              tile=case.tile if tile is None else tile, tail=tail)
    if case.mode in (MODE_GATE_RES, MODE_GATE_STORE) and case.gated:
        kw["gate"] = vecs[1]
    if case.mode == MODE_QKV_ROPE:
        ropes = [t.to(DEV) for t in o.tables]
        if case.rope in ("compact", "by_row"):
            cs = [rope_compact(o.tables[0], o.tables[1]), rope_compact(o.tables[2], o.tables[3])]
            if case.rope == "by_row":
                cs = [t[o.pos] for t in cs]
                kw["rope_by_row"] = 1
            ropes += [t.contiguous().to(DEV) for t in cs]
        kw.update(ropes=ropes, seq_n=case.seq_n, rope_dim=case.rope_dim, rope_skip_q=1 if case.skip_q else 0,
                  rope_theta=ROPE_THETA if case.rope == "computed" else 0.0)
        if case.use_pos:
            kw["rope_pos"] = o.pos.to(torch.int32).to(DEV)
    gemm(eng, Ab[:M, :K], Wb[:N, :K], bias=vecs[0], C_io=Cv, **kw)
    whole = Cb.cpu()
    what = f"{case.name} tile={kw['tile']} padded={padded}"
    assert bool((whole[:G].float() == CONV_FILL).all()), f"{what}: the guard rows in front of C were written"
    assert bool((whole[G + M:].float() == CONV_FILL).all()), f"{what}: the guard rows behind C were written"
    assert bool((whole[G:G + M, N:].float() == CONV_FILL).all()), f"{what}: the padding columns of C were written"
    return whole[G:G + M, :N]


GEMM_M_EDGES = (1, 15, 17, 63, 65, 129, 255, 257)
GEMM_M_WALK = {"f32_128": 1025, "f32_256": 2100, "bf16_64": 577, "bf16_128": 1025, "bf16_6464": 577, "pp": 2100, "w16": 2100}
_BF16_TWINS = (64, 6464, 256)


def gemm_cases():
    """One base shape per form (M = 200, N = 256, K = 2 K-tiles; the persistent kernel K = 128, its 16-wave fallback K = 64) and ONE axis
    varied at a time: M around every tile / wave / MFMA row count and once with m_tiles > 8 and a ragged last tile; N; K in K-tiles;
    every epilogue the form builds; n_store.  The bf16_128 epilogue cases carry the other bf16 tilings as bit-identical twins."""
    cs = []
    for form, (dt, tile, rows, BK) in GEMM_FORMS.items():
        bf = dt == torch.bfloat16
        K0 = 64 if form == "w16" else (128 if bf else 64)
        base = dict(M=200, N=256, K=K0)
        w16_act = dict(act=ACT_GELU_TANH) if form == "w16" else {}
        add = lambda name, section, **kw: cs.append(GemmCase(f"{form}_{name}", section, form, **{**base, **kw}))
        for M in GEMM_M_EDGES + (GEMM_M_WALK[form],):
            add(f"M{M}", "M", M=M, **w16_act)
        for N in ((256, 768) if rows == 256 else (128, 384, 768)):
            add(f"N{N}", "N", N=N, **w16_act)
        if form == "pp":
            ks = (192, 320, 512)
        elif form == "w16":
            ks = ()                     # K = 64 is what routes a plain bf16 launch here; the erf-GELU cases below vary K
        else:
            ks = (BK, 3 * BK, 5 * BK, 512)
        for K in ks:
            add(f"K{K}", "K", K=K)
        if form == "w16":
            for K in (64, 128, 192, 320, 512):
                add(f"erf_K{K}", "K", K=K, act=ACT_GELU_ERF)
            add("erf_M2100", "M", M=2100, K=128, act=ACT_GELU_ERF)
        # ---- epilogues
        tw = dict(twins=_BF16_TWINS) if form == "bf16_128" else {}
        add("store", "epilogue", **tw)
        for an, act in (("gelu_tanh", ACT_GELU_TANH), ("gelu_erf", ACT_GELU_ERF), ("silu", ACT_SILU)):
            kernel = dict(kernel=K_BF16_W16) if (form == "pp" and act == ACT_GELU_ERF) else {}
            add(an, "epilogue", act=act, **tw, **kernel)
        if bf:
            add("store_f32out", "epilogue", out_f32=True, **tw)
            add("gelu_tanh_f32out", "epilogue", act=ACT_GELU_TANH, out_f32=True, **tw)
        add("gate_res", "epilogue", mode=MODE_GATE_RES, **tw)
        add("res_ungated", "epilogue", mode=MODE_GATE_RES, gated=False, **tw)
        add("gate_store", "epilogue", mode=MODE_GATE_STORE, **tw)
        # rope: N = 512 = q | k | v of rope_dim 128 and 128 plain columns behind v (N > 3 rope_dim); M = 200 = 2 sequences of 70 and a ragged third
        rp = dict(mode=MODE_QKV_ROPE, N=512, rope_dim=128, seq_n=70)
        add("rope_tables", "epilogue", rope="tables", **rp, **tw)
        add("rope_tables_pos", "epilogue", rope="tables", use_pos=True, **rp, **tw)
        add("rope_tables_skip_q", "epilogue", rope="tables", skip_q=True, **rp, **tw)
        add("rope_tight", "epilogue", rope="tables", **{**rp, "N": 384 if rows != 256 else 768, "rope_dim": 128 if rows != 256 else 256})
        if bf:
            add("rope_compact", "epilogue", rope="compact", **rp, **tw)
            add("rope_compact_pos", "epilogue", rope="compact", use_pos=True, **rp)
            for sn in (70, 4096):
                Mc = 200 if sn == 70 else 4096 + 200
                add(f"rope_computed_s{sn}", "epilogue", rope="computed", **{**rp, "seq_n": sn, "M": Mc}, **(tw if sn == 70 else {}))
            add("rope_computed_pos_skip_q", "epilogue", rope="computed", use_pos=True, skip_q=True, **{**rp, "seq_n": 4096, "M": 300})
        if form == "pp":
            add("rope_by_row", "epilogue", rope="by_row", **rp)
            add("rope_by_row_pos", "epilogue", rope="by_row", use_pos=True, **rp)
        # ---- n_store (plain store only: the ABI refuses it elsewhere), both output types
        for ns in (100, 132):
            add(f"nstore{ns}", "n_store", n_store=ns, out_f32=not bf, **w16_act)
            if bf:
                add(f"nstore{ns}_f32out", "n_store", n_store=ns, out_f32=True, **w16_act)
    # ---- tile = 0: the automatic choice, bit-identical to the forced form the dispatch rule names
    cs.append(GemmCase("auto_f32_small", "auto", "f32_128", M=200, N=256, K=64, tile=0))
    cs.append(GemmCase("auto_f32_big", "auto", "f32_256", M=4100, N=256, K=32, tile=0))
    cs.append(GemmCase("auto_bf16_small", "auto", "bf16_64", M=200, N=256, K=128, tile=0))
    cs.append(GemmCase("auto_bf16_mid", "auto", "bf16_128", M=12300, N=1024, K=64, tile=0))
    cs.append(GemmCase("auto_bf16_pp", "auto", "pp", M=4096 + 9, N=3072, K=128, tile=0, act=ACT_GELU_TANH))
    assert len({c.name for c in cs}) == len(cs)
    return cs


# the persistent workgroup that walks more than one tile (602 tiles on 256 CUs), whole output; and the split-K tail shape
GEMM_WALK = dict(M=256 * 300 + 77, N=512, K=128)
GEMM_TAIL = dict(M=136 * 256 - 100, N=512, K=512)


def gemm_walk_cases():
    return [GemmCase("pp_walk_gate_store", "walk", "pp", mode=MODE_GATE_STORE, **GEMM_WALK),
            GemmCase("pp_walk_gelu_tanh", "walk", "pp", act=ACT_GELU_TANH, **GEMM_WALK)]


def gemm_tail_case():
    return GemmCase("pp_split_k_tail", "tail", "pp", mode=MODE_GATE_STORE, **GEMM_TAIL)


# ------------------------------------------------------------------------------------ norms and the text kernels: cases, float64 references, bounds
# (tests/test_norm_gpu.py runs the cases on the device, tests/test_norm_ref_cpu.py checks the claims made here without one;
#  profiles/norm_parity/notes.md).  Every reference is float64 on the operands as the kernel receives them; A_e is the same expression on
# absolute values; the metric is parity_err; every bound is max(c 2^-24, 4 x yardstick) with c counted from the kernel's roundings (each
# docstring gives the count) and the yardstick the CPU library in fp32 on the same operands.  No constant is fitted to a device result.

NORM_GUARD = 3                          # guard rows in front of and behind an output with a leading dimension
MISH_SLOPE = 1.09                       # bounds |mish'| (1.0884 at z = 1.49)
# |act_apply(z, mish) - mish(z)| <= 12 x 2^-24 |z|.  The roundings of x t / (t + 2), t = n (n + 2), n = exp2(1.4427 x): the rounded
# argument moves x by one relative rounding (|f'| |x| 2^-24 <= 1.09), v_exp_f32 is good to 1 ulp = 2 x 2^-24 of n, which is a shift of x
# by that much (<= 2 |x| 2^-24 through x tanh'(..) <= |x|), then n + 2, n (n + 2), t + 2, v_rcp_f32 (1 ulp = 2), x t and the last product:
# 7 relative roundings of a value <= |x|.  1.09 + 2 + 7 = 10.1, taken as 12 (tests/test_norm_ref_cpu.py: an fp32 emulation on a dense grid).
MISH_ALLOW = 12.0 * EPS24
EPS_F32 = float(torch.tensor(1e-6, dtype=torch.float32))        # the 1e-6 the kernels hold as a float


def _nan_rows(t, ld, tail_rows):
    """[R][W] host tensor -> device [R + tail_rows][ld] whose padding columns and tail rows hold NaN (float) or 2^30 (int)."""
    R, W = t.shape
    fill = NAN if t.dtype.is_floating_point else 2 ** 30
    buf = torch.full((R + tail_rows, ld), fill, dtype=t.dtype, device=DEV)
    buf[:R, :W] = t.to(DEV)
    return buf


def _nan_tail(t, tail=8, head=0):
    """Any host tensor, flat on the device, `head` NaN elements in front of it and `tail` behind -> (keep-alive, pointer of the data)."""
    fill = NAN if t.dtype.is_floating_point else 2 ** 30
    buf = torch.full((head + t.numel() + tail,), fill, dtype=t.dtype, device=DEV)
    buf[head:head + t.numel()] = t.reshape(-1).to(DEV)
    return buf, buf.data_ptr() + head * t.element_size()


def _pad_intact(buf, R, W, what):
    """The padding of a buffer made by _nan_rows still holds its poison."""
    bad = (lambda v: ~torch.isnan(v)) if buf.dtype.is_floating_point else (lambda v: v != 2 ** 30)
    assert not bool(bad(buf[:R, W:]).any()), f"{what}: a padding column was written"
    assert not bool(bad(buf[R:]).any()), f"{what}: a row behind the last was written"


def _rows_out(R, W, ld, dtype):
    """-> (whole buffer [G + R + G][ld] of CONV_FILL, the [R][ld] view in its middle)."""
    buf = torch.full((R + 2 * NORM_GUARD, ld), CONV_FILL, dtype=dtype, device=DEV)
    return buf, buf[NORM_GUARD:NORM_GUARD + R]


def _rows_out_intact(buf, R, W, what):
    assert bool((buf[:NORM_GUARD] == CONV_FILL).all()) and bool((buf[NORM_GUARD + R:] == CONV_FILL).all()), f"{what}: a guard row was written"
    assert bool((buf[NORM_GUARD:NORM_GUARD + R, W:] == CONV_FILL).all()), f"{what}: a padding column of the output was written"


def _butterfly64(v):
    """wave_sum of vv_common.h on a [..., 64] fp32 tensor: v += v[lane ^ o], o = 32 .. 1; every lane ends with the same sum."""
    lane = torch.arange(64)
    for o in (32, 16, 8, 4, 2, 1):
        v = v + v[..., lane ^ o]
    return v[..., 0]


def mish_f32_emulation(x):
    """act_apply(x, VV_ACT_MISH) step by step in fp32."""
    n = torch.exp2(torch.tensor(1.4426950408889634, dtype=torch.float32) * x)
    t = n * (n + 2.0)
    return torch.where(x > 20.0, x, x * t * (1.0 / (t + 2.0)))


# ---- LayerNorm (ln_mod_kernel)
LN_DATA = ("normal", "mean300", "const", "outlier", "tiny")


@dataclasses.dataclass(frozen=True)
class LnCase:
    name: str
    D: int = 260
    R: int = 5
    out_bf16: bool = False
    delta_bf16: bool = False
    add_one: int = 1
    has_w: bool = True
    has_b: bool = True
    n_delta: int = 0
    keep_x: int = 0
    tail_row0: int = 0
    tail_parts: tuple = (0, 0)          # split-K parts of delta and of delta2 (0 = that delta has no tail)
    data: str = "normal"
    seed: int = 0
    eps: float = 1e-6
    kernel = "ln_mod_kernel"

    @property
    def out_dtype(self):
        return torch.bfloat16 if self.out_bf16 else torch.float32

    @property
    def delta_dtype(self):
        return torch.bfloat16 if self.delta_bf16 else torch.float32

    def ops(self):
        g = torch.Generator().manual_seed(7000 + self.seed)
        R, D = self.R, self.D
        o = _Ops()
        z = torch.randn(R, D, generator=g)
        if self.data == "mean300":
            o.x = 300.0 + 0.03 * z
        elif self.data == "const":
            o.x = (1.7 + 0.25 * torch.arange(R, dtype=torch.float32))[:, None].expand(R, D).contiguous()
        elif self.data == "outlier":
            o.x = z.clone()
            o.x[:, -1] = 1e4
        elif self.data == "tiny":
            o.x = 1e-4 * z
        else:
            o.x = z
        o.w, o.b = torch.randn(D, generator=g) * 0.3, torch.randn(D, generator=g) * 0.3
        o.d = [(torch.randn(R, D, generator=g) * 0.5).to(self.delta_dtype) for _ in range(2)]
        o.t = [torch.randn(max(p, 1), R - self.tail_row0, D, generator=g) * 0.25 for p in self.tail_parts]
        return o

    def refs(self, o=None):
        return ln_ref(self, o)


def ln_delta(case, o, i):
    """What the kernel adds for delta i, as fp32: the delta itself, and on the rows of a split-K tail the fp32 parts summed in part order,
    the SUM rounded once to the delta's dtype."""
    e = o.d[i].float().clone()
    p = case.tail_parts[i]
    if p:
        acc = o.t[i][0].clone()
        for k in range(1, p):
            acc = acc + o.t[i][k]
        e[case.tail_row0:] = acc.to(case.delta_dtype).float()
    return e


def ln_stream(case, o):
    """The fp32 residual stream the kernel normalises (and writes back unless keep_x): (x + d1) + d2, exact."""
    xs = o.x
    for i in range(case.n_delta):
        xs = xs + ln_delta(case, o, i)
    return xs


def _ln_wb(case, o):
    one = float(case.add_one)
    return (o.w if case.has_w else torch.full((case.D,), 1.0 - one)), (o.b if case.has_b else torch.zeros(case.D)), one


def ln_eval(case, o, mode, xs=None):
    xs = ln_stream(case, o) if xs is None else xs
    w, b, one = _ln_wb(case, o)
    if mode == "f32":
        return F.layer_norm(xs, (case.D,), eps=case.eps) * (w + one) + b
    X, wf = xs.double(), w.double() + one
    mean = X.mean(1, keepdim=True)
    rstd = (((X - mean) ** 2).mean(1, keepdim=True) + float(torch.tensor(case.eps, dtype=torch.float32))).rsqrt()
    if mode == "abs":
        return (X.abs() + X.abs().mean(1, keepdim=True)) * rstd * wf.abs() + b.double().abs()
    return (X - mean) * rstd * wf + b.double()


LN_C = 44.0


def ln_bound(yardstick):
    """max(44 x 2^-24, 4 x yardstick).  The roundings of ln_mod_kernel, each relative to a term A_e dominates: the mean takes at most 16
    serial adds per lane (4 register groups x (3 adds of the float4 + 1 accumulate)), 6 shuffle levels and the division: 23, against
    mean|x| rstd |w + one|.  The variance: the subtraction and the square of every term (3 on the square), the same 23 for the sum and the
    division, the + eps: 27, halved by the inverse square root, plus 2 for v_rsq_f32 (1 ulp): 15.5, against |x - mean| rstd |w + one|.
    The affine: x - mean, x rstd, w + one, the product, + b: 5.  23 + 15.5 + 5 = 43.5."""
    return max(LN_C * EPS24, 4.0 * yardstick)


def ln_ref(case, o=None):
    o = case.ops() if o is None else o
    r = _Ops()
    r.xs = ln_stream(case, o)
    r.ref, r.A, r.f32 = ln_eval(case, o, "f64", r.xs), ln_eval(case, o, "abs", r.xs), ln_eval(case, o, "f32", r.xs)
    r.allow = BF16_STORE * r.ref.abs() if case.out_bf16 else None
    r.yard = parity_err(r.f32, r.ref, r.A)[0]
    r.bound = ln_bound(r.yard)
    return r


def ln_emulate(case, o, xs=None):
    """ln_mod_kernel's arithmetic in fp32, in its order: lane l holds the float4s l, l + 64, l + 128, l + 192 of the row."""
    xs = ln_stream(case, o) if xs is None else xs
    R, D = xs.shape
    w, b, one = _ln_wb(case, o)
    X = torch.zeros(R, 1024)
    X[:, :D] = xs
    live = (torch.arange(1024) < D).view(1, 4, 64, 4)
    X = X.view(R, 4, 64, 4)
    def lanes(v):                                         # [R][4 groups][64][4] -> per-lane serial sum over the groups, then the butterfly
        g = (v[..., 0] + v[..., 1]) + (v[..., 2] + v[..., 3])
        s = torch.zeros(R, 64)
        for i in range(4):
            s = s + g[:, i]
        return _butterfly64(s)
    mean = (lanes(X) / torch.tensor(float(D))).view(R, 1, 1, 1)
    a = torch.where(live, X - mean, torch.zeros(()))
    rstd = torch.rsqrt(lanes(a * a) / torch.tensor(float(D)) + torch.tensor(case.eps, dtype=torch.float32)).view(R, 1, 1, 1)
    y = ((X - mean) * rstd).reshape(R, 1024)[:, :D] * (w + one) + b
    return y.to(case.out_dtype)


def ln_launch(eng, case, o, *, padded, expect_error=False, mutate=None):
    """One launch -> (y [R][D] on the CPU in the output dtype, the stream x after the launch [R][D]).  Padded: ldx = D + 4, ldy = D + 8,
    ld_delta = D + 12, NaN in every padding column.  Always: two NaN rows behind x, the deltas and each tail part block, NaN behind w and
    b, NaN in the delta's own tail rows, guard rows around y; all of it checked after the launch."""
    R, D = case.R, case.D
    ldx, ldy, ldd = (D + 4, D + 8, D + 12) if padded else (D, D, D)
    keep = []
    dx = _nan_rows(o.x, ldx, 2)
    ybuf, y = _rows_out(R, D, ldy, case.out_dtype)
    a = rt.vv_ln_args()
    a.out_dtype = rt.VV_BF16 if case.out_bf16 else rt.VV_F32
    a.x, a.ldx, a.y, a.ldy, a.R, a.D, a.add_one, a.eps, a.keep_x = dx.data_ptr(), ldx, y.data_ptr(), ldy, R, D, case.add_one, case.eps, case.keep_x
    if case.has_w:
        kw, a.w = _nan_tail(o.w)
        keep.append(kw)
    if case.has_b:
        kb, a.b = _nan_tail(o.b)
        keep.append(kb)
    a.delta_dtype = rt.VV_BF16 if case.delta_bf16 else rt.VV_F32
    for i in range(case.n_delta):
        d = o.d[i].clone()
        if case.tail_parts[i]:
            d[case.tail_row0:] = NAN                       # the GEMM leaves these rows unwritten: the kernel must not read them
        dd = _nan_rows(d, ldd, 2)
        keep.append(dd)
        if i == 0:
            a.delta, a.ld_delta = dd.data_ptr(), ldd
        else:
            a.delta2 = dd.data_ptr()
        p = case.tail_parts[i]
        if p:
            tr = R - case.tail_row0
            tb = _nan_rows(o.t[i][:p].reshape(p * tr, D), ldd, 2)
            keep.append(tb)
            if i == 0:
                a.delta_tail, a.delta_tail_parts = tb.data_ptr(), p
            else:
                a.delta2_tail, a.delta2_tail_parts = tb.data_ptr(), p
    if any(case.tail_parts):
        a.tail_row0 = case.tail_row0
    if mutate is not None:
        mutate(a)
    rc = eng.lib.vv_layernorm(eng.ctx, C.byref(a), stream())
    torch.cuda.synchronize()
    what = f"{case.name} ({'padded' if padded else 'contiguous'})"
    if expect_error:
        assert rc == -22, (what, rc)
        assert bool((ybuf == CONV_FILL).all()), f"{what}: a refused launch wrote y"
        assert torch.equal(dx[:R, :min(D, ldx)].cpu(), o.x[:, :min(D, ldx)]), f"{what}: a refused launch wrote x"
        return None, None
    check(eng, rc)
    _rows_out_intact(ybuf, R, D, what)
    _pad_intact(dx, R, D, what + " x")
    return y[:, :D].cpu(), dx[:R, :D].cpu()


def ln_cases():
    """One base shape (D = 260: a partly filled second register group; R = 5: a second workgroup with one live wave), one axis at a time."""
    cs = []
    for ob in (False, True):
        for db in (False, True):
            tag = ("bf16" if ob else "f32") + "_" + ("bf16" if db else "f32")
            for D in (4, 60, 252, 256, 260, 512, 1020, 1024):
                cs.append(LnCase(f"ln/{tag}/D{D}", D=D, out_bf16=ob, delta_bf16=db, n_delta=1, seed=D))
    for tag, ob, db in (("f32_f32", False, False), ("bf16_bf16", True, True)):
        k = dict(out_bf16=ob, delta_bf16=db)
        for R in (1, 3, 4, 5, 37):
            cs.append(LnCase(f"ln/{tag}/R{R}", R=R, n_delta=2, seed=100 + R, **k))
        for add_one in (0, 1):
            for hw, hb in ((True, True), (False, True), (True, False), (False, False)):
                cs.append(LnCase(f"ln/{tag}/one{add_one}_w{int(hw)}_b{int(hb)}", add_one=add_one, has_w=hw, has_b=hb, seed=120, **k))
        for nd, keep in ((0, 0), (1, 0), (1, 1), (2, 0), (2, 1)):
            cs.append(LnCase(f"ln/{tag}/delta{nd}_keep{keep}", n_delta=nd, keep_x=keep, seed=130 + nd, **k))
        for parts in (2, 3, 8):
            for r0 in (0, 1, 4):
                for which, tp in (("d1", (parts, 0)), ("d2", (0, parts)), ("both", (parts, parts))):
                    cs.append(LnCase(f"ln/{tag}/tail{parts}_row{r0}_{which}", n_delta=2, tail_row0=r0, tail_parts=tp, seed=140 + parts, **k))
        for data in LN_DATA:
            cs.append(LnCase(f"ln/{tag}/{data}", data=data, seed=150, **k))
    cs.append(LnCase("ln/bf16_bf16/D1020_tail3_keep", D=1020, out_bf16=True, delta_bf16=True, n_delta=2, keep_x=1, tail_row0=4, tail_parts=(3, 3), seed=160))
    cs.append(LnCase("ln/f32_bf16/D4_R1_delta2", D=4, R=1, delta_bf16=True, n_delta=2, seed=161))
    assert len({c.name for c in cs}) == len(cs)
    return cs


def ln_host_cases():
    """For tools/elementwise_host_check.py alone: tail parts with tail_row0 == R, no row in the tail.  vvk_ln_mod refuses that launch
    (test_layernorm_refusals_write_nothing: tail_row0_at_R), so the device never sees it; the kernel must still read no part buffer."""
    return [LnCase(f"ln/{tag}/tail2_rowR_both", n_delta=2, tail_row0=5, tail_parts=(2, 2), out_bf16=b, delta_bf16=b, seed=170)
            for tag, b in (("f32_f32", False), ("bf16_bf16", True))]


# ---- GroupNorm (groupnorm_kernel)
ACT_MISH = 4


@dataclasses.dataclass(frozen=True)
class GnCase:
    name: str
    B: int = 2
    C: int = 8
    T: int = 300
    G: int = 2
    has_gamma: bool = True
    has_beta: bool = True
    act: int = 0
    data: str = "normal"                # normal | mean300 | first<k> | last<k>: that element of every slab set to k x the slab's spread
    offset: int = 0                     # floats between a 16-byte boundary and x / y: 1 takes the scalar path at T % 4 == 0
    seed: int = 0
    eps: float = 1e-5
    kernel = "groupnorm_kernel"

    @property
    def n(self):
        return self.C // self.G * self.T

    @property
    def vec(self):
        return self.T % 4 == 0 and self.offset % 4 == 0 and self.n % 4 == 0

    def ops(self):
        g = torch.Generator().manual_seed(8000 + self.seed)
        o = _Ops()
        z = torch.randn(self.B, self.C, self.T, generator=g)
        o.x = 300.0 + 0.03 * z if self.data == "mean300" else z
        if self.data.startswith(("first", "last")):
            k = float(self.data.lstrip("firstla"))
            slab = o.x.view(self.B, self.G, self.n)
            slab[:, :, 0 if self.data.startswith("first") else -1] = k
        o.gamma, o.beta = torch.randn(self.C, generator=g), torch.randn(self.C, generator=g)
        return o

    def refs(self, o=None):
        return gn_ref(self, o)


def gn_eval(case, o, mode):
    """-> (output, pre-activation z)."""
    ga = o.gamma if case.has_gamma else torch.ones(case.C)
    be = o.beta if case.has_beta else torch.zeros(case.C)
    if mode == "f32":
        z = F.group_norm(o.x, case.G, ga, be, eps=case.eps)
        return (F.mish(z) if case.act == ACT_MISH else z), z
    X = o.x.double().view(case.B, case.G, case.n)
    mean = X.mean(2, keepdim=True)
    rstd = (((X - mean) ** 2).mean(2, keepdim=True) + float(torch.tensor(case.eps, dtype=torch.float32))).rsqrt()
    ga, be = ga.double()[None, :, None], be.double()[None, :, None]
    if mode == "abs":
        z = ((X.abs() + X.abs().mean(2, keepdim=True)) * rstd).view(o.x.shape) * ga.abs() + be.abs()
        return (MISH_SLOPE * z if case.act == ACT_MISH else z), z
    z = ((X - mean) * rstd).view(o.x.shape) * ga + be
    return (F.mish(z) if case.act == ACT_MISH else z), z


def gn_c(case):
    """The roundings of groupnorm_kernel for a slab of n elements, depth = the serial adds of one thread (ceil(n / 4 / 256) + 2 on the
    vector path: the float4's two levels and the accumulate; ceil(n / 256) on the scalar one), + 6 shuffle levels + 2 LDS levels + the
    division = depth + 9 for a sum.  The mean is m0 + d, d = the mean of fl(x - m0): whatever m0's own error, the mean's error is d's:
    the subtraction, the sum (depth + 9) of terms of up to |x| + |m0| <= 2 mean-scale, the last add: 2 (depth + 10) + 1.  The variance:
    3 on each square, depth + 9, - d^2 and + eps: depth + 14, halved, + 2 for v_rsq_f32.  The affine: x - mean, gamma x rstd, the
    product, + beta: 4."""
    depth = (-(-(case.n // 4) // 256) + 2) if case.vec else -(-case.n // 256)
    return 2.0 * (depth + 10) + 1 + (depth + 14) / 2.0 + 2 + 4


def gn_bound(case, yardstick):
    return max(gn_c(case) * EPS24, 4.0 * yardstick)


def gn_ref(case, o=None):
    o = case.ops() if o is None else o
    r = _Ops()
    (r.ref, r.z), (r.A, _), (r.f32, _) = gn_eval(case, o, "f64"), gn_eval(case, o, "abs"), gn_eval(case, o, "f32")
    r.allow = MISH_ALLOW * r.z.abs() if case.act == ACT_MISH else None
    r.yard = parity_err(r.f32, r.ref, r.A)[0]
    r.bound = gn_bound(case, r.yard)
    return r


def _gn_sum(case, v):
    """One workgroup's sum over a slab, [B][G][n] fp32 -> [B][G][1]: thread t takes the float4s (or floats) t, t + 256, ...; wave
    butterflies; (r0 + r1) + (r2 + r3)."""
    B, G, n = v.shape
    if case.vec:
        per = -(-(n // 4) // 256)
        p = torch.zeros(B, G, per * 1024)
        p[..., :n] = v
        p = p.view(B, G, per, 256, 4)
        p = (p[..., 0] + p[..., 1]) + (p[..., 2] + p[..., 3])
    else:
        per = -(-n // 256)
        p = torch.zeros(B, G, per * 256)
        p[..., :n] = v
        p = p.view(B, G, per, 256)
    s = torch.zeros(B, G, 256)
    for i in range(per):
        s = s + p[:, :, i]
    w = _butterfly64(s.view(B, G, 4, 64))
    return ((w[..., 0] + w[..., 1]) + (w[..., 2] + w[..., 3])).unsqueeze(-1)


def gn_emulate(case, o, form="two_pass"):
    """groupnorm_kernel's arithmetic in fp32.  form: two_pass (the kernel), first_shift (the one-pass variance shifted by the slab's
    first element: the kernel before profiles/norm_parity), unshifted (sum and sum of squares of x itself)."""
    X = o.x.view(case.B, case.G, case.n)
    n = torch.tensor(float(case.n))
    if form == "two_pass":
        m0 = _gn_sum(case, X) / n
        a = X - m0
        sd = _gn_sum(case, a) / n
        var = (_gn_sum(case, a * a) / n - sd * sd).clamp_min(0.0)
        mean = m0 + sd
    else:
        p = X[..., :1] if form == "first_shift" else torch.zeros(case.B, case.G, 1)
        a = X - p
        sd = _gn_sum(case, a) / n
        var = (_gn_sum(case, a * a) / n - sd * sd).clamp_min(0.0)
        mean = p + sd
    rstd = torch.rsqrt(var + torch.tensor(case.eps, dtype=torch.float32))
    ga = (o.gamma if case.has_gamma else torch.ones(case.C)).view(1, case.G, -1, 1)
    be = (o.beta if case.has_beta else torch.zeros(case.C)).view(1, case.G, -1, 1)
    z = (X - mean).view(case.B, case.G, case.C // case.G, case.T) * (ga * rstd.unsqueeze(-1)) + be
    z = z.view(o.x.shape)
    return mish_f32_emulation(z) if case.act == ACT_MISH else z


def gn_launch(eng, case, o, *, padded):
    """One launch -> y [B][C][T] on the CPU.  y sits between guard bands of CONV_FILL; gamma and beta are followed by NaN; padded: x has
    NaN in front of and behind it.  `offset` floats shift both x and y off the 16-byte grid."""
    off = case.offset
    head = 4 + off if padded or off else 0
    kx, px = _nan_tail(o.x, tail=8 if padded else 0, head=head)
    ybuf, y = _guarded(o.x.shape, CONV_GUARD + off, CONV_FILL)
    keep, pg, pb = [], None, None
    if case.has_gamma:
        k1, pg = _nan_tail(o.gamma)
        keep.append(k1)
    if case.has_beta:
        k2, pb = _nan_tail(o.beta)
        keep.append(k2)
    check(eng, eng.lib.vv_groupnorm(eng.ctx, px, y.data_ptr(), pg, pb, case.B, case.C, case.T, case.G, case.eps, case.act, stream()))
    torch.cuda.synchronize()
    _bands_intact(ybuf, CONV_GUARD + off, CONV_FILL, case.name)
    return y.cpu()


def gn_cases():
    cs = [GnCase("gn/base")]
    for name, (B, C, T, G) in (("n40", (1, 4, 20, 2)), ("n2400", (1, 8, 600, 2)), ("cpg1", (2, 4, 64, 4)), ("G1", (1, 6, 100, 1)),
                               ("G_eq_C", (1, 8, 36, 8)), ("T301", (2, 8, 301, 2)), ("T303", (2, 8, 303, 2)), ("T1", (1, 8, 1, 2))):
        cs.append(GnCase(f"gn/{name}", B=B, C=C, T=T, G=G, seed=len(cs)))
    cs.append(GnCase("gn/offset1", offset=1, seed=20))
    cs.append(GnCase("gn/offset1_n40", B=1, C=4, T=20, G=2, offset=1, seed=21))
    for hg, hb in ((False, True), (True, False), (False, False)):
        cs.append(GnCase(f"gn/gamma{int(hg)}_beta{int(hb)}", has_gamma=hg, has_beta=hb, seed=22))
    cs.append(GnCase("gn/mish", act=ACT_MISH, seed=23))
    cs.append(GnCase("gn/mish_T301", T=301, act=ACT_MISH, seed=24))
    cs.append(GnCase("gn/mean300", data="mean300", seed=25))
    cs.append(GnCase("gn/mean300_T301", T=301, data="mean300", seed=26))
    for k in (10, 100, 1000):
        for where in ("first", "last"):
            cs.append(GnCase(f"gn/{where}{k}", data=f"{where}{k}", seed=30 + k))
            cs.append(GnCase(f"gn/{where}{k}_n2400", B=1, C=8, T=600, G=2, data=f"{where}{k}", seed=31 + k))
            cs.append(GnCase(f"gn/{where}{k}_T301", T=301, data=f"{where}{k}", seed=32 + k))
    cs.append(GnCase("gn/n200", B=1, C=4, T=100, G=2, seed=19))              # 50 float4s: the last wave sums nothing, the third a part
    assert len({c.name for c in cs}) == len(cs)
    return cs


# ---- the text stack: text_embed_kernel, dwconv_kernel, grn_stats_kernel + grn_apply_kernel
def _lens(lens, n_seq, N):
    """Per-sequence valid length as the kernels take it: seq_len[s % B] clamped to [0, N]; None = N."""
    return [N if lens is None else max(min(lens[s % len(lens)], N), 0) for s in range(n_seq)]


@dataclasses.dataclass(frozen=True)
class TeCase:
    name: str
    B: int = 2
    N: int = 9
    Dt: int = 8
    ld_ids: int = 6
    vocab_rows: int = 5
    text_len: tuple = (4, 6)
    seed: int = 0
    far_ids: bool = False               # ids of -5 and vocab_rows + 3 inside the text: clamped well beyond the table on both sides
    kernel = "text_embed_kernel"

    def ops(self):
        g = torch.Generator().manual_seed(9000 + self.seed)
        o = _Ops()
        # ids walk through vocab_rows - 3 .. vocab_rows + 1 and -2: id + 1 reaches the last row and is clamped beyond it on both sides
        o.ids = (torch.arange(self.B * self.ld_ids).view(self.B, self.ld_ids) % 6 + self.vocab_rows - 4).to(torch.int32)
        o.ids[:, 0] = -2
        if self.far_ids:
            o.ids[:, 0], o.ids[:, 1] = -5, self.vocab_rows + 3
        o.emb, o.pos = torch.randn(self.vocab_rows, self.Dt, generator=g), torch.randn(self.N, self.Dt, generator=g)
        o.text_len = torch.tensor(self.text_len, dtype=torch.int32)
        return o


def te_ref(case, o):
    """fp32, bit for bit: emb[clamp(id)] + pos[t]; the drop half [B, 2 B) and everything behind the text take the filler id 0."""
    out = torch.empty(2 * case.B, case.N, case.Dt)
    for s in range(2 * case.B):
        b = s % case.B
        for t in range(case.N):
            i = int(o.ids[b, t]) + 1 if (s < case.B and t < int(o.text_len[b]) and t < case.ld_ids) else 0
            out[s, t] = o.emb[min(max(i, 0), case.vocab_rows - 1)] + o.pos[t]
    return out


def te_launch(eng, case, o, *, padded):
    """ids carry one row of 2^30 behind them, text_len, emb and pos are followed by NaN / 2^30; padded: emb and pos start 4 floats into
    their allocations behind NaN.  (ld_ids is the kernel's bound on t, not only a stride: it stays the case's.)"""
    ids = _nan_rows(o.ids, case.ld_ids, 1)
    h = 4 if padded else 0
    (k1, pe), (k2, pp), (k3, pl) = _nan_tail(o.emb, head=h), _nan_tail(o.pos, head=h), _nan_tail(o.text_len)
    obuf, out = _guarded((2 * case.B, case.N, case.Dt), CONV_GUARD, CONV_FILL)
    rc = eng.lib.vv_text_embed(eng.ctx, ids.data_ptr(), case.ld_ids, pl, pe, pp, case.vocab_rows, out.data_ptr(), case.B, case.N, case.Dt, stream())
    check(eng, rc)
    torch.cuda.synchronize()
    _bands_intact(obuf, CONV_GUARD, CONV_FILL, case.name)
    return out.cpu()


def te_cases():
    cs = [TeCase("te/base")]
    for name, tl in (("len0", (0, 0)), ("len1", (1, 1)), ("len_ld", (6, 6)), ("len_gt_ld", (8, 50)), ("len_gt_N", (30, 9))):
        cs.append(TeCase(f"te/{name}", text_len=tl, seed=len(cs)))
    cs.append(TeCase("te/N_gt_all", N=20, text_len=(3, 5), seed=10))
    cs.append(TeCase("te/N_lt_ld", N=4, text_len=(6, 2), seed=11))
    cs.append(TeCase("te/B1_Dt4", B=1, Dt=4, text_len=(5,), seed=12))
    cs.append(TeCase("te/Dt100_blocks", B=3, N=40, Dt=100, ld_ids=33, text_len=(33, 1, 17), seed=13))      # more than one workgroup
    cs.append(TeCase("te/far_ids", text_len=(6, 2), far_ids=True, seed=14))
    return cs


@dataclasses.dataclass(frozen=True)
class DwCase:
    name: str
    KW: int = 7
    C: int = 64
    N: int = 40
    B: int = 2
    lens: tuple = (40, 17)              # None: seq_len NULL
    seed: int = 0
    kernel = "dwconv_kernel"

    @property
    def n_seq(self):
        return 2 * self.B

    def ops(self):
        g = torch.Generator().manual_seed(9500 + self.seed)
        o = _Ops()
        o.x = torch.randn(self.n_seq, self.N, self.C, generator=g)
        o.w = torch.randn(self.C, self.KW, generator=g) / math.sqrt(self.KW)
        o.bias = torch.randn(self.C, generator=g) * 0.3
        o.lens = _lens(self.lens, self.n_seq, self.N)
        return o

    def refs(self, o=None):
        return dw_ref(self, o)


def dw_eval(case, o, mode):
    dt = torch.float32 if mode == "f32" else torch.float64
    x, w, b = o.x.to(dt).clone(), o.w.to(dt), o.bias.to(dt)
    for s, L in enumerate(o.lens):
        x[s, L:] = 0.0                                    # input beyond len is zero, exactly as the kernel skips it
    if mode == "abs":
        x, w, b = x.abs(), w.abs(), b.abs()
    return F.conv1d(x.transpose(1, 2), w[:, None, :], b, padding=case.KW // 2, groups=case.C).transpose(1, 2).contiguous()


def dw_bound(case, yardstick):
    """max((KW + 2) x 2^-24, 4 x yardstick): one chain per element, bias first: KW products (one rounding each, together <= 2^-24 A_e)
    and KW adds whose partial sums never exceed A_e; + 1 of room for a compiler that does not contract to FMA."""
    return max((case.KW + 2) * EPS24, 4.0 * yardstick)


def dw_ref(case, o=None):
    o = case.ops() if o is None else o
    r = _Ops()
    r.ref, r.A, r.f32 = dw_eval(case, o, "f64"), dw_eval(case, o, "abs"), dw_eval(case, o, "f32")
    r.allow = None
    r.yard = parity_err(r.f32, r.ref, r.A)[0]
    r.bound = dw_bound(case, r.yard)
    return r


def dw_emulate(case, o):
    """dwconv_kernel in fp32: acc = bias, then += w[c][k] x in tap order, taps outside [0, len) skipped."""
    out = o.bias.expand(case.n_seq, case.N, case.C).clone()
    pad = case.KW // 2
    for k in range(case.KW):
        for s, L in enumerate(o.lens):
            lo, hi = max(0, pad - k), min(case.N, L + pad - k)          # t with 0 <= t + k - pad < L
            if hi > lo:
                out[s, lo:hi] = out[s, lo:hi] + o.w[:, k] * o.x[s, lo + k - pad:hi + k - pad]
    return out


def dw_launch(eng, case, o, *, padded):
    """Input rows at and beyond a sequence's len hold NaN (the kernel must not read them); NaN behind in, w, bias and seq_len; padded:
    in starts 4 floats into its allocation, behind NaN."""
    x = o.x.clone()
    for s, L in enumerate(o.lens):
        x[s, L:] = NAN
    kx, px = _nan_tail(x, head=4 if padded else 0)
    (k1, pw), (k2, pb) = _nan_tail(o.w), _nan_tail(o.bias)
    k3, pl = (None, None) if case.lens is None else _nan_tail(torch.tensor(case.lens, dtype=torch.int32))
    obuf, out = _guarded(o.x.shape, CONV_GUARD, CONV_FILL)
    check(eng, eng.lib.vv_dwconv(eng.ctx, px, out.data_ptr(), pw, pb, pl, case.B, case.n_seq, case.N, case.C, case.KW, stream()))
    torch.cuda.synchronize()
    _bands_intact(obuf, CONV_GUARD, CONV_FILL, case.name)
    return out.cpu()


def dw_cases():
    cs = [DwCase("dw/base")]
    for KW in (3, 7, 31):
        for N in sorted({1, 2, KW // 2, 40}):
            cs.append(DwCase(f"dw/K{KW}_N{N}", KW=KW, N=N, lens=(N, max(N // 2, 1)), seed=len(cs)))
    for C in (4, 100):
        cs.append(DwCase(f"dw/C{C}", C=C, seed=len(cs)))
    for name, lens in (("len0_1", (0, 1)), ("lenN_gtN", (40, 45)), ("len_null", None), ("len_neg", (-3, 39))):
        cs.append(DwCase(f"dw/{name}", lens=lens, seed=len(cs)))
    cs.append(DwCase("dw/B3_K31", KW=31, B=3, lens=(40, 15, 16), seed=len(cs)))
    cs.append(DwCase("dw/K1", KW=1, lens=(40, 0), seed=len(cs)))
    return cs


@dataclasses.dataclass(frozen=True)
class GrnCase:
    name: str
    C: int = 128
    N: int = 40
    B: int = 2
    lens: tuple = (40, 17)
    bf16: bool = False
    zero_channel: int = -1
    seed: int = 0
    kernel = "grn_stats_kernel+grn_apply_kernel"

    @property
    def n_seq(self):
        return 2 * self.B

    @property
    def dtype(self):
        return torch.bfloat16 if self.bf16 else torch.float32

    def ops(self):
        g = torch.Generator().manual_seed(9700 + self.seed)
        o = _Ops()
        o.x = torch.randn(self.n_seq, self.N, self.C, generator=g).to(self.dtype)
        if self.zero_channel >= 0:
            o.x[:, :, self.zero_channel] = 0.0
        o.gamma, o.beta = torch.randn(self.C, generator=g), torch.randn(self.C, generator=g) * 0.3
        o.lens = _lens(self.lens, self.n_seq, self.N)
        return o

    def refs(self, o=None):
        return grn_ref(self, o)


def grn_eval(case, o, mode):
    """-> (y [n_seq][N][C], sumsq [n_seq][C]).  The statistics run over the valid tokens, the apply over all N rows."""
    dt = torch.float32 if mode == "f32" else torch.float64
    x, ga, be = o.x.to(dt), o.gamma.to(dt), o.beta.to(dt)
    ss = torch.stack([(x[s, :L] ** 2).sum(0) for s, L in enumerate(o.lens)])
    g = ss.sqrt()
    nx = (g / (g.mean(1, keepdim=True) + torch.tensor(1e-6, dtype=torch.float32).to(dt)))[:, None, :]
    if mode == "abs":
        return x.abs() * (ga.abs() * nx + 1.0) + be.abs(), ss
    return x * (ga * nx + 1.0) + be, ss


def grn_counts(case, o):
    """(c of the output, c of sumsq).  sumsq: the square, ceil(len / 4) serial adds of a token phase, two LDS levels: S = ceil(len / 4) + 3.
    The output: g = sqrt(sumsq) carries S / 2 + 1; the channel mean another ceil(C / 256) serial adds, 6 shuffle levels, 2 LDS levels and
    the division on top of that; + 1e-6, g / mean, gamma x, + 1, x scale, + beta: 6.  Together S + ceil(C / 256) + 17."""
    S = -(-max(o.lens) // 4) + 3
    return S + -(-case.C // 256) + 17.0, float(S)


def grn_ref(case, o=None):
    o = case.ops() if o is None else o
    r = _Ops()
    (r.ref, r.ss), (r.A, _), (r.f32, r.ss32) = grn_eval(case, o, "f64"), grn_eval(case, o, "abs"), grn_eval(case, o, "f32")
    r.allow = BF16_STORE * r.ref.abs() if case.bf16 else None
    r.yard = parity_err(r.f32, r.ref, r.A)[0]
    c, cs = grn_counts(case, o)
    r.bound = max(c * EPS24, 4.0 * r.yard)
    r.ss_A = r.ss.clamp_min(1e-300)                       # a channel without energy must give an exact zero
    r.ss_yard = parity_err(r.ss32, r.ss, r.ss_A)[0]
    r.ss_bound = max(cs * EPS24, 4.0 * r.ss_yard)
    return r


def grn_emulate(case, o):
    """The two kernels in fp32: phase p sums tokens p, p + 4, ...; (r0 + r1) + (r2 + r3); then the mean over channels by 256 threads."""
    x = o.x.float()
    ss = torch.zeros(case.n_seq, case.C)
    for s, L in enumerate(o.lens):
        ph = []
        for p in range(4):
            acc = torch.zeros(case.C)
            for t in range(p, L, 4):
                acc = acc + x[s, t] * x[s, t]
            ph.append(acc)
        ss[s] = (ph[0] + ph[1]) + (ph[2] + ph[3])
    g = ss.sqrt()
    per = -(-case.C // 256)
    gp = torch.zeros(case.n_seq, per * 256)
    gp[:, :case.C] = g
    part = torch.zeros(case.n_seq, 256)
    for i in range(per):
        part = part + gp[:, i * 256:(i + 1) * 256]
    w = _butterfly64(part.view(case.n_seq, 4, 64))
    mean = (((w[:, 0] + w[:, 1]) + (w[:, 2] + w[:, 3])) / torch.tensor(float(case.C)))[:, None]
    sc = o.gamma * (g / (mean + torch.tensor(1e-6, dtype=torch.float32))) + 1.0
    return (x * sc[:, None, :] + o.beta).to(case.dtype), ss


def grn_launch(eng, case, o, *, padded):
    """In place.  x sits between guard bands (CONV_FILL, finite: the apply pass reads only its own rows); sumsq likewise; NaN behind
    gamma, beta and seq_len.  padded: a wider guard, so that x lands elsewhere on the 16-byte grid."""
    guard = CONV_GUARD + (8 if padded else 0)
    xbuf, x = _guarded(o.x.shape, guard, CONV_FILL, init=o.x, dtype=case.dtype)
    sbuf, ss = _guarded((case.n_seq, case.C), CONV_GUARD, CONV_FILL)
    (k1, pg), (k2, pb) = _nan_tail(o.gamma), _nan_tail(o.beta)
    k3, pl = (None, None) if case.lens is None else _nan_tail(torch.tensor(case.lens, dtype=torch.int32))
    check(eng, eng.lib.vv_grn(eng.ctx, rt.VV_BF16 if case.bf16 else rt.VV_F32, x.data_ptr(), ss.data_ptr(), pg, pb, pl, case.B, case.n_seq,
                              case.N, case.C, stream()))
    torch.cuda.synchronize()
    _bands_intact(xbuf, guard, CONV_FILL, case.name + " x")
    _bands_intact(sbuf, CONV_GUARD, CONV_FILL, case.name + " sumsq")
    return x.cpu(), ss.cpu()


def grn_cases():
    cs = []
    for bf in (False, True):
        tag = "bf16" if bf else "f32"
        cs.append(GrnCase(f"grn/{tag}/base", bf16=bf))
        for C in (64, 192):
            cs.append(GrnCase(f"grn/{tag}/C{C}", C=C, bf16=bf, seed=C))
        for N in (1, 15, 16, 17):
            cs.append(GrnCase(f"grn/{tag}/N{N}", N=N, lens=(N, max(N - 2, 1)), bf16=bf, seed=N))
        for name, lens in (("len0_1", (0, 1)), ("lenN", (40, 40)), ("len_null", None)):
            cs.append(GrnCase(f"grn/{tag}/{name}", lens=lens, bf16=bf, seed=50))
        cs.append(GrnCase(f"grn/{tag}/zero_channel", zero_channel=65, bf16=bf, seed=51))
        cs.append(GrnCase(f"grn/{tag}/C512_B1", C=512, B=1, lens=(33,), bf16=bf, seed=52))       # two channels per thread in the mean
        cs.append(GrnCase(f"grn/{tag}/C320", C=320, bf16=bf, seed=53))                             # the second trip of the mean's loop: one wave of four
        for N in (4, 5):
            cs.append(GrnCase(f"grn/{tag}/N{N}", N=N, lens=(N, N + 5), bf16=bf, seed=54 + N))
        cs.append(GrnCase(f"grn/{tag}/len0_N_gtN", B=3, lens=(0, 40, 45), bf16=bf, seed=60))
    return cs


# ---- mel front end (mel_kernel)
# x |log|.  The build lowers logf(x) in mel_kernel to y = v_log_f32(x), then r = y ln2_hi, r += fma(y, ln2_hi, -r) + y ln2_lo (the kernel's
# assembly: v_log_f32, v_mul 0x3f317217, v_fma, v_fmac 0x3377d1cf, v_fmac 0x3f317217): v_log_f32 is specified to 1 ulp of the base-2
# logarithm, 2 x 2^-24 of it and so of the result; the product by ln 2 is carried in two floats; one rounding of the result (2^-24).
# Together 3 x 2^-24, i.e. up to 1.5 ulp off the correctly rounded float.
MEL_LOG_ALLOW = 3.0 * EPS24


def mel_tables(spec):
    """The fp32 tables the kernel is bound to (pack.py): the periodic Hann window and the filterbank [n_fft / 2 + 1][n_mel]."""
    from vietvoice_tts_amd.model_spec import mel_filterbank
    return torch.hann_window(spec.win_length, periodic=True, dtype=torch.float32), mel_filterbank(spec).float()


@dataclasses.dataclass(frozen=True)
class MelCase:
    name: str
    lens: tuple
    signal: str = "noise"               # noise | zero (item 0 silent) | square (+-full scale, -32768 included) | impulse (sample 0 / the last sample)
    seed: int = 0
    kernel = "mel_kernel"

    def ops(self):
        g = torch.Generator().manual_seed(9900 + self.seed)
        o = _Ops()
        S = max(self.lens)
        a = (torch.randn(2, S, generator=g) * 4000).clamp(-30000, 30000).to(torch.int16)
        if self.signal == "zero":
            a[0] = 0
        elif self.signal == "square":
            hi = (torch.arange(S) // 25) % 2 == 0
            a[:] = torch.where(hi, torch.tensor(32767, dtype=torch.int16), torch.tensor(-32768, dtype=torch.int16))
        elif self.signal == "impulse":
            a[:] = 0
            a[0, 0] = 20000
            a[1, self.lens[1] - 1] = -20000
        for b, L in enumerate(self.lens):
            a[b, L:] = 32767                              # what lies behind audio_len inside ld_audio is never read
        o.audio = a
        return o


def _mel_frames(a, L, spec, window, edge_repeat=False):
    """int16 clip a[:L] -> float64 frames [L // hop + 1][n_fft], centred, reflected without repeating the edge sample, windowed."""
    n_fft, hop = spec.n_fft, spec.hop_length
    pos = torch.arange(L // hop + 1)[:, None] * hop + torch.arange(n_fft)[None, :] - n_fft // 2
    S = max(L, 1)                                         # an empty clip has one frame, of the row's first (padding) sample
    if edge_repeat:
        pos = torch.where(pos < 0, -pos - 1, pos)
        pos = torch.where(pos >= S, 2 * S - 1 - pos, pos)
    else:
        pos = torch.where(pos < 0, -pos, pos)
        pos = torch.where(pos >= S, 2 * (S - 1) - pos, pos)
    pos = pos.clamp(0, S - 1)
    return a[:S].double()[pos] / 32768.0 * window.double()[None, :]


def mel_eval(case, o, spec, mode, variant=None):
    """-> (log-mel [2][F_max][n_mel], linear mel): float64 from the fp32 tables (mode f64), or A_e in the linear domain (mode abs).  Frames
    behind an item's own are zeros.  variant: a deliberately wrong front end (the mutation table of tests/test_norm_ref_cpu.py)."""
    window, fb = mel_tables(spec)
    if variant == "sym_hann":
        window = torch.hann_window(spec.win_length, periodic=False, dtype=torch.float32)
    if variant == "fb_shift":
        fb = torch.roll(fb, 1, dims=1)
    floor = float(torch.tensor(1e-6 if variant == "floor1e-6" else 1e-5, dtype=torch.float32))
    F_max = max(case.lens) // spec.hop_length + 1
    out = torch.zeros(2, F_max, spec.n_mel, dtype=torch.float64)
    lin = torch.zeros_like(out)
    for b, L in enumerate(case.lens):
        fr = _mel_frames(o.audio[b], L, spec, window, edge_repeat=variant == "edge_repeat")
        if mode == "abs":
            l = (math.sqrt(2.0) * fr.abs().sum(1))[:, None] * fb.double().sum(0)[None, :]
        else:
            mag = torch.fft.rfft(fr, dim=1).abs()
            l = (mag ** 2 if variant == "power" else mag) @ fb.double()
        n = fr.shape[0] - (1 if variant == "last_frame_missing" else 0)
        lin[b, :n] = l[:n]
        out[b, :n] = l[:n].clamp_min(floor).log()
    return out, lin


def mel_c(spec):
    """The roundings of mel_kernel against sum |fr|: the window product, the rounded twiddle, the n_fft FMAs of one bin's chain: n_fft + 2
    on re and on im, which is what sqrt(2) sum |fr| bounds for the magnitude; re^2, im^2, their sum and the root: 3; the filterbank's FMAs
    that add something (the most non-zero entries of a column) and the final rounding: K + 1."""
    _, fb = mel_tables(spec)
    return float(spec.n_fft + 2 + 3 + int((fb != 0).sum(0).max()) + 1)


def mel_ref(case, spec, orc, o=None):
    """ref / A / allow in the log domain: A = A_lin / max(lin_ref, 1e-5) (the slope of the log at the clamped reference: a near-silent bin
    is covered by that denominator, not skipped), allow = logf's own ulp.  Frames behind a clip: ref 0, nothing allowed."""
    o = case.ops() if o is None else o
    r = _Ops()
    r.ref, r.lin = mel_eval(case, o, spec, "f64")
    _, A_lin = mel_eval(case, o, spec, "abs")
    floor = float(torch.tensor(1e-5, dtype=torch.float32))
    r.A = (A_lin / r.lin.clamp_min(floor)).clamp_min(1e-300)
    r.allow = MEL_LOG_ALLOW * r.ref.abs()
    r.f32 = torch.zeros(r.ref.shape)
    orc = copy.copy(orc)                                  # the fp32 oracle on the SAME operands: the window and filterbank the kernel is bound to
    orc.window, orc.fb = mel_tables(spec)
    for b, L in enumerate(case.lens):
        m = orc.mel(o.audio[b, :L])
        r.f32[b, :m.shape[0]] = m
    r.yard = parity_err(r.f32, r.ref, r.A, r.allow)[0]
    r.bound = max(mel_c(spec) * EPS24, 4.0 * r.yard)
    return r


def _fma32(a, b, c):
    """fp32 fma through float64: the product of two floats is exact there."""
    return (a.double() * b.double() + c.double()).float()


def mel_emulate(case, o, spec):
    """mel_kernel in fp32: one FMA chain over n per bin with the rounded twiddle table, the magnitude, one FMA chain over the bins."""
    window, fb = mel_tables(spec)
    n_fft, nb = spec.n_fft, spec.n_fft // 2 + 1
    ang = 2.0 * math.pi * torch.arange(n_fft, dtype=torch.float64) / n_fft
    tc, ts = ang.cos().float(), ang.sin().float()
    F_max = max(case.lens) // spec.hop_length + 1
    out = torch.zeros(2, F_max, spec.n_mel)
    k = torch.arange(nb)
    for b, L in enumerate(case.lens):
        fr = ((o.audio[b].float()[:max(L, 1)])[_mel_pos(L, spec)] * torch.tensor(1.0 / 32768.0)) * window[None, :]
        re, im = torch.zeros(fr.shape[0], nb), torch.zeros(fr.shape[0], nb)
        for n in range(n_fft):
            idx = (n * k) & (n_fft - 1)
            re, im = _fma32(fr[:, n, None], tc[idx][None, :], re), _fma32(fr[:, n, None], ts[idx][None, :], im)
        mag = torch.sqrt(re * re + im * im)
        acc = torch.zeros(fr.shape[0], spec.n_mel)
        for j in range(nb):
            acc = _fma32(fb[j][None, :], mag[:, j, None], acc)
        out[b, :fr.shape[0]] = torch.log(acc.clamp_min(1e-5))
    return out


def _mel_pos(L, spec):
    pos = torch.arange(L // spec.hop_length + 1)[:, None] * spec.hop_length + torch.arange(spec.n_fft)[None, :] - spec.n_fft // 2
    S = max(L, 1)
    pos = torch.where(pos < 0, -pos, pos)
    pos = torch.where(pos >= S, 2 * (S - 1) - pos, pos)
    return pos.clamp(0, S - 1)


def mel_launch(eng, case, o, spec, *, padded):
    """-> mel [2][F_max][n_mel] on the CPU.  padded: ld_audio = the longest clip + 37, 32767 in every sample behind an audio_len and in
    a row behind the last; the output sits between guard bands."""
    S = max(case.lens)
    ld = S + (37 if padded else 0)
    a = torch.full((3, ld), 32767, dtype=torch.int16)
    a[:2, :S] = o.audio
    da = a.to(DEV)
    kl, pl = _nan_tail(torch.tensor(case.lens, dtype=torch.int32))
    F_max = S // spec.hop_length + 1
    mbuf, mel = _guarded((2, F_max, spec.n_mel), CONV_GUARD, CONV_FILL)
    mel.fill_(CONV_FILL)
    check(eng, eng.lib.vv_mel(eng.ctx, da.data_ptr(), ld, pl, mel.data_ptr(), 2, F_max, stream()))
    torch.cuda.synchronize()
    _bands_intact(mbuf, CONV_GUARD, CONV_FILL, case.name)
    return mel.cpu()


def mel_cases(spec):
    h, half = spec.hop_length, spec.n_fft // 2
    cs = [MelCase("mel/noise/shortest", (half + 1, half + 1)),
          MelCase("mel/noise/k_hop", (6 * h, 4 * h), seed=1),
          MelCase("mel/noise/k_hop_plus1", (6 * h + 1, 4 * h + 1), seed=2),
          MelCase("mel/noise/k_hop_minus1", (6 * h - 1, 4 * h - 1), seed=3),
          MelCase("mel/noise/one_short", (6 * h + 164, half + 1), seed=4),
          MelCase("mel/zero", (6 * h, 4 * h + 76), signal="zero", seed=5),
          MelCase("mel/square", (6 * h, 6 * h + 1), signal="square", seed=6),
          MelCase("mel/impulse", (6 * h, 6 * h - 1), signal="impulse", seed=7)]
    return cs


def mel_short_cases(spec):
    """Clips the fp32 oracle cannot frame (its reflection needs more than n_fft / 2 samples): no samples (one frame of the row's first
    sample), one sample, n_fft / 2.  Checked against the counted bound alone (mel_ref_counted)."""
    half = spec.n_fft // 2
    return [MelCase("mel/short/0_1", (0, 1), seed=8), MelCase("mel/short/half_half_plus1", (half, half + 1), seed=9)]


def mel_ref_counted(case, spec, o=None):
    """mel_ref without the fp32 oracle: the bound is the count mel_c alone (no yardstick term), so it is never the wider one."""
    o = case.ops() if o is None else o
    r = _Ops()
    r.ref, r.lin = mel_eval(case, o, spec, "f64")
    _, A_lin = mel_eval(case, o, spec, "abs")
    floor = float(torch.tensor(1e-5, dtype=torch.float32))
    r.A = (A_lin / r.lin.clamp_min(floor)).clamp_min(1e-300)
    r.allow = MEL_LOG_ALLOW * r.ref.abs()
    r.f32, r.yard = r.ref.float(), 0.0
    r.bound = mel_c(spec) * EPS24
    return r


def old_metric(got, ref32):
    """The whole-tensor figure the earlier tests bound: max |got - ref| / max |ref| against the fp32 library."""
    return float((got.double() - ref32.double()).abs().max() / (ref32.double().abs().max() + 1e-12))


def norm_line(case, err, r, old, where, bound=None, yard=None):
    b, y = (r.bound if bound is None else bound), (r.yard if yard is None else yard)
    return (f"NORM_PARITY case={case.name} kernel={case.kernel} err={err:.3e} yardstick={y:.3e} bound={b:.3e} "
            f"err/bound={err / b:.3f} old_metric={old:.3e} worst_index={where}")
