"""Helpers for the -m gpu parity tests: call single kernels through the C ABI."""
import ctypes as C
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
