"""-m gpu: vv_attention (both kernels) against a float64 reference of the same operands, row by row.

Metric (tests/gpu_util.py attention_errs): per (sequence, head, query row) max_d |got - ref| / max |V| over that head's valid keys --
the output is a convex combination of V rows, so no row can hide behind a large value elsewhere.  Bounds: fp32 TOL_F32; bf16
min(TOL_BF16, 3 x model + 2^-8), model = the float64 rounding model of a bf16 attention on the same case (the kernel makes the same
three roundings at other points -- zero or a bf16 reference instead of the row max, Q rounded after the q_mul product -- so two
independent realisations of equal size give up to ~2x in the worst element; 3 leaves room for v_exp_f32 and the fp32 accumulation
order; 2^-8 is one bf16 output step at full range.  Where one key holds all of a row's weight the model is exact and the kernel
returns bf16(v x bf16(p) / p): those families get two steps, gpu_util.ATTN_DOMINATED_FAMILIES).
tests/test_attention_ref_cpu.py keeps the model at or below half of TOL_BF16 on every case, so the cap cannot hide a kernel error.
Every launch also checks what must NOT be written: padding columns of out, sentinel rows after the last row, packed rows nobody owns.
Each case prints its figures (ATTN_PARITY lines); profiles/attention_parity/notes.md records them per family."""
import pytest
import torch

pytestmark = pytest.mark.gpu

from tests import gpu_util as gu  # noqa: E402

CASES = gu.attn_cases()
GRID = [(c, dt) for c in CASES for dt in c.dtypes()]
FILL, SENTINELS = 7.0, 4
DT_NAME = {torch.float32: "f32", torch.bfloat16: "bf16"}
BY_NAME = {c.name: c for c in CASES}


def _launch(eng, case, dtype, which, ops=None, lens=None, mutate=None):
    """One launch of a case in one layout -> (whole out buffer on the CPU, lens, starts, total_rows)."""
    ops0, q_scale, _ = case.operands(dtype)
    qkv, lens0, starts, rows = case.layout(ops0 if ops is None else ops, which)
    if mutate is not None:
        mutate(qkv, lens0, starts)
    lens = lens0 if lens is None else lens
    tab = case.rope_table()
    out = gu.attention(eng, qkv.to(gu.DEV), n_seq=case.n_seq, seq_n=case.seq_n, heads=case.heads, kv_len=lens, row_start=starts,
                       total_rows=rows if starts is not None else 0, q_scale=q_scale, rope_cs_q=None if tab is None else tab.float().to(gu.DEV),
                       ld_out=case.dim + case.pad_out, sentinel_rows=SENTINELS, fill=FILL)
    return out.cpu(), lens, starts, rows


def _assert_untouched(out, case, lens, starts, rows, tag):
    """Padding columns, sentinel rows and (packed) rows no sequence owns still hold the fill value."""
    assert bool((out[:, case.dim:].float() == FILL).all()), (tag, "padding columns of out were written")
    assert bool((out[rows:].float() == FILL).all()), (tag, "sentinel rows after the last row were written")
    if starts is not None:
        owned = torch.zeros(out.shape[0], dtype=torch.bool)
        for s, L in zip(starts, lens):
            owned[s:s + max(L, 0)] = True
        bad = ((out.float() != FILL).any(dim=1) & ~owned).nonzero().flatten().tolist()
        assert not bad, (tag, "rows owned by no sequence were written", bad[:8])


@pytest.mark.parametrize("case,dtype", GRID, ids=[f"{c.name}-{DT_NAME[dt]}" for c, dt in GRID])
def test_attention_float64_parity(hip_tiny, case, dtype):
    """Sections 2 and 3: every case in the padded layout with every key valid, padded with ragged lengths, and packed; every valid row
    against float64 inside the bound; nothing written outside the owned rows; (fp32, and bf16 where no tile is redone) the packed and
    the padded launch agree bit for bit on rows [0, kv_len).

    Rows where one key holds all of the weight (two_refs, spike) come out as bf16(v x bf16(p) / p) and have a bound of two bf16 steps
    (gpu_util.ATTN_DOMINATED_FAMILIES; profiles/attention_parity/notes.md)."""
    eng = hip_tiny["f32"]
    shp = dict(n_seq=case.n_seq, seq_n=case.seq_n, heads=case.heads)
    outs, refs_of, misses = {}, {}, []
    for which in case.layouts:
        key = "full" if which == "full" else "ragged"
        if key not in refs_of:
            refs_of[key] = gu.attn_case_refs(case, dtype, key)
        refs, model_err = refs_of[key]
        out, lens, starts, rows = _launch(eng, case, dtype, which)
        outs[which] = (out, lens, starts)
        tag = (case.name, DT_NAME[dtype], which)
        _assert_untouched(out, case, lens if lens is not None else [case.seq_n] * case.n_seq, starts, rows, tag)
        err, where = gu.attention_errs(out, refs, **shp, lens=lens, starts=starts)
        bound = gu.attn_case_bound(case, dtype, model_err or 0.0)
        print(f"\nATTN_PARITY case={case.name} family={case.family} dtype={DT_NAME[dtype]} layout={which} err={err:.3e} "
              f"model={-1.0 if model_err is None else model_err:.3e} bound={bound:.3e} worst_seq_head_row={where}")
        if not err <= bound:
            misses.append((tag, f"err {err:.3e} > bound {bound:.3e} at (sequence, head, row) {where}"))
    assert not misses, misses
    # bf16: only where no tile is redone (the edge cases: every log2 score inside +-40, checked in tests/test_attention_ref_cpu.py) --
    # a redo is decided per wave, and the padded launch has the rows >= kv_len in the wave that the packed one does not
    if "ragged" in outs and "packed" in outs and (dtype == torch.float32 or case.family == "edge"):
        (a, lens, _), (b, _, starts) = outs["ragged"], outs["packed"]
        for s, L in enumerate(lens):
            assert torch.equal(a[s * case.seq_n: s * case.seq_n + L, :case.dim], b[starts[s]: starts[s] + L, :case.dim]), \
                (case.name, DT_NAME[dtype], "packed and padded rows differ in sequence", s)


MASK_GRID = [(n, dt) for n in ["seq_n129", "pairs48", "rope_ragged", "spike576", "mixed_first_tile", "flat63"] for dt in BY_NAME[n].dtypes()]


@pytest.mark.parametrize("name,dtype", MASK_GRID, ids=[f"{n}-{DT_NAME[dt]}" for n, dt in MASK_GRID])
def test_masked_rows_cannot_leak(hip_tiny, name, dtype):
    """Padded layout: K and V of the rows >= kv_len[s] replaced by +-1e30 (finite) against zeros there -- a leak through the mask with
    ANY weight moves the output; every valid query row must be bit-identical."""
    case = BY_NAME[name]
    eng = hip_tiny["f32"]
    outs = []
    for big in (0.0, 1.0e30):
        ops, _, _ = case.operands(dtype)
        for s, L in enumerate(case.lens):
            n = case.seq_n - L
            sign = 1.0 - 2.0 * ((torch.arange(n)[:, None] + torch.arange(2 * case.dim)[None, :]) % 2)
            ops[s, L:, case.dim:] = (sign * big).to(ops.dtype)
        outs.append(_launch(eng, case, dtype, "ragged", ops=ops)[0])
    for s, L in enumerate(case.lens):
        a, b = (o[s * case.seq_n: s * case.seq_n + L] for o in outs)
        assert bool(torch.isfinite(b.float()).all()) and torch.equal(a, b), (name, DT_NAME[dtype], "masked rows leak into sequence", s)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
@pytest.mark.parametrize("name", ["seq_n129", "pairs9", "spike200", "mixed_down_then_up"])
def test_packed_neighbours_do_not_matter(hip_tiny, name, dtype):
    """Packed layout: other sequences' contents and lengths -- the one stored right after s included -- and the gap rows changed, or s
    run alone in a buffer of its own: sequence s's rows are bit-identical."""
    case = BY_NAME[name]
    eng = hip_tiny["f32"]
    base, lens, starts, _ = _launch(eng, case, dtype, "packed")
    ops, q_scale, _ = case.operands(dtype)
    picks = sorted({0, case.n_seq // 2, case.n_seq - 2, case.n_seq - 1})
    for s in picks:
        L = lens[s]

        def others(qkv, lens0, starts0, s=s, L=L):
            keep = qkv[starts0[s]: starts0[s] + L].clone()
            g = torch.Generator().manual_seed(55 + s)
            qkv[:, :3 * case.dim] = (torch.randn(qkv.shape[0], 3 * case.dim, generator=g) * 2.0).to(qkv.dtype)
            qkv[starts0[s]: starts0[s] + L] = keep
        new_lens = [lens[i] if i == s else max(1, lens[i] // 2) for i in range(case.n_seq)]
        alt = _launch(eng, case, dtype, "packed", lens=new_lens, mutate=others)[0]
        assert torch.equal(alt[starts[s]: starts[s] + L], base[starts[s]: starts[s] + L]), (name, DT_NAME[dtype], "neighbours change sequence", s)
        own = torch.zeros(L, 3 * case.dim + case.pad_qkv, dtype=ops.dtype)
        own[:, :3 * case.dim] = ops[s, :L]
        alone = gu.attention(eng, own.to(gu.DEV), n_seq=1, seq_n=case.seq_n, heads=case.heads, kv_len=[L], row_start=[0], total_rows=L,
                             q_scale=q_scale, ld_out=case.dim + case.pad_out, sentinel_rows=SENTINELS, fill=FILL).cpu()
        assert torch.equal(alone[:L], base[starts[s]: starts[s] + L]), (name, DT_NAME[dtype], "alone differs from packed for sequence", s)
        assert bool((alone[L:].float() == FILL).all())


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
def test_packed_zero_length_sequence_owns_no_row(hip_tiny, dtype):
    """Packed layout: a sequence with kv_len <= 0 -- first, in the middle, last, zero and negative -- is neither read nor written: its
    row_start is its successor's first row (or total_rows, one row past the buffers), which must keep what its owner computed (or the
    fill value).  The neighbours are correct against float64 and bit-identical to the launch without the empty sequences."""
    eng = hip_tiny["f32"]
    heads, seq_n = 2, 200
    dim = heads * 64
    lens, starts = [0, 70, -3, 129, 0], [0, 0, 70, 70, 199]
    rows = 199
    g = torch.Generator().manual_seed(41)
    qkv = torch.randn(rows + SENTINELS, 3 * dim, generator=g)       # the operand buffer has its own sentinel rows: total_rows stays `rows`
    qkv[:, :dim] *= 0.35
    qkv = qkv.to(dtype)
    out = gu.attention(eng, qkv.to(gu.DEV), n_seq=5, seq_n=seq_n, heads=heads, kv_len=lens, row_start=starts, total_rows=rows,
                       sentinel_rows=SENTINELS, fill=FILL).cpu()
    assert bool((out[rows:].float() == FILL).all()), "the empty last sequence wrote past the last row"
    live = gu.attention(eng, qkv.to(gu.DEV), n_seq=2, seq_n=seq_n, heads=heads, kv_len=[70, 129], row_start=[0, 70], total_rows=rows,
                        sentinel_rows=SENTINELS, fill=FILL).cpu()
    assert torch.equal(out, live), "an empty sequence changed a neighbour's rows"
    shp = dict(n_seq=2, seq_n=seq_n, heads=heads, lens=[70, 129], starts=[0, 70])
    refs = gu.attention_ref(qkv, **shp)
    model_err = gu.attention_errs(gu.attention_model_bf16(qkv, **shp), refs, **shp)[0] if dtype == torch.bfloat16 else 0.0
    err, where = gu.attention_errs(out, refs, **shp)
    bound = gu.TOL_F32 if dtype == torch.float32 else min(gu.TOL_BF16, 3.0 * model_err + gu.BF16_STEP)
    print(f"\nATTN_PARITY case=zero_length family=zero_length dtype={DT_NAME[dtype]} layout=packed err={err:.3e} model={model_err:.3e} "
          f"bound={bound:.3e} worst_seq_head_row={where}")
    assert err <= bound, (err, bound, where)
    # every sequence empty: nothing at all is written
    none = gu.attention(eng, qkv.to(gu.DEV), n_seq=3, seq_n=seq_n, heads=heads, kv_len=[0, 0, -1], row_start=[0, 5, rows], total_rows=rows,
                        sentinel_rows=SENTINELS, fill=FILL).cpu()
    assert bool((none.float() == FILL).all())


def test_padded_zero_length_is_clamped_to_one_key(hip_tiny):
    """Padded layout: the sequence has its seq_n rows whatever the length, and a length <= 0 is taken as 1 (documented in vvtts.h)."""
    eng = hip_tiny["f32"]
    heads, seq_n = 2, 40
    g = torch.Generator().manual_seed(43)
    for dtype in (torch.float32, torch.bfloat16):
        qkv = torch.randn(2 * seq_n, 3 * heads * 64, generator=g).to(dtype)
        a = gu.attention(eng, qkv.to(gu.DEV), n_seq=2, seq_n=seq_n, heads=heads, kv_len=[0, -7]).cpu()
        b = gu.attention(eng, qkv.to(gu.DEV), n_seq=2, seq_n=seq_n, heads=heads, kv_len=[1, 1]).cpu()
        assert torch.equal(a, b)
        for s in range(2):      # one key: every query row is that key's V row x bf16(p) / p, rounded to bf16 -- two roundings of <= 2^-8 relative each
            want = qkv[s * seq_n, 2 * heads * 64:].double()
            got = b[s * seq_n:(s + 1) * seq_n].double()
            tol = 2.0 ** -7 * (1.0 + 2.0 ** -8) if dtype == torch.bfloat16 else 1e-6     # 2^-8 on v, then 2^-8 on v (1 + 2^-8)
            assert bool(((got - want[None, :]).abs() <= tol * want.abs()[None, :]).all())
