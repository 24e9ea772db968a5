"""CPU: the float64 attention reference and the bf16 rounding model that tests/test_attention_gpu.py measures the kernels with.
The reference is checked against torch's scaled_dot_product_attention in float64; the model must stay at or below HALF of TOL_BF16
on every case of the GPU grid -- the bf16 bound is min(TOL_BF16, 3 x model + 2^-8), and a cap that sat below the model's own error
would hide a kernel error behind it.  A seeded case that exceeds it gets other input, never another cap."""
import math

import pytest
import torch
import torch.nn.functional as F

from tests import gpu_util as gu

CASES = gu.attn_cases()


@pytest.mark.parametrize("n_seq,seq_n,heads,lens,q_scale", [(2, 40, 2, [40, 17], 1.0), (3, 129, 1, [129, 64, 1], 0.125), (1, 70, 3, None, 0.3)])
def test_reference_matches_sdpa_float64(n_seq, seq_n, heads, lens, q_scale):
    g = torch.Generator().manual_seed(seq_n)
    dim = heads * 64
    qkv = torch.randn(n_seq * seq_n, 3 * dim + 8, generator=g, dtype=torch.float64)
    refs = gu.attention_ref(qkv, n_seq=n_seq, seq_n=seq_n, heads=heads, lens=lens, q_scale=q_scale)
    for s in range(n_seq):
        L = seq_n if lens is None else lens[s]
        blk = qkv[s * seq_n: s * seq_n + L, :3 * dim].reshape(L, 3, heads, 64).permute(1, 2, 0, 3)      # [3][heads][L][64]
        want = F.scaled_dot_product_attention(blk[0], blk[1], blk[2], scale=q_scale).permute(1, 0, 2)
        ref, vmax = refs[s]
        assert ref.shape == (L, heads, 64) and float((ref - want).abs().max()) < 1e-12
        assert torch.equal(vmax, blk[2].abs().amax(dim=(1, 2)))


def test_reference_packed_rows_base2_and_rope():
    """Packed starts address the same rows as the padded layout; base 2 equals the natural softmax of ln2 x scores; the roped reference
    equals the plain one on q roped by hand."""
    g = torch.Generator().manual_seed(3)
    n_seq, seq_n, heads, lens = 3, 50, 2, [50, 20, 7]
    qkv = torch.randn(n_seq * seq_n, 3 * 128, generator=g, dtype=torch.float64)
    starts, parts, r = [], [], 0
    for s, L in enumerate(lens):
        starts.append(r)
        parts += [qkv[s * seq_n: s * seq_n + L], torch.randn(2, 3 * 128, generator=g, dtype=torch.float64)]
        r += L + 2
    packed = torch.cat(parts, 0)
    shp = dict(n_seq=n_seq, seq_n=seq_n, heads=heads, lens=lens)
    a = gu.attention_ref(qkv, **shp, q_scale=0.5)
    b = gu.attention_ref(packed, **shp, starts=starts, q_scale=0.5)
    assert all(torch.equal(x[0], y[0]) and torch.equal(x[1], y[1]) for x, y in zip(a, b))
    c = gu.attention_ref(qkv, **shp, base2=True)
    d = gu.attention_ref(qkv, **shp, q_scale=math.log(2.0))
    assert max(float((x[0] - y[0]).abs().max()) for x, y in zip(c, d)) < 1e-13
    tab = gu.rope_cs_table(seq_n, 0.125)
    roped = qkv.clone()
    for s in range(n_seq):
        q = qkv[s * seq_n:(s + 1) * seq_n, :128].reshape(seq_n, heads, 32, 2)
        co, si = tab[:, None, 0::2], tab[:, None, 1::2]
        roped[s * seq_n:(s + 1) * seq_n, :128] = torch.stack([q[..., 0] * co - q[..., 1] * si, q[..., 1] * co + q[..., 0] * si], -1).reshape(seq_n, 128)
    e = gu.attention_ref(qkv, **shp, rope_cs_q=tab)
    f = gu.attention_ref(roped, **shp, q_scale=1.0)
    assert max(float((x[0] - y[0]).abs().max()) for x, y in zip(e, f)) < 1e-13
    assert abs(float(tab[0, 0]) - 0.125) < 1e-15 and float(tab[0, 1]) == 0.0


def test_level_family_operands_are_exact_in_bf16_and_q_mul_is_one():
    assert float(torch.tensor(gu.LOG2E_F32, dtype=torch.float32) * torch.tensor(gu.LN2_F32, dtype=torch.float32)) == 1.0
    for case in gu.attn_level_cases():
        d = case.dim
        q0, k0 = case.master[..., 0:d:64], case.master[..., d:2 * d:64]
        assert torch.equal(q0, q0.bfloat16().float()) and torch.equal(k0, k0.bfloat16().float()), case.name


def test_error_metric_is_per_row_and_reports_the_worst():
    n_seq, seq_n, heads = 2, 8, 2
    g = torch.Generator().manual_seed(1)
    qkv = torch.randn(n_seq * seq_n, 3 * 128, generator=g, dtype=torch.float64)
    refs = gu.attention_ref(qkv, n_seq=n_seq, seq_n=seq_n, heads=heads)
    out = torch.cat([r[0].reshape(seq_n, 128) for r in refs], 0)
    out[seq_n + 3, 64 + 9] += 0.5 * float(refs[1][1][1])          # sequence 1, head 1, row 3: half of that head's V range
    out[2, 5] = float("nan")                                       # a nan is the worst error, not an ignored one
    worst, where = gu.attention_errs(out, refs, n_seq=n_seq, seq_n=seq_n, heads=heads)
    assert worst == float("inf") and where == (0, 0, 2)
    out[2, 5] = refs[0][0][2, 0, 5]
    worst, where = gu.attention_errs(out, refs, n_seq=n_seq, seq_n=seq_n, heads=heads)
    assert abs(worst - 0.5) < 1e-12 and where == (1, 1, 3)


@pytest.mark.parametrize("case", CASES, ids=[c.name for c in CASES])
def test_model_error_stays_below_half_the_cap(case):
    for which in ("full", "ragged"):
        _, model_err = gu.attn_case_refs(case, torch.bfloat16, which)
        print(f"\nATTN_MODEL case={case.name} family={case.family} lens={which} model={model_err:.3e}")
        assert model_err <= 0.5 * gu.TOL_BF16, (case.name, which, model_err)


def test_edge_cases_never_leave_the_speculative_range():
    """The packed-equals-padded bit identity of the bf16 kernel is asserted on the edge cases only, where no tile is redone: every log2
    score of every (query, key) pair, rows beyond kv_len included, stays inside +-40 (a half-row sum then stays inside 2^+-45)."""
    for case in gu.attn_edge_cases():
        assert gu.attn_case_max_log2_score(case) < 40.0, case.name
