"""CPU checks of the norm / mel / text parity harness (tests/gpu_util.py): the float64 references against independently written
formulas, an fp32 emulation of every kernel's summation order (the would-be device output) inside its bound on every case, the stated
ceilings on the bounds, the Mish allowance against an fp32 emulation of act_apply, and the mutations the per-element bounds must reject
-- with what the earlier whole-tensor tolerances make of each (profiles/norm_parity/notes.md holds the table)."""
import math

import pytest
import torch
import torch.nn.functional as F

from tests import gpu_util as gu

EPS = gu.EPS24
LN, GN, DW, GRN, TE = gu.ln_cases(), gu.gn_cases(), gu.dw_cases(), gu.grn_cases(), gu.te_cases()


def _ids(cases):
    return [c.name for c in cases]


def _err(got, r, ref=None, A=None, allow="r"):
    return gu.parity_err(got.double(), r.ref if ref is None else ref, r.A if A is None else A, r.allow if allow == "r" else allow)[0]


# ------------------------------------------------------------------------------------ references against plain formulas
def test_case_lists_cover_what_they_claim():
    assert {c.D for c in LN} == {4, 60, 252, 256, 260, 512, 1020, 1024} and {c.R for c in LN} >= {1, 3, 4, 5, 37}
    assert {(c.out_bf16, c.delta_bf16) for c in LN if c.n_delta} == {(a, b) for a in (False, True) for b in (False, True)}
    assert {(p, c.tail_row0, c.tail_parts[0] > 0, c.tail_parts[1] > 0) for c in LN for p in (max(c.tail_parts),) if p and c.R == 5 and c.D == 260} == \
        {(p, r0, a, b) for p in (2, 3, 8) for r0 in (0, 1, 4) for a, b in ((True, False), (False, True), (True, True))}
    assert {c.data for c in LN} == set(gu.LN_DATA) and {(c.has_w, c.has_b) for c in LN} == {(a, b) for a in (False, True) for b in (False, True)}
    assert any(c.n < 256 for c in GN) and any(c.vec and (c.n // 4) % 256 and c.n // 4 > 256 for c in GN) and any(c.C // c.G == 1 for c in GN)
    assert any(c.G == 1 for c in GN) and any(c.G == c.C for c in GN) and {c.T % 4 for c in GN} >= {0, 1, 3}
    assert any(c.offset == 1 and c.T % 4 == 0 and not c.vec for c in GN)
    assert {c.KW for c in DW} == {1, 3, 7, 31} and {c.C for c in DW} == {4, 64, 100} and any(c.lens is None for c in DW)
    assert {c.C for c in GRN} >= {64, 128, 192} and {c.N for c in GRN} >= {1, 15, 16, 17, 40} and {c.bf16 for c in GRN} == {False, True}


@pytest.mark.parametrize("case", [c for c in LN if c.seed % 3 == 0], ids=lambda c: c.name)
def test_layernorm_reference_agrees_with_the_library_in_float64(case):
    o = case.ops()
    r = case.refs(o)
    w, b, one = gu._ln_wb(case, o)
    plain = F.layer_norm(r.xs.double(), (case.D,), eps=float(torch.tensor(case.eps, dtype=torch.float32))) * (w.double() + one) + b.double()
    assert float(((plain - r.ref).abs() / r.A).max()) < 1e-12
    assert float(r.A.min()) > 0.0 and bool((r.A >= r.ref.abs() * (1 - 1e-12)).all())
    # the stream: deltas as their dtype holds them; a two-part tail is the exact sum rounded to fp32 (one add), then to the delta's dtype
    if all(p in (0, 2) for p in case.tail_parts):
        xs = o.x.clone()
        for i in range(case.n_delta):
            d = o.d[i].float().clone()
            if case.tail_parts[i]:
                d[case.tail_row0:] = (o.t[i][0].double() + o.t[i][1].double()).float().to(case.delta_dtype).float()
            xs = xs + d
        assert torch.equal(xs, r.xs)
    if case.data == "const":                 # a constant row normalises to b: (x - mean) is exactly zero in the reference
        assert float((r.ref - b.double()).abs().max()) < 1e-9


@pytest.mark.parametrize("case", GN[::3], ids=lambda c: c.name)
def test_groupnorm_reference_agrees_with_the_library_in_float64(case):
    o = case.ops()
    r = case.refs(o)
    ga = (o.gamma if case.has_gamma else torch.ones(case.C)).double()
    be = (o.beta if case.has_beta else torch.zeros(case.C)).double()
    z = F.group_norm(o.x.double(), case.G, ga, be, eps=float(torch.tensor(case.eps, dtype=torch.float32)))
    plain = z * torch.tanh(F.softplus(z)) if case.act == gu.ACT_MISH else z
    assert float(((plain - r.ref).abs() / r.A).max()) < 1e-11
    assert float(r.A.min()) > 0.0


def test_dwconv_and_grn_references_agree_with_loops():
    case = gu.DwCase("dw/plain", KW=7, C=8, N=9, B=2, lens=(9, 4))
    o = case.ops()
    r = case.refs(o)
    want = torch.zeros(case.n_seq, case.N, case.C, dtype=torch.float64)
    for s in range(case.n_seq):
        for t in range(case.N):
            acc = o.bias.double().clone()
            for k in range(case.KW):
                tt = t + k - case.KW // 2
                if 0 <= tt < o.lens[s]:
                    acc += o.w[:, k].double() * o.x[s, tt].double()
            want[s, t] = acc
    assert float((want - r.ref).abs().max()) < 1e-13 and o.lens == [9, 4, 9, 4]
    case = gu.GrnCase("grn/plain", C=64, N=6, B=2, lens=(6, 3))
    o = case.ops()
    r = case.refs(o)
    for s in range(case.n_seq):
        x = o.x[s].double()
        g = torch.linalg.vector_norm(x[:o.lens[s]], dim=0)
        want = o.gamma.double() * (x * (g / (g.mean() + gu.EPS_F32))) + o.beta.double() + x
        assert float((want - r.ref[s]).abs().max()) < 1e-13


# ------------------------------------------------------------------------------------ emulations inside the bounds, ceilings on the bounds
@pytest.mark.parametrize("case", LN, ids=_ids(LN))
def test_layernorm_emulation_passes_and_the_bound_has_a_ceiling(case):
    """The would-be device output passes; the yardstick is a real figure and no bound exceeds 2 x 44 x 2^-24."""
    o = case.ops()
    r = case.refs(o)
    assert r.bound == max(gu.LN_C * EPS, 4 * r.yard) and r.bound <= 2 * gu.LN_C * EPS, r.yard / EPS
    assert (r.yard > 0.0 or case.data == "const") and _err(gu.ln_emulate(case, o, r.xs), r) <= r.bound
    out = r.f32.to(case.out_dtype)
    assert _err(out, r) <= r.bound


@pytest.mark.parametrize("case", GN, ids=_ids(GN))
def test_groupnorm_emulation_passes_and_the_bound_has_a_ceiling(case):
    o = case.ops()
    r = case.refs(o)
    c = gu.gn_c(case)
    assert 36.0 <= c <= 60.0 and r.bound <= 2 * c * EPS and 0.0 < r.yard, (c, r.yard / EPS)
    assert _err(gu.gn_emulate(case, o), r) <= r.bound


@pytest.mark.parametrize("case", DW, ids=_ids(DW))
def test_dwconv_emulation_passes_and_the_bound_has_a_ceiling(case):
    o = case.ops()
    r = case.refs(o)
    assert r.bound <= 2 * (case.KW + 2) * EPS and 0.0 < r.yard
    assert _err(gu.dw_emulate(case, o), r) <= r.bound


@pytest.mark.parametrize("case", GRN, ids=_ids(GRN))
def test_grn_emulation_passes_and_the_bound_has_a_ceiling(case):
    o = case.ops()
    r = case.refs(o)
    c, cs = gu.grn_counts(case, o)
    assert r.bound <= 2 * c * EPS and c <= 40 and r.ss_bound <= 3 * cs * EPS          # no yardstick above 1/2 (3/4 for sumsq) of the count
    y, ss = gu.grn_emulate(case, o)
    assert _err(y, r) <= r.bound
    assert _err(ss, r, ref=r.ss, A=r.ss_A, allow=None) <= r.ss_bound


def test_mel_emulation_passes_and_the_bound_has_a_ceiling(tiny_setup):
    spec, _, orc = tiny_setup
    c = gu.mel_c(spec)
    assert spec.n_fft + 6 < c <= spec.n_fft + spec.n_fft // 2 + 7
    for case in gu.mel_cases(spec):
        o = case.ops()
        r = gu.mel_ref(case, spec, orc, o)
        assert r.bound == c * EPS, (case.name, r.yard / EPS)           # the fp32 FFT library sits far below a quarter of the chain's count
        assert _err(gu.mel_emulate(case, o, spec), r) <= r.bound, case.name
        assert max(case.lens) // spec.hop_length + 1 <= 8 and min(case.lens) >= spec.n_fft // 2 + 1


def test_text_embed_reference_clamps_and_fills():
    for case in TE:
        o = case.ops()
        ref = gu.te_ref(case, o)
        assert torch.equal(ref[case.B:], (o.emb[0][None, None, :] + o.pos[None, :, :]).expand(case.B, -1, -1))        # the drop half: filler
        assert int(o.ids.max()) + 1 > case.vocab_rows - 1 and int(o.ids.min()) + 1 < 0                                 # ids clamp on both sides
        for b in range(case.B):
            n = min(int(o.text_len[b]), case.ld_ids, case.N)
            assert torch.equal(ref[b, n:], ref[case.B + b, n:])


# ------------------------------------------------------------------------------------ Mish
def test_mish_allowance_and_slope():
    z = torch.cat([torch.linspace(-30.0, 30.0, 2_000_001), torch.linspace(-1.0, 1.0, 400_001), torch.tensor([0.0, 1e-20, -1e-20, 20.0, 20.000002])]).float()
    got, want = gu.mish_f32_emulation(z).double(), F.mish(z.double())
    ratio = torch.where(z == 0, torch.zeros(()).double(), (got - want).abs() / (EPS * z.double().abs().clamp_min(1e-300)))
    print(f"\nNORM_MISH worst |act_apply - mish| / (2^-24 |z|) = {float(ratio.max()):.2f} at z = {float(z[int(ratio.argmax())]):.4f}")
    assert float(ratio.max()) <= gu.MISH_ALLOW / EPS and bool(torch.isfinite(got).all())
    zz = torch.linspace(-12.0, 12.0, 480_001, dtype=torch.float64, requires_grad=True)
    (d,) = torch.autograd.grad(F.mish(zz).sum(), zz)
    assert 1.088 < float(d.abs().max()) < gu.MISH_SLOPE


# ------------------------------------------------------------------------------------ mutations
def _table(kernel, rows):
    """rows: (mutation, [(case name, err / bound, old metric accepts)]) -> prints one line per mutation, asserts every case caught."""
    missed = []
    for name, res in rows:
        assert res, f"{kernel}/{name}: no case applies"
        caught = [n for n, e, _ in res if e > 1.0]
        print(f"NORM_MUTATION kernel={kernel} mutation={name} cases={len(res)} caught={len(caught)} min_err/bound={min(e for _, e, _ in res):.3g} "
              f"old_tolerance_accepts={sum(1 for _, _, a in res if a)}/{len(res)}")
        missed += [(name, n, e) for n, e, _ in res if not e > 1.0]
    assert not missed, missed


def _ln_with(case, o, r, *, xs=None, mean=None, rstd=None, w=None, b=None, one=None):
    xs = r.xs if xs is None else xs
    w0, b0, one0 = gu._ln_wb(case, o)
    X = xs.double()
    m = X.mean(1, keepdim=True) if mean is None else mean(X)
    v = ((X - X.mean(1, keepdim=True)) ** 2).mean(1, keepdim=True)
    rs = (v + gu.EPS_F32).rsqrt() if rstd is None else rstd(X, v)
    return (X - m) * rs * ((w0 if w is None else w).double() + (one0 if one is None else one)) + (b0 if b is None else b).double()


def test_layernorm_bound_rejects_mutations():
    """Each wrong kernel, stored in the case's output dtype as a device would, misses the bound on every case it applies to."""
    muts = {k: [] for k in ("var_over_D_minus_1", "eps_outside_sqrt", "last_group_out_of_mean", "add_one_ignored", "w_b_shifted_4", "last_row_unwritten",
                            "tail_part_dropped", "two_bf16_steps")}
    for case in LN:
        o = case.ops()
        r = case.refs(o)
        D, R = case.D, case.R
        w0, b0, one0 = gu._ln_wb(case, o)

        def rec(name, y):
            y = y.to(case.out_dtype)
            old = gu.old_metric(y, r.f32) < (1e-2 if case.out_bf16 else 1e-5)
            muts[name].append((case.name, _err(y, r) / r.bound, old))
        # (mean300: A_e carries |x| rstd = 10^4 against outputs of order 1 -- that case checks cancellation, it cannot see a relative error of
        #  the normalised value; a constant row normalises to b whatever the variance)
        if case.data not in ("const", "mean300"):
            rec("var_over_D_minus_1", _ln_with(case, o, r, rstd=lambda X, v: (v * D / (D - 1) + gu.EPS_F32).rsqrt()))
        if case.data == "tiny":                       # where eps = 1e-6 dominates the variance
            rec("eps_outside_sqrt", _ln_with(case, o, r, rstd=lambda X, v: 1.0 / (v.sqrt() + gu.EPS_F32)))
        if D == 260:
            rec("last_group_out_of_mean", _ln_with(case, o, r, mean=lambda X: X[:, :256].sum(1, keepdim=True) / D))
        if case.add_one and case.data != "const":
            rec("add_one_ignored", _ln_with(case, o, r, one=0.0))
        if (case.has_w or case.has_b) and D > 4:          # at D = 4 a shift by four columns is the identity
            rec("w_b_shifted_4", _ln_with(case, o, r, w=torch.roll(w0, 4), b=torch.roll(b0, 4)))
        y = r.ref.clone()
        y[R - 1] = gu.CONV_FILL
        rec("last_row_unwritten", y)
        for i in range(case.n_delta):
            if case.tail_parts[i]:
                xs = o.x
                for j in range(case.n_delta):
                    e = gu.ln_delta(case, o, j)
                    if j == i:
                        acc = o.t[i][0].clone()
                        for k in range(1, case.tail_parts[i] - 1):
                            acc = acc + o.t[i][k]
                        e[case.tail_row0:] = acc.to(case.delta_dtype).float()
                    xs = xs + e
                rec("tail_part_dropped", _ln_with(case, o, r, xs=xs))
                break
        if case.out_bf16 and case.data != "mean300":
            y = r.ref.bfloat16()
            i = int((r.ref.abs() / r.A).argmax())
            flat = y.view(-1).view(torch.int16)
            flat[i] += 2
            rec("two_bf16_steps", y)
    _table("ln_mod_kernel", list(muts.items()))


def test_groupnorm_bound_rejects_mutations():
    """Among them the kernel's earlier form: the one-pass variance shifted by the slab's first element, on the first-element-outlier data."""
    muts = {"channel_off_by_one_at_the_row_end": [], "unshifted_one_pass": [], "first_element_shift": []}
    for case in GN:
        o = case.ops()
        r = case.refs(o)

        def rec(name, y, tol=1e-5):
            muts[name].append((case.name, _err(y, r) / r.bound, gu.old_metric(y, r.f32) < tol))
        if (case.has_gamma or case.has_beta) and case.C > 1 and case.act == 0:
            ga = (o.gamma if case.has_gamma else torch.ones(case.C)).double()
            be = (o.beta if case.has_beta else torch.zeros(case.C)).double()
            z0 = (r.ref - be[None, :, None]) / ga[None, :, None]                     # the normalised value
            ch = ((torch.arange(case.C * case.T) + 1) // case.T).clamp_max(case.C - 1).view(case.C, case.T)
            rec("channel_off_by_one_at_the_row_end", z0 * ga[ch][None] + be[ch][None])
        if case.data == "mean300":
            rec("unshifted_one_pass", gu.gn_emulate(case, o, "unshifted"), tol=2e-3)
        if case.data.startswith("first"):
            rec("first_element_shift", gu.gn_emulate(case, o, "first_shift"))
    _table("groupnorm_kernel", list(muts.items()))


def test_dwconv_bound_rejects_mutations():
    muts = {"causal_padding": [], "mask_at_N_not_len": [], "weights_read_as_KW_by_C": []}
    for case in DW:
        o = case.ops()
        r = case.refs(o)
        x, w, b = o.x.double().clone(), o.w.double(), o.bias.double()
        xz = x.clone()
        for s, L in enumerate(o.lens):
            xz[s, L:] = 0.0

        def conv(xx, ww, left):
            p = F.pad(xx.transpose(1, 2), (left, case.KW - 1 - left))
            return F.conv1d(p, ww[:, None, :], b, groups=case.C).transpose(1, 2)

        def rec(name, y):
            muts[name].append((case.name, _err(y, r) / r.bound, gu.old_metric(y, r.f32) < 2e-3))
        assert float((conv(xz, w, case.KW // 2) - r.ref).abs().max()) < 1e-13
        if max(o.lens) > 0 and case.KW > 1:               # at KW = 1 both paddings are none and [C][KW] is [KW][C]: the two mutations are the identity
            rec("causal_padding", conv(xz, w, case.KW - 1))
        if any(0 < L < case.N for L in o.lens) or (any(L < case.N for L in o.lens) and case.N > 1):
            rec("mask_at_N_not_len", conv(x, w, case.KW // 2))
        if max(o.lens) > 0 and case.KW > 1:
            rec("weights_read_as_KW_by_C", conv(xz, w.reshape(case.KW, case.C).t().contiguous(), case.KW // 2))
    _table("dwconv_kernel", list(muts.items()))


def test_grn_bound_rejects_mutations():
    muts = {"sums_over_padded_tokens": [], "residual_missing": [], "channel_mean_over_C_minus_1": []}
    for case in GRN:
        o = case.ops()
        r = case.refs(o)
        x, ga, be = o.x.double(), o.gamma.double(), o.beta.double()

        def y_of(ss, div=case.C, resid=1.0):
            g = ss.sqrt()
            nx = (g / (g.sum(1, keepdim=True) / div + gu.EPS_F32))[:, None, :]
            y = x * (ga * nx + resid) + be
            return y.bfloat16() if case.bf16 else y

        def rec(name, y):
            muts[name].append((case.name, _err(y, r) / r.bound, gu.old_metric(y, r.f32) < 2e-3))
        assert _err(y_of(r.ss), r) <= 1e-9 or case.bf16
        if any(L < case.N for L in o.lens):
            rec("sums_over_padded_tokens", y_of((x ** 2).sum(1)))
        rec("residual_missing", y_of(r.ss, resid=0.0))
        if max(o.lens) > 0:
            rec("channel_mean_over_C_minus_1", y_of(r.ss, div=case.C - 1))
    _table("grn", list(muts.items()))


def test_mel_bound_rejects_mutations(tiny_setup):
    spec, _, orc = tiny_setup
    names = ("sym_hann", "edge_repeat", "power", "floor1e-6", "fb_shift", "last_frame_missing")
    muts = {k: [] for k in names}
    for case in gu.mel_cases(spec):
        o = case.ops()
        r = gu.mel_ref(case, spec, orc, o)
        for name in names:
            if name == "floor1e-6" and case.signal not in ("zero", "impulse"):
                continue                                  # the floor shows where a bin reaches it: silence, and the bins an impulse leaves empty
            y, _ = gu.mel_eval(case, o, spec, "f64", name)
            # the old test: 1e-4 of the frame peak in the linear domain, 2e-3 in the log domain on the loud bins, per item over its frames
            ok = True
            for b, L in enumerate(case.lens):
                n = L // spec.hop_length + 1
                lg, lr = y[b, :n].exp(), r.f32[b, :n].double().exp()
                loud = lr > 1e-3 * lr.max()
                ok &= float((lg - lr).abs().max()) < 1e-4 * float(lr.max()) and float((y[b, :n] - r.f32[b, :n].double())[loud].abs().max()) < 2e-3
            muts[name].append((case.name, _err(y, r) / r.bound, ok))
    _table("mel_kernel", list(muts.items()))
