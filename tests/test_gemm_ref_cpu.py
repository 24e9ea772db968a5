"""CPU checks of the GEMM parity harness (tests/gpu_util.py): the float64 references against independently written plain formulas, the
yardsticks and the bounds, the activation allowance against an fp32 emulation of act_pair, the measured angle error of the computed rope,
the kernel every case claims to reach against a restatement of launch(), and the mutations the per-element bound must reject."""
import math

import pytest
import torch

from tests import gpu_util as gu

CASES = gu.gemm_cases()
BY_NAME = {c.name: c for c in CASES}
SMALL = [c for c in CASES if c.M * c.N <= 300 * 512 and c.section in ("epilogue", "n_store", "K")]
EPS = gu.EPS24


def _ids(cases):
    return [c.name for c in cases]


# ------------------------------------------------------------------------------------ references
def _plain(case):
    """The case's expression written again without gemm_eval: a broadcast product summed over k, textbook activations, the rope pair as a
    complex product with the angle pos / theta^(2 i / 64)."""
    o = case.ops()
    A, W = o.A.double(), o.W.double()
    z = torch.einsum("mk,nk->mn", A, W) + o.bias.double()[None, :]
    if case.mode == gu.MODE_STORE:
        if case.act == gu.ACT_GELU_TANH:
            return 0.5 * z * (1.0 + torch.tanh(math.sqrt(2.0 / math.pi) * (z + 0.044715 * z ** 3)))
        if case.act == gu.ACT_GELU_ERF:
            return 0.5 * z * (1.0 + torch.erf(z / math.sqrt(2.0)))
        if case.act == gu.ACT_SILU:
            return z / (1.0 + torch.exp(-z))
        return z
    if case.mode == gu.MODE_GATE_STORE:
        return z * o.gate.double()[None, :]
    if case.mode == gu.MODE_GATE_RES:
        return o.x0.double() + (z * o.gate.double()[None, :] if case.gated else z)
    D, lo = case.rope_dim, (case.rope_dim if case.skip_q else 0)
    cols = torch.arange(lo, 2 * D, 2)
    i = (cols % 64) // 2
    if case.rope == "computed":
        rot = torch.polar(torch.ones(case.M, len(cols), dtype=torch.float64), o.pos.double()[:, None] / gu.ROPE_THETA ** (2.0 * i.double()[None, :] / 64.0))
    else:
        q = (cols < D)[None, :]
        rot = torch.complex(torch.where(q, o.tables[0][o.pos][:, cols % 64], o.tables[2][o.pos][:, cols % 64]).double(),
                            torch.where(q, o.tables[1][o.pos][:, cols % 64], o.tables[3][o.pos][:, cols % 64]).double())
    v = torch.complex(z[:, cols], z[:, cols + 1]) * rot
    out = z.clone()
    out[:, cols], out[:, cols + 1] = v.real, v.imag
    return out


REF_SAMPLE = [c for c in SMALL if c.form in ("f32_128", "pp", "bf16_6464") and c.section != "K"]


@pytest.mark.parametrize("case", REF_SAMPLE, ids=_ids(REF_SAMPLE))
def test_float64_reference_agrees_with_plain_formulas(case):
    r = case.refs()
    plain = _plain(case)
    assert plain.shape == r.ref.shape == (case.M, case.N)
    # (the computed angle: pos x theta^-x against pos / theta^x in float64 differ by 2^-52 of an angle of up to 4095 rad)
    assert float(((plain - r.ref).abs() / r.A).max()) < (4e-12 if case.rope == "computed" else 1e-13)
    assert float(r.A.min()) > 0.0 and bool((r.A >= r.ref.abs() * (1 - 1e-12)).all())
    if case.mode == gu.MODE_QKV_ROPE:       # the tables are what they are said to be: q carries the softmax scale, positions reach past one sequence
        o = case.ops()
        assert torch.equal(o.tables[0], (o.tables[2].double() * gu.Q_SCALE).float()) and 0 <= int(o.pos.min()) and int(o.pos.max()) < case.seq_n
        assert case.use_pos == (not torch.equal(o.pos, torch.arange(case.M) % case.seq_n))
        assert torch.equal(gu.rope_compact(o.tables[2], o.tables[3])[:, 1::2], o.tables[3][:, 0::2])


@pytest.mark.parametrize("case", CASES, ids=_ids(CASES))
def test_yardstick_and_bound(case):
    """Every yardstick is a real figure of at most 64 x 2^-24, and no bound exceeds the classical (K + 8) 2^-24."""
    r = case.refs()
    assert 0.0 < r.yard <= 64 * EPS, r.yard
    assert r.bound == max(8 * EPS, 4 * r.yard) and r.bound <= (case.K + 8) * EPS, (r.bound / EPS, case.K)
    # the would-be device output (the fp32 library, rounded where the form stores bf16) passes its own check
    out = r.f32 if case.out_f32 else r.f32.bfloat16()
    assert gu.parity_err(out, r.ref, r.A, r.allow)[0] <= r.bound


def test_walk_and_tail_cases_claim_the_persistent_kernel():
    for c in gu.gemm_walk_cases() + [gu.gemm_tail_case()]:
        for padded in (False, True):
            assert c.reached(padded) == gu.K_PP_STAGED == c.kernel
        assert c.m_tiles * (c.N // 256) > 256            # more tiles than workgroups: a workgroup walks on


# ------------------------------------------------------------------------------------ the activation allowance
def _act_pair_f32(x, act):
    """act_pair of vv_gemm.hip in fp32, step by step: q = x x; t = x fma(q, k3, k1); x rcp(1 + exp2(t)).  The constants are the fp32
    values of the source's expressions (products of doubles, rounded once: what the compiler folds)."""
    f32 = torch.float32
    tanh = act == gu.ACT_GELU_TANH
    k1 = torch.tensor(-1.4426950408889634, dtype=f32) * torch.tensor(2.0 * 0.7978845608028654 if tanh else 1.0, dtype=f32)
    k3 = torch.tensor(-1.4426950408889634, dtype=f32) * torch.tensor(2.0 * 0.7978845608028654 * 0.044715 if tanh else 0.0, dtype=f32)
    q = x * x
    inner = (q.double() * k3.double() + k1.double()).to(f32)          # fma: one rounding (the product is exact in float64)
    t = x * inner
    d = torch.exp2(t) + 1.0
    return x * (1.0 / d)


@pytest.mark.parametrize("act", [gu.ACT_GELU_TANH, gu.ACT_SILU])
def test_activation_allowance_holds_for_the_emulated_epilogue(act):
    """|act_pair(z) - f(z)| <= 8 x 2^-24 |z| on a dense grid of z in [-30, 30] (fp32 values), f exact in float64."""
    z = torch.cat([torch.linspace(-30.0, 30.0, 2_000_001), torch.linspace(-1.0, 1.0, 400_001), torch.tensor([0.0, 1e-20, -1e-20, 1e-6, -1e-6])]).float()
    got = _act_pair_f32(z, act).double()
    want = gu.gemm_act(z.double(), act)
    assert bool(torch.isfinite(got).all())
    ratio = ((got - want).abs() / (EPS * z.double().abs().clamp_min(1e-300)))
    ratio = torch.where(z == 0, torch.zeros_like(ratio), ratio)
    worst = float(ratio.max())
    print(f"\nGEMM_ACT act={act} worst |act_pair - f| / (2^-24 |z|) = {worst:.2f} at z = {float(z[int(ratio.argmax())]):.4f}")
    assert worst <= gu.ACT_ALLOW / EPS
    assert float((got[z == 0]).abs().max()) == 0.0


def test_activation_slope_bounds_the_derivatives():
    z = torch.linspace(-12.0, 12.0, 480_001, dtype=torch.float64, requires_grad=True)
    for act, top in ((gu.ACT_GELU_TANH, 1.129), (gu.ACT_GELU_ERF, 1.129), (gu.ACT_SILU, 1.100)):
        (d,) = torch.autograd.grad(gu.gemm_act(z, act).sum(), z)
        assert top - 1e-3 < float(d.abs().max()) < top + 1e-3 and float(d.abs().max()) < gu.ACT_SLOPE


# ------------------------------------------------------------------------------------ the computed rope
def test_computed_rope_angle_error_is_measured():
    """kappa and theta0 of |angle error| <= kappa 2^-24 angle + theta0: measured from the fp32 emulation of rope_pair_computed against the
    float64 angle, positions 0..4095, all 32 pairs.  The envelope holds everywhere by construction; what is asserted beyond that is what
    the number formats give: the error is a relative one (a handful of roundings), and exact at position 0."""
    kappa, theta0 = gu.rope_angle_model()
    pos = torch.arange(4096)
    true = gu.rope_angles(pos)
    d = gu.rope_computed_emulation(pos) - torch.remainder(true, 2 * math.pi)
    d = (torch.remainder(d + math.pi, 2 * math.pi) - math.pi).abs()
    assert bool((d <= kappa * EPS * true + theta0 + 1e-18).all())
    assert float(d[0].max()) == 0.0
    p0 = float(d[:, 0].max())
    print(f"\nGEMM_ROPE_MODEL kappa={kappa:.2f} theta0={theta0:.3e} rad; worst angle error {float(d.max()):.3e} rad, pair 0: {p0:.3e} rad at position "
          f"{int(d[:, 0].argmax())}, pair 31: {float(d[:, 31].max()):.3e} rad")
    assert 1.0 < kappa < 64.0 and theta0 < 64 * EPS         # roundings of an exponent below 16, one exp2, one product: tens of 2^-24 at most
    # the allowance this grants at the top of the range stays far under one bf16 step of the roped value (2^-8): a position off by one
    # turns pair 0 by a radian
    assert gu.ROPE_FACTOR * (kappa * EPS * 4095 + theta0) < 0.05


# ------------------------------------------------------------------------------------ claims
def test_every_claimed_kernel_is_the_one_the_dispatch_rule_gives():
    reached = set()
    for c in CASES:
        for padded in (False, True):
            assert c.reached(padded) == c.kernel, (c.name, padded, c.reached(padded), c.kernel)
        reached.add(c.kernel)
        if c.tile == 0:
            assert c.reached(True, tile=gu._TILE_OF_KERNEL[c.kernel]) == c.kernel, c.name
        for t in c.twins:
            assert c.N % 256 == 0 and c.reached(True, tile=t) in (gu.K_BF16_64, gu.K_BF16_RING, gu.K_PP_STAGED, gu.K_PP_PLAIN, gu.K_BF16_W16), (c.name, t)
    assert reached == {gu.K_F32_128, gu.K_F32_256, gu.K_BF16_128, gu.K_BF16_64, gu.K_BF16_RING, gu.K_BF16_W16, gu.K_PP_STAGED, gu.K_PP_PLAIN}
    assert {c.kernel for c in CASES if c.tile == 0} == {gu.K_F32_128, gu.K_F32_256, gu.K_BF16_64, gu.K_BF16_128, gu.K_PP_STAGED}
    # the 16-wave fallback is reached both ways: K < 128, and erf-GELU at K >= 128
    w16 = [c for c in CASES if c.kernel == gu.K_BF16_W16]
    assert any(c.K == 64 and c.act != gu.ACT_GELU_ERF for c in w16) and any(c.K >= 128 and c.act == gu.ACT_GELU_ERF for c in w16)
    # the twins of the persistent kernel's two store paths and of its fallback
    tw = {c.reached(True, tile=256) for c in CASES if c.twins}
    assert tw == {gu.K_PP_STAGED, gu.K_PP_PLAIN, gu.K_BF16_W16}


def test_case_list_covers_the_axes():
    for form, (dt, tile, rows, BK) in gu.GEMM_FORMS.items():
        mine = [c for c in CASES if c.form == form and c.tile != 0]
        assert {c.M for c in mine if c.section == "M"} >= set(gu.GEMM_M_EDGES) | {gu.GEMM_M_WALK[form]}, form
        walk = next(c for c in mine if c.M == gu.GEMM_M_WALK[form])
        assert walk.m_tiles > 8 and walk.M % rows, form                       # second group of the mt walk, ragged last tile, early-return blocks
        assert (walk.m_tiles + 7) // 8 * 8 > walk.m_tiles, form
        assert {c.N for c in mine} >= ({256, 768} if rows == 256 else {128, 256, 384, 768}), form
        ks = {c.K for c in mine}
        assert ks >= ({128, 192, 320, 512} if form in ("pp", "w16") else {BK, 2 * BK, 3 * BK, 5 * BK, 512}), form
        assert {c.n_store for c in mine} >= {0, 100, 132}, form
        assert {(c.n_store, c.out_f32) for c in mine if c.n_store} >= {(n, f) for n in (100, 132) for f in ((True,) if dt == torch.float32 else (True, False))}, form
        epi = {(c.mode, c.act, c.gated, c.out_f32) for c in mine}
        for act in (0, 1, 2, 3):
            assert (gu.MODE_STORE, act, True, dt == torch.float32) in epi, (form, act)
        assert {(gu.MODE_GATE_RES, 0, True, True), (gu.MODE_GATE_RES, 0, False, True), (gu.MODE_GATE_STORE, 0, True, dt == torch.float32)} <= epi, form
        ropes = {(c.rope, c.use_pos, c.skip_q) for c in mine if c.mode == gu.MODE_QKV_ROPE}
        assert {("tables", False, False), ("tables", True, False), ("tables", False, True)} <= ropes, form
        assert any(c.N > 3 * c.rope_dim for c in mine if c.rope) and any(c.N == 3 * c.rope_dim for c in mine if c.rope), form
        if dt == torch.bfloat16:
            assert (gu.MODE_STORE, 0, True, True) in epi and (gu.MODE_STORE, 1, True, True) in epi, form
            assert {("compact", False, False), ("computed", False, False), ("computed", True, True)} <= ropes, form
            assert {c.seq_n for c in mine if c.rope == "computed"} == {70, 4096}, form
            assert max(int(c.ops().pos.max()) for c in mine if c.rope == "computed" and c.seq_n == 4096 and not c.use_pos) == 4095, form
    assert {(c.rope, c.use_pos) for c in CASES if c.form == "pp" and c.rope == "by_row"} == {("by_row", False), ("by_row", True)}
    assert all(c.mode == gu.MODE_STORE for c in CASES if c.n_store)
    assert {c.act for c in CASES if c.form == "w16" and c.section in ("M", "N")} == {gu.ACT_GELU_TANH, gu.ACT_GELU_ERF}
    assert gu.GEMM_WALK == dict(M=256 * 300 + 77, N=512, K=128) and gu.GEMM_TAIL == dict(M=136 * 256 - 100, N=512, K=512)


# ------------------------------------------------------------------------------------ mutations
def _mutations(case):
    """-> {name: would-be output fp32 [M][N] before the store rounding} for the mutations that apply to the case's epilogue."""
    o, r = case.ops(), case.refs()
    M, N, K = case.M, case.N, case.K

    def with_ops(**kw):
        s = gu._Ops()
        s.__dict__.update(o.__dict__)
        s.__dict__.update(kw)
        return gu.gemm_eval(case, s, "f32")[0]

    muts = {}
    if case.mode == gu.MODE_QKV_ROPE:
        muts["rope_pos_plus_1"] = with_ops(pos=(o.pos + 1) % case.seq_n)
        flipped = [t.clone() for t in o.tables]
        for t in (flipped[1], flipped[3]):
            t[:, 48:] = -t[:, 48:]
        muts["sin_sign_pairs_24_31"] = with_ops(tables=flipped)
    b2 = o.bias.clone()
    b2[8:12] = 0.0
    muts["bias_group_zeroed"] = with_ops(bias=b2)
    sw = r.f32.clone()
    sw[:, 8:12], sw[:, 12:16] = r.f32[:, 12:16], r.f32[:, 8:12]
    muts["groups_swapped"] = sw
    A2 = o.A.clone()
    A2[M // 2, K - case.BK:] = 0
    muts["row_without_last_k_tile"] = with_ops(A=A2)
    if case.mode == gu.MODE_STORE and case.act == gu.ACT_GELU_TANH:
        muts["gelu_erf_for_tanh"] = gu.gemm_eval(case, o, "f32", act=gu.ACT_GELU_ERF)[0]
    return muts


def _store(case, x):
    return x if case.out_f32 else x.bfloat16().float()


MUT_CASES = [BY_NAME[f"{form}_{epi}"] for form in ("f32_128", "bf16_128", "pp") for epi in ("store", "gelu_tanh", "rope_tables", "gate_store")] \
    + [BY_NAME["bf16_128_store_f32out"], BY_NAME["pp_gate_res"]]


@pytest.mark.parametrize("case", MUT_CASES, ids=_ids(MUT_CASES))
def test_the_parity_bound_rejects_mutations(case):
    """A would-be device output (the fp32 library's result, rounded to bf16 where the form stores bf16) passes; each mutation of it is
    rejected by the per-element bound.  With bf16 output a mutation is REQUIRED to be caught only if it moves some element by more than
    the 2^-8 |ref_e| store term.  One GEMM_MUTATION line each: caught by parity, accepted or not by the old whole-tensor tolerance."""
    r = case.refs()
    old_tol = gu.TOL_F32 if not case.bf16_in else (gu.TOL_BF16 if not case.out_f32 else 2e-3)
    base = _store(case, r.f32)
    assert gu.parity_err(base, r.ref, r.A, r.allow)[0] <= r.bound
    outs = {k: _store(case, v) for k, v in _mutations(case).items()}
    rr, cc = case.M // 3, 21
    step = 2.0 ** (math.floor(math.log2(abs(float(base[rr, cc])))) - 7)        # one bf16 step at that element
    two = base.clone()
    two[rr, cc] += 2 * step
    outs["element_plus_2_bf16_steps"] = two
    unw = base.clone()
    unw[case.M - 1] = case.ops().x0[case.M - 1] if case.mode == gu.MODE_GATE_RES else gu.CONV_FILL      # the residual stream keeps x0
    outs["row_M-1_unwritten"] = unw
    missed = []
    for name, out in outs.items():
        err = gu.parity_err(out, r.ref, r.A, r.allow)[0]
        old = gu.rel_err(out, r.ref)
        moved = (out.double() - base.double()).abs()
        required = case.out_f32 or bool((moved > gu.BF16_STORE * r.ref.abs() * 2).any())       # under one store term each way: the store may hide it
        caught = err > r.bound
        print(f"\nGEMM_MUTATION case={case.name} mutation={name} parity_err/bound={err / r.bound:.3g} caught={caught} required={required} "
              f"old_rel_err={old:.2e} old_tolerance_accepts={old < old_tol}")
        if required and not caught:
            missed.append((name, err, r.bound))
    assert not missed, missed
