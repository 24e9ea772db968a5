"""The sampler matrix without a device (tests/sampler_util.py): the one reference solver anchored bit for bit against the six solvers of the
option files on their own cases; the covering array of the factor table; every option that is on moves the float64 reference by more than
100 bounds, for every case and item; and the mutation table: each mutation of the fp32 solver misses the parity bound of
tests/test_sampler_matrix_gpu.py (4 x the fp32 solver's own distance from float64 + 2^-23) on every case it applies to."""
import numpy as np
import pytest
import torch

from tests import sampler_util as S

OLD_TOL = 1e-3        # the bound of the option files, for the table's last column


@pytest.fixture(scope="module")
def env():
    return S.setup()


def _plan(spec, method, nfe):
    from vietvoice_tts_amd.model_spec import ode_plan
    return ode_plan(nfe, spec.sway_coef, method)


def _mine(orc, pre, plan, **kw):
    return S.ref_solve_all(orc, pre, pre["noise"], plan, **kw)


# ------------------------------------------------------------------------------------------------ 1. the anchors, bit for bit
def test_anchor_ref_solve(env):
    """tests/test_ode_gpu.py: the four Runge-Kutta parametrisations and Euler with the model's strength, midpoint with a strength per item."""
    from tests.test_ode_gpu import ref_solve
    spec, _, _, orcs, pres = env
    orc, g = orcs["f32"], float(spec.cfg_strength)
    for name, nfe in (("euler", 8), ("midpoint", 5), ("heun2", 5), ("heun3", 3), ("rk4", 3)):
        pre = pres["f32", 0]
        assert torch.equal(_mine(orc, pre, _plan(spec, name, nfe), g=g), ref_solve(orc, pre, pre["noise"], name, nfe, g)), (name, nfe)
    for b, gb in enumerate([2.0, 1.0, 3.5]):
        pre = pres["f32", b]
        assert torch.equal(_mine(orc, pre, _plan(spec, "midpoint", 5), g=gb), ref_solve(orc, pre, pre["noise"], "midpoint", 5, gb)), b


def test_anchor_ref_solve_guided(env):
    """tests/test_guidance_gpu.py: the Euler window (evaluations 2 ... 4 of 7) and the windows inside a midpoint and an rk4 step."""
    from tests.test_guidance_gpu import WINDOW, _window_mask, ref_solve_guided
    spec, _, _, orcs, pres = env
    orc, g, pre = orcs["f32"], float(spec.cfg_strength), pres["f32", 0]
    todo = [("euler", 8, 2, 4)] + [(name, *WINDOW[name]) for name in ("midpoint", "rk4")]
    for name, nfe, e_lo, e_hi in todo:
        plan = _plan(spec, name, nfe)
        col = [int(v) for v in _window_mask(plan.t.numel(), 1, e_lo, e_hi)[:, 0]]
        assert torch.equal(_mine(orc, pre, plan, g=g, mask_col=col), ref_solve_guided(orc, pre, pre["noise"], name, nfe, g, col)), name


def test_anchor_ref_solve_apg(env):
    """tests/test_apg_gpu.py: euler and rk4 on 5 points, eta and cap per item, in float64 -- the dtype that solver runs in there.  In fp32
    the two differ by design: ref_solve_apg sums <D, d>, <d, d>, <D, D> in the oracle's dtype, ref_solve_all in float64 as DESIGN N11 and
    multistep_util.ref_multistep do (the fp32 anchor of the projected term is test_anchor_ref_multistep's apg case)."""
    from tests.test_apg_gpu import CAPS, ETAS, ref_solve_apg
    spec, _, _, orcs, pres = env
    orc, g = orcs["f64"], float(spec.cfg_strength)
    for name in ("euler", "rk4"):
        plan = _plan(spec, name, 5)
        for b in range(3):
            pre = pres["f64", b]
            want, _ = ref_solve_apg(orc, pre, pre["noise"], name, 5, g, ETAS[b], CAPS[b])
            assert torch.equal(_mine(orc, pre, plan, g=g, apg=(ETAS[b], CAPS[b])), want), (name, b)
    plan, pre = _plan(spec, "euler", 5), pres["f64", 0]
    col = [0, 1, 1, 0]
    want, _ = ref_solve_apg(orc, pre, pre["noise"], "euler", 5, g, 0.0, 0.05, guided=col)
    assert torch.equal(_mine(orc, pre, plan, g=g, apg=(0.0, 0.05), mask_col=col), want)


def test_anchor_ref_multistep(env):
    """tests/test_multistep_gpu.py: ab2 and ab3 on 2, 3, 5 and 9 points; on 9 points an interval, a strength of 0 and projected guidance."""
    from tests.multistep_util import ref_multistep
    spec, _, _, orcs, pres = env
    orc, g, pre = orcs["f32"], float(spec.cfg_strength), pres["f32", 0]
    for name, q in (("ab2", 2), ("ab3", 3)):
        for nfe in (2, 3, 5, 9):
            assert torch.equal(_mine(orc, pre, _plan(spec, name, nfe), g=g), ref_multistep(orc, pre, pre["noise"], q, nfe, g)), (name, nfe)
        plan = _plan(spec, name, 9)
        flags = [False] * 3 + [True] * 3 + [False] * 2
        assert S.mask_column([float(v) for v in plan.t], g, (0.1, 0.6)) == [int(v) for v in flags]
        assert torch.equal(_mine(orc, pre, plan, g=g, mask_col=[int(v) for v in flags]), ref_multistep(orc, pre, pre["noise"], q, 9, g, guided=flags))
        assert torch.equal(_mine(orc, pre, plan, g=0.0), ref_multistep(orc, pre, pre["noise"], q, 9, 0.0))
        assert torch.equal(_mine(orc, pre, plan, g=g, apg=(0.0, None)), ref_multistep(orc, pre, pre["noise"], q, 9, g, apg=(0.0, None)))


def test_anchor_ref_solve_reuse(env):
    """tests/test_cfg_reuse_gpu.py: its CASES, every item."""
    from tests.cfg_reuse_util import ref_solve_reuse
    from tests.test_cfg_reuse_gpu import CASES
    from vietvoice_tts_amd.model_spec import guidance_mask
    spec, _, _, orcs, pres = env
    orc = orcs["f32"]
    for case, (method, nfe, reuse, interval, gs) in CASES.items():
        gs = [float(spec.cfg_strength)] * 3 if gs is None else list(gs)
        plan = _plan(spec, method, nfe)
        mask = guidance_mask(plan, interval, gs, reuse)
        for b in range(3):
            pre = pres["f32", b]
            col = [int(v) for v in mask[:, b]]
            k = reuse if isinstance(reuse, int) else reuse[b]
            assert col == S.mask_column([float(v) for v in plan.t], gs[b], interval, k), (case, b)
            assert torch.equal(_mine(orc, pre, plan, g=gs[b], mask_col=col), ref_solve_reuse(orc, pre, pre["noise"], method, nfe, gs[b], col)), (case, b)


def test_anchor_ref_solve_cached(env):
    """tests/test_block_cache_gpu.py: its CASES; item 0, and every item where the strengths differ."""
    from tests.block_cache_util import ref_solve_cached, schedule
    from tests.test_block_cache_gpu import CASES
    spec, _, _, orcs, pres = env
    orc = orcs["f32"]
    for case, (method, nfe, span, every, interval, gs) in CASES.items():
        items = (0,) if gs is None else (0, 1, 2)
        gs = [float(spec.cfg_strength)] * 3 if gs is None else list(gs)
        plan = _plan(spec, method, nfe)
        t = [float(v) for v in plan.t]
        modes = S.cache_modes(t, every, interval)
        assert modes == schedule(t, every, interval), case
        for b in items:
            pre = pres["f32", b]
            assert torch.equal(_mine(orc, pre, plan, g=gs[b], span=span, modes=modes), ref_solve_cached(orc, pre, pre["noise"], method, nfe, gs[b], span, modes)), (case, b)


def test_a_split_of_a_stateless_form_is_the_same_arithmetic(env):
    """What sampler_util.reference relies on when it leaves the calls out of its key; and what a split does to a stateful form."""
    spec, _, _, orcs, pres = env
    orc, g, pre = orcs["f32"], float(spec.cfg_strength), pres["f32", 0]
    plan = _plan(spec, "heun3", 3)
    col = S.mask_column([float(v) for v in plan.t], g, S.INTERVAL)
    whole = _mine(orc, pre, plan, g=g, mask_col=col, apg=(0.0, 0.05))
    assert torch.equal(_mine(orc, pre, plan, g=g, mask_col=col, apg=(0.0, 0.05), calls=[(0, 1), (1, 1)]), whole)
    ab = _plan(spec, "ab3", 5)
    assert not torch.equal(_mine(orc, pre, ab, g=g, calls=[(0, 2), (2, 2)]), _mine(orc, pre, ab, g=g))       # the kept slopes live for one call
    assert torch.equal(_mine(orc, pre, ab, g=g, calls=[(0, 2), (2, 2)], mut=("history_kept",)), _mine(orc, pre, ab, g=g))


# ------------------------------------------------------------------------------------------------ 2. the table
def test_the_cases_cover_every_supported_pair_and_nothing_else():
    cs = S.cases()
    ok, no = S.pairs(True), S.pairs(False)
    print(f"SAMPLER_TABLE cases {len(cs)} supported pairs {len(ok)} refused pairs {len(no)}")
    for fa, fb in no:
        print(f"  refused: {fa[0]}={fa[1]} with {fb[0]}={fb[1]}: {S.supported(dict([fa, fb]))[1][0]}")
    assert len(cs) <= 120
    assert len({S.case_id(c) for c in cs}) == len(cs)
    for c in cs:
        assert set(c) == set(S.FACTORS) and all(c[f] in S.FACTORS[f] for f in S.FACTORS)
        assert S.supported(c)[0], c
    missing = [p for p in ok if not any(all(c[f] == l for f, l in p) for c in cs)]
    assert not missing, missing[:5]
    assert len(ok) + len(no) == sum(len(S.FACTORS[a]) * len(S.FACTORS[b]) for i, a in enumerate(S.FACTORS) for b in list(S.FACTORS)[i + 1:])
    assert S.cases() == cs                                                   # deterministic
    # every level of every factor the issue names is there
    assert len(S.FACTORS["plan"]) == 8 and len(S.FACTORS["form"]) == 8 and len(S.FACTORS) == 9
    for level, (method, nfe) in S.PLANS.items():
        n = S.plan_of(level).t.numel()
        assert 6 <= n <= 12 or level == "ab3short", (level, n)
    assert S.plan_of("ab3short").dt.numel() < len(S.plan_of("ab3short").beta[0])


def test_the_restated_masks_and_schedules_are_the_products(env):
    """mask_column / cache_modes (the reference side) against model_spec.guidance_mask / block_cache_schedule (what the device is handed),
    for every case."""
    from vietvoice_tts_amd.model_spec import block_cache_schedule, guidance_mask
    spec = env[0]
    for c in S.cases():
        plan = S.plan_of(c["plan"])
        t = [float(v) for v in plan.t]
        items = S.items_of(c)
        opts = [S.item_options(c, b, spec) for b in items]
        o = S.FORMS[c["form"]]
        if "cache" in o:
            assert block_cache_schedule(plan, o["cache"][2], o.get("cache_interval")).tolist() == S.cache_modes(t, o["cache"][2], o.get("cache_interval"))
            continue
        reuse = o.get("reuse")
        ks = None if reuse is None else [p["k"] for p in opts]
        mask = guidance_mask(plan, o.get("interval"), [p["g"] for p in opts], ks)
        for i, p in enumerate(opts):
            col = S.mask_column(t, p["g"], p["interval"], p["k"])
            assert col == ([1] * len(t) if mask is None else [int(v) for v in mask[:, i]]), (S.case_id(c), i)


# ------------------------------------------------------------------------------------------------ 3. every option matters where it is on
@pytest.mark.parametrize("form", [f for f in S.FORMS if f != "none"])
def test_every_option_matters_where_it_is_on(env, form):
    """For each case, item and option that is on: the float64 reference without the option lies more than 100 bounds from the one with it.
    Only an item the option does not touch by construction is exempt, with the reason printed."""
    spec = env[0]
    seen, exempt, lowest = set(), 0, None
    for c in S.cases():
        if c["form"] != form:
            continue
        for b in S.items_of(c):
            opt = S.item_options(c, b, spec)
            key = (c["plan"], b, S._freeze(opt))
            if key in seen:
                continue
            seen.add(key)
            r64, y, bd = S.parity_refs(c["plan"], b, opt)
            for name, without, why in S.removals(opt, S.plan_of(c["plan"])):
                if without is None:
                    exempt += 1
                    print(f"SAMPLER_MATTERS {c['plan']} {c['strength']} {form} item {b} {name}: exempt -- {why}")
                    continue
                apart = S.err(S.reference("f64", c["plan"], b, without), r64)
                lowest = apart / bd if lowest is None else min(lowest, apart / bd)
                print(f"SAMPLER_MATTERS {c['plan']} {c['strength']} {form} item {b} {name}: apart {apart:.3e} bound {bd:.3e} ratio {apart / bd:.0f}")
                assert apart > S.MATTERS * bd, (S.case_id(c), b, name, apart, bd)
    print(f"SAMPLER_MATTERS {form}: {len(seen)} (plan, item, options) of the cases, {exempt} exempt, lowest ratio {lowest}")
    assert seen and lowest is not None


# ------------------------------------------------------------------------------------------------ 4. the mutation table
@pytest.mark.parametrize("name", S.MUTATIONS)
def test_the_bound_rejects_the_mutation(env, name):
    """The mutation applied to the fp32 solver, against the float64 reference: its error must exceed the bound on every (case, item) it
    applies to.  Where it does not apply the reason is counted and printed.  The last figure: on how many of them 1e-3 accepts it."""
    spec = env[0]
    seen, skipped, applied, old_accepts, lowest = set(), {}, 0, 0, None
    for c in S.cases():
        for b in S.items_of(c):
            opt = S.item_options(c, b, spec)
            x, why = S.mutant(name, c["plan"], b, opt, c)
            key = (c["plan"], b, S._freeze(opt), None if x is None else x.data_ptr())
            if key in seen:
                continue
            seen.add(key)
            if x is None:
                skipped[why] = skipped.get(why, 0) + 1
                continue
            r64, y, bd = S.parity_refs(c["plan"], b, opt)
            e = S.err(x, r64)
            applied += 1
            old_accepts += e < OLD_TOL
            lowest = e / bd if lowest is None else min(lowest, e / bd)
            assert e > bd, (name, S.case_id(c), b, e, bd)
    for why, n in skipped.items():
        print(f"SAMPLER_MUTATION {name}: skipped {n} -- {why}")
    print(f"SAMPLER_MUTATION {name}: rejected on {applied} of {applied} (case, item) it applies to, lowest err / bound "
          f"{'-' if lowest is None else format(lowest, '.1f')}; 1e-3 accepts it on {old_accepts}")
    assert applied or name == "history_kept"
