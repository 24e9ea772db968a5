"""Helpers of the sampler matrix (tests/test_sampler_matrix_cpu.py, tests/test_sampler_matrix_gpu.py), no GPU needed to import.

``ref_solve_all`` is ONE reference solver for every option of the flow-matching sampler: a plain restatement of DESIGN.md 8 N7 (Runge-Kutta
plans, per-item strength), N8 (guidance interval), N11 (projected guidance), N20 (Adams-Bashforth plans), N21 (guidance reuse) and N23
(block caching) around the oracle, in the oracle's dtype (fp32 or float64).  The CPU file anchors it bit for bit against the six solvers the
option files carry.  ``FACTORS`` is the one table of what a call may combine, ``supported`` the driver's rules restated, ``cases`` a covering
array: every pair of levels the rules admit together occurs in a case.  ``bound`` states the parity bound once; ``mutant`` is the mutation
table's fp32 solver with one thing wrong."""
import math

import numpy as np

FULL, STORE, LIGHT = 0, 1, 2
DEPTH = 4                                     # the four-block tiny model of test_block_cache_gpu.py
MODEL_SEED = 9527
RAGGED = dict(a=[256 * 12, 256 * 14 + 100, 256 * 20], t=[20, 11, 30], g=[18, 17, 24])     # 31, 32 and 45 frames: below, at, above a 32-frame tile
BATCH_SEED = 3
PERM = (2, 0, 1)                              # the permuted batch, with EXTRA more padded frames
EXTRA = 7
ONE = 2                                       # the item of the B = 1 batch (45 frames: two tiles; strength 3.0, k = 3 in the per-item levels)
INTERVAL = (0.05, 0.7)
ITEM_G = (2.0, 0.0, 3.0)
ITEM_K = (1, 2, 3)
ETAS = (0.0, 0.5, 0.25)
CAPS = (None, 0.05, 0.4)
FLOOR = 2.0 ** -23                            # one fp32 rounding of the stored state and one of the comparison
MARGIN = 4.0                                  # the project's margin for a device that sums in another order (gemm_bound, conv_bound, ln_bound)
MATTERS = 100.0                               # an option that is on moves the float64 reference by more than this many bounds


def bound(yardstick):
    return MARGIN * yardstick + FLOOR


def err(x, ref):
    """max |x - ref| / max |ref|, in float64."""
    x, ref = x.double(), ref.double()
    return float((x - ref).abs().max()) / float(ref.abs().max())


# ------------------------------------------------------------------------------------------------ the reference solver
def grid64(nfe_step, sway):
    """The float64 points of the sway-sampled grid, restated."""
    t = np.linspace(0.0, 1.0, nfe_step, dtype=np.float64)
    return t + sway * (np.cos(np.pi / 2 * t) - 1.0 + t)


def mask_column(t, g, interval=None, k=None):
    """N8 / N21 for one item: 0 / 1 / 2 per evaluation from the evaluation times.  Guided where the strength is not 0 and the time lies
    inside the interval, both edges inclusive; the j-th guided evaluation is computed (1) when j % k == 0 and reused (2) otherwise."""
    col, j = [], 0
    for te in t:
        if g == 0.0 or not (interval is None or interval[0] <= float(te) <= interval[1]):
            col.append(0)
            continue
        col.append(1 if (k is None or j % k == 0) else 2)
        j += 1
    return col


def cache_modes(t, every, interval=None):
    """N23: 0 / 1 / 2 per evaluation.  The candidates are the evaluations inside the interval; the j-th candidate is light when every > 1
    and j % every != 0; a full evaluation stores when the next one is light."""
    light, j = [], 0
    for te in t:
        c = interval is None or interval[0] <= float(te) <= interval[1]
        light.append(c and every > 1 and j % every != 0)
        j += int(c)
    return modes_of(light)


def modes_of(light):
    return [LIGHT if l else (STORE if e + 1 < len(light) and light[e + 1] else FULL) for e, l in enumerate(light)]


def _forward(orc, x, cat, ropes, span, mode, cache, key):
    """The DiT at the time orc.t_grid[0] with N23's span rule.  STORE keeps cache[key] = the residual stream at the entry of block span[1]
    (or of the final norm) less the stream at the entry of block span[0]; LIGHT runs the blocks in front of the span, adds cache[key] and
    runs the blocks behind it; FULL is the model as it is."""
    import torch.nn.functional as F
    s, w = orc.spec, orc.w
    d, (a, b) = s.dim, span
    temb = F.silu(orc.time_embed(0))
    h = orc.input_embed(x, cat)
    mark = None
    for i in range(s.depth + 1):
        if mode == LIGHT and a <= i < b:
            if i == a:
                h = h + cache[key]
            continue
        if mode == STORE and i == a:
            mark = h
        if mode == STORE and i == b:
            cache[key] = h - mark
        if i == s.depth:
            break
        p = f"blocks.{i}"
        mod = F.linear(temb, w[p + ".adaln.weight"], w[p + ".adaln.bias"])
        sh_a, sc_a, g_a, sh_m, sc_m, g_m = mod.chunk(6)
        n = F.layer_norm(h, (d,), eps=1e-6) * (1 + sc_a) + sh_a
        h = h + g_a * orc.attention(n, p, ropes)
        m = F.layer_norm(h, (d,), eps=1e-6) * (1 + sc_m) + sh_m
        m = F.gelu(F.linear(m, w[p + ".ff1.weight"], w[p + ".ff1.bias"]), approximate="tanh")
        h = h + g_m * F.linear(m, w[p + ".ff2.weight"], w[p + ".ff2.bias"])
    mod = F.linear(temb, w["final.adaln.weight"], w["final.adaln.bias"])
    sc_f, sh_f = mod.chunk(2)
    h = F.layer_norm(h, (d,), eps=1e-6) * (1 + sc_f) + sh_f
    return F.linear(h, w["final.proj.weight"], w["final.proj.bias"])


def _ab_step(x, t, n, f, k, uniform=False):
    """One Adams-Bashforth step of order k on the float64 grid t: the polynomial through (t_n, f_n), (t_{n-1}, f_{n-1}), ... in Newton form,
    integrated over [t_n, t_{n+1}].  f[-1] = f_n.  uniform (a mutation): the steps behind t_n taken as long as h_n."""
    h = t[n + 1] - t[n]
    x = x + h * f[-1]
    if k >= 2:
        a = h if uniform else t[n] - t[n - 1]
        d1 = (f[-1] - f[-2]) / a
        x = x + (h * h / 2.0) * d1
    if k >= 3:
        b = h if uniform else t[n - 1] - t[n - 2]
        d1_old = (f[-2] - f[-3]) / b
        d2 = (d1 - d1_old) / (a + b)
        x = x + (h ** 3 / 3.0 + a * h * h / 2.0) * d2
    return x


def ref_solve_all(orc, pre, x, plan, *, g, mask_col=None, apg=None, span=None, modes=None, calls=None, mut=()):
    """The reference sampler, one item, in the oracle's dtype.

    plan: a model_spec.OdePlan (N7: the tableau a, b and the evaluation times t_n + c_i h_n; N20, plan.beta set: Adams-Bashforth of order
    len(plan.beta[0]) on the float64 grid, one evaluation per step at the fp32 value of t_n).  g: the item's strength.  mask_col (N8 / N21):
    0 / 1 / 2 per evaluation e = step * s + stage -- 0: the slope is the conditional prediction pc; 1: both predictions, D = pc - pu kept,
    slope pc + D g; 2: pc alone, slope pc + D g with the kept D; None: 1 everywhere.  apg = (eta, cap) (N11): at a computed evaluation,
    d = x_e + (1 - t_e) pc, the sums <D, d>, <d, d>, <D, D> in float64, s = cap / rms where rms = (1 - t_e) sqrt(<D, D> / n) exceeds the
    cap (else 1), slope pc + g s D + g s (eta - 1) <D, d> / <d, d> d.  span, modes (N23): the blocks [span[0], span[1]) are skipped at the
    evaluations whose mode is 2, each CFG branch adds back its own contribution stored at the last evaluation of mode 1.  calls: the
    (step0, n_steps) of the device calls in order, None = one call for the whole plan; a call reads nothing an earlier one left: the
    kept difference, the stored contributions and the kept slopes start empty (under N20 the order at step n of a call is
    min(q, n - step0 + 1)).  mut: names of MUTATIONS, for the mutation table alone."""
    ropes = (pre["rope_cos_q"], pre["rope_sin_q"], pre["rope_cos_k"], pre["rope_sin_k"])
    cat, drop = pre["cat_mel_text"], pre["cat_mel_text_drop"]
    n_steps, s = int(plan.dt.numel()), plan.s
    q = 0 if plan.beta is None else len(plan.beta[0])
    t64 = grid64(n_steps + 1, orc.spec.sway_coef) if q else None
    calls = [(0, n_steps)] if calls is None else list(calls)
    kept, cache, f = [None, None], {}, []

    def slope(e, t_e, xi, t_p):
        orc.t_grid = [t_e]
        if modes is not None:
            pc = _forward(orc, xi, cat, ropes, span, modes[e], cache, "c")
            pu = _forward(orc, xi, drop, ropes, span, modes[e], cache, "u")
            return pc + (pc - pu) * g
        pc = orc.dit_forward(xi, cat, ropes, 0)
        col = 1 if mask_col is None else mask_col[e]
        if col == 0 or g == 0.0:
            return pc
        if col == 2:
            D = kept[1] if ("reuse_older" in mut and kept[1] is not None) else kept[0]
            return pc + D * g
        pu = orc.dit_forward(xi, drop, ropes, 0)
        D = pc - pu
        kept[1], kept[0] = kept[0], D
        if apg is None:
            return pc + D * g
        eta, r = apg
        d = xi + (1.0 - t_p) * pc
        S1, S2, S3 = float((D * d).double().sum()), float((d * d).double().sum()), float((D * D).double().sum())
        rms = (1.0 - t_p) * math.sqrt(S3 / D.numel())
        sc = r / rms if (r is not None and rms > r) else 1.0
        Cc = 0.0 if S2 == 0.0 else g * sc * (eta - 1.0) * S1 / S2
        return pc + (g * sc) * D + Cc * d

    for step0, n in calls:
        kept[0] = kept[1] = None
        cache.clear()
        if "history_kept" not in mut:
            f = []
        for st in range(step0, step0 + n):
            if q:
                f.append(slope(st, float(np.float32(t64[st])), x, float(np.float32(t64[st]))))
                k = min(q, st + 1) if "history_kept" in mut else min(q, st - step0 + 1)
                x = _ab_step(x, t64, st, f, k, uniform="ab_uniform" in mut)
                f = f[-3:]
                continue
            h, ks = float(plan.dt[st]), []
            for i in range(s):
                xi = x
                for j in range(i):
                    if plan.a[i][j] != 0.0:
                        xi = xi + (h * plan.a[i][j]) * ks[j]
                t_e = float(plan.t[st * s + i])
                t_0 = float(plan.t[st * s])
                ks.append(slope(st * s + i, t_0 if "stage_at_tn" in mut else t_e, xi, t_0 if "apg_t_step_start" in mut else t_e))
            for j in range(s):
                if plan.b[j] != 0.0:
                    x = x + (h * plan.b[j]) * ks[j]
    return x


# ------------------------------------------------------------------------------------------------ the table
# plan level -> (ode_method, grid points): 6 ... 12 evaluations each; "ab3short" has fewer steps (2) than ab3 keeps slopes (3)
PLANS = {"euler": ("euler", 8), "midpoint": ("midpoint", 5), "heun2": ("heun2", 5), "heun3": ("heun3", 3), "rk4": ("rk4", 3),
         "ab2": ("ab2", 8), "ab3": ("ab3", 8), "ab3short": ("ab3", 3)}
# guidance form -> the options it turns on
FORMS = {"none": {}, "interval": dict(interval=INTERVAL), "reuse2": dict(reuse=2), "reuse123iv": dict(reuse=ITEM_K, interval=INTERVAL),
         "apg": dict(apg=True), "apgiv": dict(apg=True, interval=INTERVAL), "cache13x2": dict(cache=(1, 3, 2)),
         "cache04x3iv": dict(cache=(0, 4, 3), cache_interval=INTERVAL)}
FACTORS = {
    "plan": tuple(PLANS),
    "strength": ("model", "item"),             # the model's scalar | per item ITEM_G
    "form": tuple(FORMS),
    "lanes": (1, 2),
    "call": ("whole", "split"),
    "lengths": ("host", "readback"),
    "ws": ("own", "caller"),                   # the context's workspace | a caller-owned block of exactly the bytes the size query names
    "reports": ("off", "on"),                  # the step report (N20, multistep plans), the drift report (N21), the block-cache report (N23)
    "batch": ("ragged", "permuted", "one"),
}
MULTISTEP = ("ab2", "ab3", "ab3short")
# The driver's rules between two levels, each with the line it restates (csrc/vv_api.hip, transformer_steps and the struct entries; at the
# commit that added this table lines 1722, 1741, 1776 and 1829 / 1904 / 1924 -- the quoted message finds the line when they have moved).
RULES = (
    (("plan", MULTISTEP), ("call", ("split",)),
     "vv_api.hip transformer_steps: 'under a multistep plan a call starts at step 0 (the kept slopes live for one call)'", "multistep plan"),
    (("form", ("reuse2", "reuse123iv")), ("call", ("split",)),
     "vv_api.hip transformer_steps: 'vv_transformer_steps_reuse: a call that reuses starts at step 0 (the stored differences live for one call)'", "reuses starts at step 0"),
    (("form", ("cache13x2", "cache04x3iv")), ("call", ("split",)),
     "vv_api.hip transformer_steps: 'vv_transformer_steps_cached: a call with a light evaluation starts at step 0'", "light evaluation starts at step 0"),
    (("lengths", ("readback",)), ("ws", ("caller",)),
     "vv_api.hip steps_struct_call / vv_transformer_steps_reuse / _cached: 'a workspace block needs the host lengths'", "needs the host lengths"),
)
# What the routing refuses of the raw options, whatever the table: (options, the line it restates, a word of the message).  The table's forms
# never combine these (a form is one level), so they are no pairs of levels; the device file asserts them beside the pairs.
OPTION_RULES = (
    (dict(cache=(1, 3, 2), interval=INTERVAL), "runtime.py transformer_steps_ex: 'block caching takes no guidance mask and no projected guidance'", "block caching takes no"),
    (dict(cache=(1, 3, 2), apg=True), "runtime.py transformer_steps_ex: 'block caching takes no guidance mask and no projected guidance'", "block caching takes no"),
    (dict(reuse=2, apg=True), "runtime.py transformer_steps_ex: 'a mask that reuses guidance differences (a 2) is not combined with projected guidance (apg)'", "not combined with projected"),
)


def supported(levels):
    """levels: factor -> level, any subset of FACTORS.  -> (True, None), or (False, the rule) for the first rule of RULES two of them break."""
    for (fa, la), (fb, lb), where, word in RULES:
        if levels.get(fa) in la and levels.get(fb) in lb:
            return False, (where, word)
    return True, None


def pairs(admitted=True):
    """Every pair of levels of two factors that ``supported`` admits (or rejects), as ((factor, level), (factor, level)) in table order."""
    names = list(FACTORS)
    out = []
    for i, fa in enumerate(names):
        for fb in names[i + 1:]:
            for la in FACTORS[fa]:
                for lb in FACTORS[fb]:
                    if supported({fa: la, fb: lb})[0] == admitted:
                        out.append(((fa, la), (fb, lb)))
    return out


def _covers(case, pair):
    return all(case[f] == l for f, l in pair)


def cases():
    """The covering array, greedy and deterministic: a case starts from the first pair not yet covered and takes, factor by factor in table
    order, the level that covers most of the pairs still open (the first one on a tie) among those the rules admit with what is set."""
    todo = pairs()
    out = []
    while todo:
        case = dict(todo[0])
        for f in FACTORS:
            if f in case:
                continue
            best, best_n = None, -1
            for l in FACTORS[f]:
                trial = dict(case, **{f: l})
                if not supported(trial)[0] or not _extendable(trial):
                    continue
                n = sum(1 for p in todo if all(trial.get(pf, None) == pl for pf, pl in p))
                if n > best_n:
                    best, best_n = l, n
            case[f] = best
        out.append({f: case[f] for f in FACTORS})
        todo = [p for p in todo if not _covers(case, p)]
    return out


def _extendable(partial):
    """Every factor not yet set has a level the rules admit with the partial case (the rules are between pairs, so this is enough)."""
    return all(f in partial or any(supported(dict(partial, **{f: l}))[0] for l in FACTORS[f]) for f in FACTORS)


def case_id(case):
    return "-".join(str(case[f]) for f in FACTORS)


def items_of(case):
    """The items of the ragged three a case runs, in the batch's order."""
    return {"ragged": (0, 1, 2), "permuted": PERM, "one": (ONE,)}[case["batch"]]


def item_options(case, b, spec):
    """What item b (its index in the ragged three) runs with under a case: dict(g, interval, k, apg, cache, cache_interval)."""
    o = FORMS[case["form"]]
    reuse = o.get("reuse")
    return dict(g=float(spec.cfg_strength) if case["strength"] == "model" else ITEM_G[b], interval=o.get("interval"),
                k=None if reuse is None else (reuse if isinstance(reuse, int) else reuse[b]),
                apg=(ETAS[b], CAPS[b]) if o.get("apg") else None, cache=o.get("cache"), cache_interval=o.get("cache_interval"))


def split_of(case, n_steps):
    """The (step0, n_steps) of a case's calls."""
    if case["call"] == "whole":
        return [(0, n_steps)]
    first = max(1, n_steps // 2)
    return [(0, first), (first, n_steps - first)]


def solver_args(opt, plan, calls=None):
    """The keyword arguments of ref_solve_all for one item's options on a plan."""
    t = [float(v) for v in plan.t]
    kw = dict(g=opt["g"], calls=calls)
    if opt["cache"] is not None:
        kw.update(span=opt["cache"][:2], modes=cache_modes(t, opt["cache"][2], opt["cache_interval"]))
        return kw
    if opt["interval"] is not None or opt["k"] is not None or opt["g"] == 0.0:
        kw["mask_col"] = mask_column(t, opt["g"], opt["interval"], opt["k"])
    kw["apg"] = opt["apg"]
    return kw


def removals(opt, plan):
    """-> [(option, the item's options with it removed, or None with the reason it touches nothing by construction)]."""
    t = [float(v) for v in plan.t]
    out = []
    guided = opt["g"] != 0.0

    def without(**kw):
        return dict(opt, **kw)
    if opt["interval"] is not None:
        out.append(("interval", without(interval=None) if guided else None, "strength 0: the item is never guided"))
    if opt["k"] is not None:
        col = mask_column(t, opt["g"], opt["interval"], opt["k"])
        why = "strength 0: the item is never guided" if not guided else "k = 1: every guided evaluation is computed" if opt["k"] == 1 else \
            "no reused evaluation on this plan" if 2 not in col else None
        out.append(("reuse", None if why else without(k=None), why))
    if opt["apg"] is not None:
        col = mask_column(t, opt["g"], opt["interval"], None)
        why = "strength 0: the item is never guided" if not guided else "no guided evaluation on this plan" if 1 not in col else None
        out.append(("apg", None if why else without(apg=None), why))
    if opt["cache"] is not None:
        m = cache_modes(t, opt["cache"][2], opt["cache_interval"])
        out.append(("cache", without(cache=None, cache_interval=None) if LIGHT in m else None, "no light evaluation on this plan: every evaluation is full"))
        if opt["cache_interval"] is not None:
            same = m == cache_modes(t, opt["cache"][2], None)
            out.append(("cache_interval", None if same or LIGHT not in m else without(cache_interval=None), "the schedule is the same without the interval"))
    return out


# ------------------------------------------------------------------------------------------------ the references, computed once
_STATE = {}
_REFS = {}


def setup():
    """-> (spec, weights, batch, {dtype name: Oracle}, {(dtype name, item): the oracle's preprocess}): the four-block tiny model, the ragged
    three of test_block_cache_gpu.py, one fp32 and one float64 oracle.  Built once per process."""
    if not _STATE:
        import dataclasses

        import torch
        from oracle.vv_oracle import Oracle
        from tests.test_e2e_gpu import make_batch
        from vietvoice_tts_amd.model_spec import ModelSpec, make_synthetic_weights
        spec = dataclasses.replace(ModelSpec.tiny(), depth=DEPTH)
        w = make_synthetic_weights(spec, seed=MODEL_SEED)
        batch = make_batch(spec, RAGGED["a"], RAGGED["t"], RAGGED["g"], seed=BATCH_SEED)
        assert [int(v) for v in batch["seq_len"]] == [31, 32, 45]
        orcs = {"f32": Oracle(spec, w, nfe_step=8), "f64": Oracle(spec, w, nfe_step=8, dtype=torch.float64)}
        pres = {}
        for name, orc in orcs.items():
            for b in range(3):
                la, lt, sl = int(batch["audio_len"][b]), int(batch["text_len"][b]), int(batch["seq_len"][b])
                pres[name, b] = orc.preprocess(batch["audio"][b, :la], batch["ids"][b, :lt], sl, batch["noise"][b, :sl])
        _STATE.update(spec=spec, w=w, batch=batch, orcs=orcs, pres=pres)
    return _STATE["spec"], _STATE["w"], _STATE["batch"], _STATE["orcs"], _STATE["pres"]


def plan_of(level):
    from vietvoice_tts_amd.model_spec import ode_plan
    spec = setup()[0]
    key = ("plan", level)
    if key not in _REFS:
        _REFS[key] = ode_plan(PLANS[level][1], spec.sway_coef, PLANS[level][0])
    return _REFS[key]


def _freeze(v):
    return tuple(sorted((k, _freeze(x)) for k, x in v.items())) if isinstance(v, dict) else tuple(_freeze(x) for x in v) if isinstance(v, (list, tuple)) else v


def reference(dtype, plan_level, b, opt, mut=(), calls=None):
    """ref_solve_all for item b with the options ``opt`` on a plan level, in the fp32 or the float64 oracle; computed once and shared.  The
    tests leave ``calls`` at None for a case that splits: the table admits a split only where nothing is kept between the evaluations of
    different steps, and there a split is the same arithmetic (test_a_split_of_a_stateless_form_is_the_same_arithmetic)."""
    _, _, _, orcs, pres = setup()
    key = (dtype, plan_level, b, _freeze(opt), tuple(mut), None if calls is None else tuple(calls))
    if key not in _REFS:
        plan = plan_of(plan_level)
        pre = pres[dtype, b]
        _REFS[key] = ref_solve_all(orcs[dtype], pre, pre["noise"], plan, mut=mut, **solver_args(opt, plan, calls))
    return _REFS[key]


def parity_refs(plan_level, b, opt):
    """-> (ref64, yardstick, bound) of one item: the float64 reference, the fp32 solver's distance from it, and the parity bound."""
    r64 = reference("f64", plan_level, b, opt)
    y = err(reference("f32", plan_level, b, opt), r64)
    return r64, y, bound(y)


# ------------------------------------------------------------------------------------------------ the mutation table
# strength_1e-4: strength x (1 + 1e-4); neighbour_strength: the next item's strength; reuse_older: a reuse load takes the difference stored one
# guided evaluation earlier; cache_shift: the block-cache schedule one evaluation late; ab_uniform: uniform-grid Adams-Bashforth
# coefficients on the sway grid; history_kept: multistep slopes kept across a split; interval_exclusive: the interval's edges exclusive at
# a grid point; stage_at_tn: a Runge-Kutta stage evaluated at t_n; apg_t_step_start: APG's 1 - t taken from the step's start inside a stage
MUTATIONS = ("strength_1e-4", "neighbour_strength", "reuse_older", "cache_shift", "ab_uniform", "history_kept", "interval_exclusive",
             "stage_at_tn", "apg_t_step_start")


def mutant(name, plan_level, b, opt, case):
    """-> (the mutant's fp32 state, None) or (None, the reason the mutation does not apply to this item of this case)."""
    spec = setup()[0]
    plan = plan_of(plan_level)
    t = [float(v) for v in plan.t]
    guided = opt["g"] != 0.0 and 0 != max(mask_column(t, opt["g"], opt["interval"], None))
    multistep = plan.beta is not None
    if name == "strength_1e-4":
        if not guided:
            return None, "the item is never guided: its strength is not read"
        return reference("f32", plan_level, b, dict(opt, g=opt["g"] * (1.0 + 1e-4))), None
    if name == "neighbour_strength":
        items = items_of(case)
        if len(items) < 2:
            return None, "B = 1: no neighbour"
        nb = items[(items.index(b) + 1) % len(items)]
        g2 = item_options(case, nb, spec)["g"]
        if g2 == opt["g"]:
            return None, "the neighbour has the same strength"
        if opt["cache"] is None and 0 == max(mask_column(t, 1.0, opt["interval"], None)):
            return None, "no guided evaluation on this plan"
        return reference("f32", plan_level, b, dict(opt, g=g2)), None
    if name == "reuse_older":
        col = mask_column(t, opt["g"], opt["interval"], opt["k"]) if opt["k"] else []
        seen = 0
        hit = False
        for v in col:
            seen += v == 1
            hit = hit or (v == 2 and seen >= 2)
        if not hit:
            return None, "no reused evaluation with two computed ones before it"
        return reference("f32", plan_level, b, opt, mut=("reuse_older",)), None
    if name == "cache_shift":
        if opt["cache"] is None:
            return None, "no block cache"
        m = cache_modes(t, opt["cache"][2], opt["cache_interval"])
        light = [False] + [v == LIGHT for v in m[:-1]]
        shifted = modes_of(light)
        if shifted == m or LIGHT not in m:
            return None, "no light evaluation to shift"
        _, _, _, orcs, pres = setup()
        key = ("f32", plan_level, b, _freeze(opt), "cache_shift")
        if key not in _REFS:
            pre = pres["f32", b]
            _REFS[key] = ref_solve_all(orcs["f32"], pre, pre["noise"], plan, g=opt["g"], span=opt["cache"][:2], modes=shifted)
        return _REFS[key], None
    if name == "ab_uniform":
        if not multistep:
            return None, "no multistep plan"
        return reference("f32", plan_level, b, opt, mut=("ab_uniform",)), None
    if name == "history_kept":
        return None, "the driver refuses step0 > 0 under a multistep plan: no case splits one (the refusal is asserted on the device)"
    if name == "interval_exclusive":
        # the case's interval snapped to the first and last evaluation time inside it builds the same mask under the inclusive rule; an
        # exclusive comparison drops those two evaluations
        iv = opt["interval"] if opt["cache"] is None else opt["cache_interval"]
        if iv is None:
            return None, "no interval"
        inside = [te for te in t if iv[0] <= te <= iv[1]]
        if not inside:
            return None, "no evaluation inside the interval"
        snapped = (np.nextafter(inside[0], 2.0), np.nextafter(inside[-1], -1.0))      # the open interval between the two grid points, as a closed one
        if opt["cache"] is None:
            if not guided:
                return None, "the item is never guided"
            return reference("f32", plan_level, b, dict(opt, interval=(float(snapped[0]), float(snapped[1])))), None
        o2 = dict(opt, cache_interval=(float(snapped[0]), float(snapped[1])))
        if cache_modes(t, opt["cache"][2], o2["cache_interval"]) == cache_modes(t, opt["cache"][2], iv):
            return None, "the schedule is the same"
        return reference("f32", plan_level, b, o2), None
    if name == "stage_at_tn":
        if plan.s == 1:
            return None, "one evaluation per step"
        return reference("f32", plan_level, b, opt, mut=("stage_at_tn",)), None
    if name == "apg_t_step_start":
        if opt["apg"] is None or not guided or plan.s == 1:
            return None, "no projected guidance inside a stage"
        return reference("f32", plan_level, b, opt, mut=("apg_t_step_start",)), None
    raise KeyError(name)
