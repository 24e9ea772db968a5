"""-m gpu: CFG-Zero* / guidance rescale / zero-init (tests/cfg_norm_util.py holds the rule, the mirror, the bound and the
reference solver).

  kernel entries   vv_cfg_norm_coef on items of 1, 31, 32, 33, 97 and 0 frames in one launch: the partial sums equal the numpy mirror bit for
                   bit, (s, f) lies within the bound derived from the summation error, an item's coefficients are the same bits alone and at
                   another place of the batch.  The reduction reads no row map (its rows are the packed ones); the permuted order is that of
                   row_start, and the permuted row_src is the stage kernel's.
  stage kernel     vv_ode_stage_norm over step_util's (n_mel, ldp) pairs and 1, 3 and 86 rows against float64 under the counted fp32 bound;
                   with coef = {1, 1} the bits of vv_ode_stage_guided.
  device           the ragged three (31, 32, 45 frames; strengths 2, 0, 3) against ref_solve_norm on the float64 oracle within
                   sampler_util.bound(yardstick), the yardstick being the same solver on the fp32 oracle.  That the rule moves the reference
                   by more than MATTERS bounds is asserted in tests/test_cfg_norm_cpu.py.
  invariances      bit for bit: an item alone, in the batch, permuted with more padding, on branch lanes (B = 1), split by step0, captured
  the rest         off means off, the report, the refusals, the profiler's class and counts, the engine paths and the front end."""
import ctypes as C

import numpy as np
import pytest
import torch

from tests import cfg_norm_util as U
from tests import sampler_util as S
from tests import step_util as T
from tests.gpu_util import DEV, EPS24, NAN, _bands_intact, _guarded, check, parity_err, stream
from vietvoice_tts_amd import runtime as rt

pytestmark = pytest.mark.gpu

FILL = T.FILL
I32 = torch.int32


# ------------------------------------------------------------------------------------------------ the rig
@pytest.fixture(scope="module")
def rig():
    """sampler_util's four-block model on engines of this module's own (fp32 and bf16), and its three batches on the device."""
    from tests.test_sampler_matrix_gpu import _moved, _one
    spec, w, batch, _, _ = S.setup()
    engs = {"f32": rt.HipSynth(spec, w, acoustic_dtype="fp32", nfe_step=8), "bf16": rt.HipSynth(spec, w, acoustic_dtype="bf16", nfe_step=8)}
    d = {k: (v.to(DEV) if torch.is_tensor(v) else v) for k, v in batch.items()}
    d["lens"] = [int(v) for v in batch["seq_len"]]
    data = {"ragged": d, "permuted": _moved(d, list(S.PERM), S.EXTRA)}
    for b in range(3):
        data["alone", b] = _one(spec, d, batch, b)
    yield spec, engs, data
    for e in engs.values():
        e.close()


def _pre(eng, d, host=True):
    return eng.preprocess(d["audio"], d["audio_len"], d["ids"], d["text_len"], d["seq_len"], d["N"], seq_len_host=d["lens"] if host else None)


def _host(d):
    return (C.c_int32 * len(d["lens"]))(*d["lens"])


def _norm(eng, per_item):
    return eng.cfg_norm_tensors([p[0] for p in per_item], [p[1] for p in per_item])


def _run(eng, d, pre, g, per_item, interval=None, calls=None, ws=None, x=None):
    """One synthesis of the batch ``d`` through transformer_steps_ex, arguments built as production builds them."""
    x = d["noise"].clone() if x is None else x
    cfg = torch.tensor(list(g), dtype=torch.float32, device=DEV)
    guide = eng.guidance_mask(interval, list(g))
    for step0, n in (calls or [(0, eng.n_steps)]):
        eng.transformer_steps_ex(x, pre, step0, n, _host(d), cfg, ws=ws, guide=guide, cfg_norm=_norm(eng, per_item))
    torch.cuda.synchronize()
    return x


class _Plan:
    """The plan in force for the duration of a test; the engine goes back to Euler on 8 points."""

    def __init__(self, eng, level, skip=0, lanes=0):
        self.eng, self.level, self.skip, self.lanes = eng, level, skip, lanes

    def __enter__(self):
        method, nfe = U.NORM_PLANS[self.level]
        self.eng.set_nfe(nfe, method, self.skip)
        self.eng.set_option("lanes", self.lanes)
        return self.eng

    def __exit__(self, *exc):
        self.eng.set_cfg_norm_report(False)
        self.eng.set_option("lanes", 0)
        self.eng.set_nfe(8, "euler")
        return False


# ------------------------------------------------------------------------------------------------ 1. the kernel entries
LENS, GUIDED, ORDER, G_ITEM, STAR, RESC = U.LENS, U.GUIDED, U.ORDER, U.G_ITEM, U.STAR, U.RESC
_coef_ops = U.coef_ops


def _coef_launch(eng, o, n_tiles, g_item=G_ITEM, star=STAR, resc=RESC, want_report=True, items=None):
    """vv_cfg_norm_coef on the operands ``o`` (or on the items ``items`` of them as a launch of their own, the tables cut to them)."""
    ids = list(range(o["B"])) if items is None else list(items)
    B = len(ids)
    pw, dp = T.framed(o["pred"])
    keep = [T.table(torch.tensor([o["start"][b] for b in ids]), 0), T.table(torch.tensor([o["lens"][b] for b in ids]), 0),
            T.table(o["u_row"], o["pred"].shape[0])]
    fl = [T.framed(torch.tensor([v[b] for b in ids], dtype=torch.float32), 0, 4)[1] for v in (g_item, star, resc)]
    parts_w, parts = _guarded((B, n_tiles, 5), 10, FILL, init=torch.full((B, n_tiles, 5), FILL, dtype=torch.float64), dtype=torch.float64)
    coef_w, coef = _guarded((B, 2), 4, FILL, init=torch.full((B, 2), FILL))
    rep_w, rep = _guarded((B, 2), 4, FILL, init=torch.full((B, 2), FILL))
    a = rt.vv_cfg_norm_coef_args()
    a.pred, a.ldp, a.Rc, a.n_mel, a.u_row = T.ptr(dp), o["ldp"], o["Rc"], o["n_mel"], T.ptr(keep[2][1])
    a.B, a.n_tiles, a.row_start, a.len, a.g = B, n_tiles, T.ptr(keep[0][1]), T.ptr(keep[1][1]), 9.0
    a.g_item, a.star, a.rescale = T.ptr(fl[0]), T.ptr(fl[1]), T.ptr(fl[2])
    a.partials, a.coef, a.report = T.ptr(parts), T.ptr(coef), T.ptr(rep) if want_report else None
    check(eng, eng.lib.vv_cfg_norm_coef(eng.ctx, C.byref(a), stream()))
    torch.cuda.synchronize()
    _bands_intact(parts_w, 10, FILL, "partials")
    _bands_intact(coef_w, 4, FILL, "coef")
    _bands_intact(rep_w, 4, FILL, "report")
    T.frame_intact(pw, dp, "pred")
    return parts.cpu().numpy(), coef.cpu().numpy(), rep.cpu().numpy()


@pytest.mark.parametrize("n_mel,ldp", [(4, 4), (4, 8), (4, 128), (100, 100), (100, 104), (100, 128)])
def test_coef_entry_against_the_mirror_and_float64(rig, n_mel, ldp):
    eng = rig[1]["f32"]
    o = _coef_ops(n_mel, ldp)
    nt = -(-max(LENS) // U.TILE) + 1                                            # one tile of partials nobody owns
    part, coef, rep = _coef_launch(eng, o, nt)
    part2, coef2, _ = _coef_launch(eng, o, nt)
    assert part.tobytes() == part2.tobytes() and coef.tobytes() == coef2.tobytes()              # the repeat: the same bits
    assert coef.tobytes() == rep.tobytes()
    pred = o["pred"].numpy()
    worst = [0.0, 0.0]
    for b, n in enumerate(LENS):
        rows = np.arange(o["start"][b], o["start"][b] + n)
        own = -(-n // U.TILE)
        if not GUIDED[b] or n == 0:
            assert tuple(coef[b]) == (1.0, 1.0), b                              # not guided, or without rows
            assert np.all(part[b, own:] == FILL) and (n == 0 or GUIDED[b] or not part[b, :own].any())      # an unguided item's tiles sum nothing
            continue
        pc, pu = pred[rows, :n_mel], pred[o["u_row"].numpy()[rows], :n_mel]
        want_parts, tot = U.gram_mirror(pc, pu)
        assert part[b, :own].tobytes() == want_parts.tobytes(), (b, "the partial sums equal the mirror bit for bit")
        assert np.all(part[b, own:] == FILL), (b, "a tile past the item's length is not written")
        s, f, bs, bf = U.coef_exact(pc, pu, G_ITEM[b], STAR[b] != 0, RESC[b])
        es, ef = abs(float(coef[b, 0]) - float(s)), abs(float(coef[b, 1]) - float(f))
        print(f"CFG_NORM_COEF M{n_mel} ld{ldp} item {b} n {n}: s {coef[b, 0]:.6f} err {es:.2e} bound {bs:.2e}; f {coef[b, 1]:.6f} err {ef:.2e} bound {bf:.2e}")
        assert es <= bs and ef <= bf, (b, es, bs, ef, bf)
        if STAR[b] == 0:
            assert coef[b, 0] == 1.0
        if RESC[b] == 0:
            assert coef[b, 1] == 1.0
        sm, fm = U.coef_from_sums(tot, pc.size, G_ITEM[b], STAR[b] != 0, RESC[b])
        worst = [max(worst[0], abs(float(sm) - float(coef[b, 0]))), max(worst[1], abs(float(fm) - float(coef[b, 1])))]
    print(f"CFG_NORM_COEF M{n_mel} ld{ldp}: device against the float64 mirror of its own formula: ds {worst[0]:.1e} df {worst[1]:.1e}")
    # an item alone and at another place of the batch: its coefficients and partial sums are the same bits
    for b in (1, 3, 4):
        p1, c1, _ = _coef_launch(eng, o, nt, items=(b,))
        own = -(-LENS[b] // U.TILE)
        assert c1[0].tobytes() == coef[b].tobytes() and p1[0, :own].tobytes() == part[b, :own].tobytes(), b
    rev = list(reversed(range(len(LENS))))
    p2, c2, _ = _coef_launch(eng, o, nt, items=rev)
    for i, b in enumerate(rev):
        assert c2[i].tobytes() == coef[b].tobytes(), b


def test_coef_entry_without_a_map_and_its_refusals(rig):
    """u_row NULL: p_u of row r is row Rc + r and every item is guided; star / rescale NULL: {1, 1} and the sums still written."""
    eng = rig[1]["f32"]
    o = _coef_ops(100, 104, lens=(33, 5), order=(0, 1), guided=(True, True))
    pw, dp = T.framed(o["pred"])
    keep = [T.table(torch.tensor(o["start"]), 0), T.table(torch.tensor(o["lens"]), 0)]
    parts = torch.full((2, 2, 5), FILL, dtype=torch.float64, device=DEV)
    coef = torch.full((2, 2), FILL, device=DEV)
    a = rt.vv_cfg_norm_coef_args()
    a.pred, a.ldp, a.Rc, a.n_mel, a.B, a.n_tiles = T.ptr(dp), 104, o["Rc"], 100, 2, 2
    a.row_start, a.len, a.g, a.partials, a.coef = T.ptr(keep[0][1]), T.ptr(keep[1][1]), 2.0, T.ptr(parts), T.ptr(coef)
    check(eng, eng.lib.vv_cfg_norm_coef(eng.ctx, C.byref(a), stream()))
    torch.cuda.synchronize()
    assert coef.cpu().tolist() == [[1.0, 1.0], [1.0, 1.0]]
    pred = o["pred"].numpy()
    want, _ = U.gram_mirror(pred[:33, :100], pred[38: 38 + 33, :100])
    assert parts[0].cpu().numpy().tobytes() == want.tobytes()
    before = (parts.clone(), coef.clone())
    for bad in (dict(n_mel=6), dict(ldp=96), dict(Rc=0), dict(B=0), dict(B=1025), dict(n_tiles=0), dict(pred=None), dict(coef=None),
                dict(partials=None), dict(row_start=None), dict(pred=T.ptr(dp) + 4), dict(coef=T.ptr(coef) + 4), dict(g=float("nan"))):
        b = rt.vv_cfg_norm_coef_args.from_buffer_copy(a)
        for k, v in bad.items():
            setattr(b, k, v)
        assert eng.lib.vv_cfg_norm_coef(eng.ctx, C.byref(b), stream()) == -22, bad
    torch.cuda.synchronize()
    assert torch.equal(parts, before[0]) and torch.equal(coef, before[1])        # a refused call launches nothing
    check(eng, eng.lib.vv_cfg_norm_coef(eng.ctx, C.byref(a), stream()))          # and leaves the context usable
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------------ 2. the stage kernel
STAGE_CASES = U.stage_cases()


def _norm_stage_launch(eng, case, o, coef):
    """step_util.stage_launch's framing with vv_ode_stage_norm at the end of it: x through the permuted row_src between NaN rows, pred and
    every table inside NaN guard rows, the outputs between bands."""
    xw, dx = T.framed(o.x)
    pw, dp = T.framed(o.pred)
    tw, row_src = T.table(o.row_src, int((~torch.isfinite(o.x[:, 0])).nonzero()[0]) if bool((~torch.isfinite(o.x[:, 0])).any()) else 0)
    uw, du = T.table(o.u_row, o.pred.shape[0])
    d = dict(x=dx, pred=dp, g_item=None, row_src=row_src, k_prev=[], k_out=None, x_out=None)
    keep = [tw, uw]
    if o.g_item is not None:
        gw, d["g_item"] = T.framed(o.g_item, 0, 8)
        keep.append(gw)
    for j in range(case.stage):
        kw, kv = T.framed(o.k_prev[j])
        keep.append(kw)
        d["k_prev"].append(kv)
    outs = {}
    kb, d["k_out"], kg = T.out_rows(case.Rc, case.n_mel)
    outs["k"] = (kb, d["k_out"], kg)
    if not case.last:
        xb, d["x_out"], xg = T.out_rows(case.Rc, case.n_mel)
        outs["x_out"] = (xb, d["x_out"], xg)
    a = T._stage_args(case, o, d, case.Rc, 0)
    cw, dc = T.framed(coef, 0, 4)
    check(eng, eng.lib.vv_ode_stage_norm(eng.ctx, C.byref(a), T.ptr(du), T.ptr(dc), stream()))
    torch.cuda.synchronize()
    T.frame_intact(xw, dx, case.name + ": x")
    T.frame_intact(pw, dp, case.name + ": pred")
    res = dict(x=dx.cpu(), k=None, x_out=None)
    for key, (whole, view, guard) in outs.items():
        _bands_intact(whole, guard, FILL, f"{case.name}: {key}")
        res[key] = view.cpu()
    return res


@pytest.mark.parametrize("case", STAGE_CASES, ids=[c.name for c in STAGE_CASES])
def test_stage_kernel_against_float64(rig, case):
    eng = rig[1]["f32"]
    o = case.ops()
    g = torch.Generator().manual_seed(case.seed)
    coef = torch.stack([0.7 + 0.3 * torch.rand(case.B, generator=g), 0.5 + 0.4 * torch.rand(case.B, generator=g)], dim=1).contiguous()
    if case.B > 1:
        coef[1] = 1.0                                                           # one item with the rule off beside the others
    got = _norm_stage_launch(eng, case, o, coef)
    ref = U.stage_ref(case, o, coef)
    ek = parity_err(got["k"], ref["k"], ref["K"].clamp_min(1e-300))[0]
    state = got["x"][o.xr] if case.last else got["x_out"]
    ea = parity_err(state, ref["acc"], ref["mag"].clamp_min(1e-300))[0]
    bk, ba = U.NORM_SLOPE_C * EPS24, T.STATE_C * EPS24
    print(f"CFG_NORM_STAGE {case.name}: k err/bound {ek / bk:.3f} state err/bound {ea / ba:.3f}")
    assert ek <= bk and ea <= ba, (case.name, ek, bk, ea, ba)
    if not case.last:
        assert T.same_bits(got["x"], o.x), "x is read only before the last stage"
    # coef = {1, 1}: the bits of vv_ode_stage_guided
    ones = torch.ones(case.B, 2)
    a, b = _norm_stage_launch(eng, case, o, ones), T.stage_launch(eng, case, o)
    for key in ("x", "k", "x_out"):
        assert (a[key] is None and b[key] is None) or T.same_bits(a[key], b[key]), (case.name, key)


def test_stage_entry_refusals(rig):
    eng = rig[1]["f32"]
    case = STAGE_CASES[5]
    o = case.ops()
    xw, dx = T.framed(o.x)
    pw, dp = T.framed(o.pred)
    _, row_src = T.table(o.row_src, 0)
    _, du = T.table(o.u_row, o.pred.shape[0])
    k_out = torch.full((case.Rc, case.n_mel), FILL, device=DEV)
    d = dict(x=dx, pred=dp, g_item=None, row_src=row_src, k_prev=[T.framed(k)[1] for k in o.k_prev], k_out=k_out, x_out=None if case.last else torch.full_like(k_out, FILL))
    a = T._stage_args(case, o, d, case.Rc, 0)
    coef = torch.ones(case.B + 1, 2, device=DEV)
    st = stream()
    assert eng.lib.vv_ode_stage_norm(eng.ctx, C.byref(a), None, T.ptr(coef), st) == -22                 # the form sits on the guided kernel: u_row is required
    assert eng.lib.vv_ode_stage_norm(eng.ctx, C.byref(a), T.ptr(du), T.ptr(coef) + 4, st) == -22        # float2 loads
    a.seq_n = 0
    assert eng.lib.vv_ode_stage_norm(eng.ctx, C.byref(a), T.ptr(du), T.ptr(coef), st) == -22            # the item of a row needs seq_n
    torch.cuda.synchronize()
    assert bool((k_out == FILL).all())
    a.seq_n = case.N
    check(eng, eng.lib.vv_ode_stage_norm(eng.ctx, C.byref(a), T.ptr(du), T.ptr(coef), st))
    torch.cuda.synchronize()
    assert not bool((k_out == FILL).any())


# ------------------------------------------------------------------------------------------------ 3. the device against the float64 solver
# cfg_zero_init = 2 on every plan, as the issue lists the cases.  rk4 on 3 points has two steps: K = 2 is outside the 0 <= K <= nfe_step - 2
# the same issue sets for check_cfg_zero_init, so that case asserts the refusal (and that the plan in force stays), and rk4 runs K = 1,
# the one truncation its grid has, beside it.
DEVICE_CASES = [(plan, name, None, 0) for plan in U.NORM_PLANS for name in U.OPTION_SETS] + \
               [(plan, "both", S.INTERVAL, 0) for plan in U.NORM_PLANS] + [(plan, "both", None, 2) for plan in U.NORM_PLANS] + [("rk4", "both", None, 1)]


@pytest.mark.parametrize("plan,name,interval,skip", DEVICE_CASES, ids=[f"{p}-{n}" + ("-interval" if i else "") + (f"-zero_init{k}" if k else "") for p, n, i, k in DEVICE_CASES])
def test_device_matches_the_reference_solver(rig, plan, name, interval, skip):
    spec, engs, data = rig
    eng, d = engs["f32"], data["ragged"]
    per_item = U.OPTION_SETS[name]
    if skip > U.NORM_PLANS[plan][1] - 2:                                        # no step would be left: refused, the plan in force unchanged
        before = (eng.nfe_step, eng.ode_method, eng.cfg_zero_init, eng.n_steps)
        with pytest.raises(ValueError, match="cfg_zero_init must satisfy 0 <= K <= nfe_step - 2"):
            eng.set_nfe(U.NORM_PLANS[plan][1], U.NORM_PLANS[plan][0], skip)
        assert (eng.nfe_step, eng.ode_method, eng.cfg_zero_init, eng.n_steps) == before
        return
    with _Plan(eng, plan, skip):
        assert eng.n_steps == U.NORM_PLANS[plan][1] - 1 - skip
        eng.set_cfg_norm_report(True)
        x = _run(eng, d, _pre(eng, d), S.ITEM_G, per_item, interval).cpu()
        rep = eng.last_cfg_norm_report()
        assert rep.shape == (eng.n_evals, 3, 2) and rep.dtype == np.float32
    for b, g in enumerate(S.ITEM_G):
        star, phi = per_item[b]
        log = []
        r64, y, bd = U.parity_refs(plan, b, g, bool(star), phi, interval, skip)
        U.reference("f64", plan, b, g, bool(star), phi, interval, skip, log=log)
        e = S.err(x[b, :d["lens"][b]], r64)
        print(f"CFG_NORM_PARITY {plan} {name} interval {interval} zero_init {skip} item {b}: err {e:.3e} yardstick {y:.3e} bound {bd:.3e} err/bound {e / bd:.3f}")
        assert e <= bd, (plan, name, b, e, bd)
        # the report: (1, 1) where the item is not guided or has the rule off, else the reference's coefficients to fp32 resolution of a
        # trajectory that has drifted by the parity error (a loose sanity check; the exact statement is the unit entry's)
        guided = {ev for ev, _s, _f in log}
        for ev in range(rep.shape[0]):
            if ev not in guided:
                assert tuple(rep[ev, b]) == (1.0, 1.0), (ev, b)
        for ev, s_ref, f_ref in log:
            assert abs(rep[ev, b, 0] - s_ref) <= 1e-3 and abs(rep[ev, b, 1] - f_ref) <= 1e-3, (ev, b, rep[ev, b], s_ref, f_ref)
            if not star:
                assert rep[ev, b, 0] == 1.0
            if not phi:
                assert rep[ev, b, 1] == 1.0


# ------------------------------------------------------------------------------------------------ 4. invariances, bit for bit
@pytest.mark.parametrize("dt", ["f32", "bf16"])
@pytest.mark.parametrize("plan", list(U.NORM_PLANS))
def test_invariances_are_bit_exact(rig, dt, plan):
    spec, engs, data = rig
    eng, d = engs[dt], data["ragged"]
    per_item, g, lens = U.OPTION_SETS["mixed"], S.ITEM_G, data["ragged"]["lens"]
    with _Plan(eng, plan, lanes=1):
        eng.set_cfg_norm_report(True)
        pre = _pre(eng, d)
        x = _run(eng, d, pre, g, per_item).cpu()
        rep = eng.last_cfg_norm_report()
        assert torch.isfinite(x).all()
        for b in range(3):                                                      # an item alone
            one = data["alone", b]
            xa = _run(eng, one, _pre(eng, one), g[b: b + 1], per_item[b: b + 1]).cpu()
            assert torch.equal(xa[0], x[b, :lens[b]]), (dt, plan, "alone", b)
            if any(per_item[b]):                                                # an item with both off, alone, is a call of the plain entries: no report
                assert np.array_equal(eng.last_cfg_norm_report()[:, 0], rep[:, b]), (dt, plan, "report alone", b)
            else:
                assert (rep[:, b] == 1.0).all()
        p = data["permuted"]                                                    # permuted, with more padding
        xp = _run(eng, p, _pre(eng, p), [g[i] for i in S.PERM], [per_item[i] for i in S.PERM]).cpu()
        for i, b in enumerate(S.PERM):
            assert torch.equal(xp[i, :lens[b]], x[b, :lens[b]]), (dt, plan, "permuted", b)
        eng.set_option("lanes", 2)                                              # item lanes in the batch, branch lanes at B = 1
        assert torch.equal(_run(eng, d, pre, g, per_item).cpu(), x), (dt, plan, "item lanes")
        assert np.array_equal(eng.last_cfg_norm_report(), rep)
        one = data["alone", S.ONE]
        xa = _run(eng, one, _pre(eng, one), g[S.ONE: S.ONE + 1], per_item[:1]).cpu()
        eng.set_option("lanes", 1)
        xb = _run(eng, one, _pre(eng, one), g[S.ONE: S.ONE + 1], per_item[:1]).cpu()
        assert torch.equal(xa, xb), (dt, plan, "branch lanes")
        eng.set_cfg_norm_report(False)
        if eng.plan.beta is None:                                               # split by step0 (a multistep call starts at step 0)
            first = max(1, eng.n_steps // 2)
            xs = _run(eng, d, pre, g, per_item, calls=[(0, first), (first, eng.n_steps - first)]).cpu()
            assert torch.equal(xs, x), (dt, plan, "split")
        # captured into a graph and replayed, from a caller-owned workspace of exactly the bytes the size query names
        need = eng.norm_ws_bytes(3, d["N"], lens)
        assert need % 256 == 0 and need > eng.guided_ws_bytes(3, d["N"], lens)
        block = torch.full((need + 4096,), 0xA5, dtype=torch.uint8, device=DEV)
        xg = d["noise"].clone()
        _run(eng, d, pre, g, per_item, ws=block[:need], x=xg)                   # warm-up: sets kernel attributes before the capture
        assert torch.equal(xg.cpu(), x), (dt, plan, "caller-owned workspace")
        cfg = torch.tensor(list(g), dtype=torch.float32, device=DEV)
        norm, host = _norm(eng, per_item), _host(d)
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            eng.transformer_steps_ex(xg, pre, 0, eng.n_steps, host, cfg, ws=block[:need], guide=eng.guidance_mask(None, list(g)), cfg_norm=norm)
        xg.copy_(d["noise"])
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(xg.cpu(), x), (dt, plan, "captured and replayed")
        assert bool((block[need:] == 0xA5).all())
        del graph


# ------------------------------------------------------------------------------------------------ 5. off means off; the report; the profiler
@pytest.mark.parametrize("dt", ["f32", "bf16"])
@pytest.mark.parametrize("plan", list(U.NORM_PLANS))
def test_off_means_off(rig, dt, plan):
    """norm = NULL is vv_transformer_steps_guided; arrays that are off for every item give its bits through the new entry and kernels; an
    item that is off beside items that are on has the bits of the plain call."""
    spec, engs, data = rig
    eng, d = engs[dt], data["ragged"]
    g = S.ITEM_G
    with _Plan(eng, plan):
        pre = _pre(eng, d)
        cfg = torch.tensor(list(g), dtype=torch.float32, device=DEV)
        for interval in (None, S.INTERVAL):
            guide = eng.guidance_mask(interval, list(g))
            want = d["noise"].clone()
            eng.transformer_steps_ex(want, pre, 0, eng.n_steps, _host(d), cfg, guide=guide)
            a = rt.vv_steps_args()
            a.B, a.N, a.seq_len, a.seq_len_host = 3, d["N"], pre["seq_len"].data_ptr(), C.cast(_host(d), C.c_void_p)
            a.cat_mel_text, a.cat_mel_text_drop, a.rope_cos_q, a.rope_sin_q, a.rope_cos_k, a.rope_sin_k = rt._pre_ptrs(pre)
            a.step0, a.n_steps, a.cfg_item = 0, eng.n_steps, cfg.data_ptr()
            x0 = d["noise"].clone()
            a.x = x0.data_ptr()
            check(eng, eng.lib.vv_transformer_steps_norm(eng.ctx, C.byref(a), guide.data_ptr(), 3, None, stream()))      # norm NULL
            zeros = torch.zeros(3, device=DEV)
            x1 = d["noise"].clone()
            eng.transformer_steps_ex(x1, pre, 0, eng.n_steps, _host(d), cfg, guide=guide, cfg_norm=(zeros, zeros))       # all-off arrays: the new kernels run
            x2 = d["noise"].clone()
            eng.transformer_steps_ex(x2, pre, 0, eng.n_steps, _host(d), cfg, guide=guide, cfg_norm=(None, zeros))
            torch.cuda.synchronize()
            assert torch.equal(x0, want) and torch.equal(x1, want) and torch.equal(x2, want), (dt, plan, interval)
        xm = _run(eng, d, pre, g, U.OPTION_SETS["mixed"])
        plain = d["noise"].clone()
        eng.transformer_steps_ex(plain, pre, 0, eng.n_steps, _host(d), cfg, guide=eng.guidance_mask(None, list(g)))
        torch.cuda.synchronize()
        L = d["lens"]
        assert torch.equal(xm[2, :L[2]], plain[2, :L[2]]) and torch.equal(xm[1, :L[1]], plain[1, :L[1]])      # the off item and the unguided item
        assert not torch.equal(xm[0, :L[0]], plain[0, :L[0]])                                                 # the item that is on
        # without a mask (every item guided everywhere): the same bits as with a mask of ones
        per_item = U.OPTION_SETS["both"]
        g1 = (2.0, 1.0, 3.0)
        c1 = torch.tensor(g1, dtype=torch.float32, device=DEV)
        xa, xb = d["noise"].clone(), d["noise"].clone()
        eng.transformer_steps_ex(xa, pre, 0, eng.n_steps, _host(d), c1, guide=None, cfg_norm=_norm(eng, per_item))
        eng.transformer_steps_ex(xb, pre, 0, eng.n_steps, _host(d), c1, guide=torch.ones((eng.n_evals, 3), dtype=torch.uint8), cfg_norm=_norm(eng, per_item))
        torch.cuda.synchronize()
        assert torch.equal(xa, xb)


def _pred_rows(spec, ws, R):
    """The DiT's output of the last evaluation in a one-lane fp32 workspace (test_cfg_reuse_gpu._pred_offset)."""
    from tests.test_cfg_reuse_gpu import _pred_offset
    MP = (spec.n_mel + 127) // 128 * 128
    o = _pred_offset(spec, R)
    return ws[o: o + R * MP * 4].view(torch.float32).reshape(R, MP).cpu().numpy()


def test_report_equals_the_unit_entry_and_the_profiler_counts(rig):
    """A call that stops behind evaluation e leaves the DiT's output of e in a caller-owned workspace: the report row of e equals
    vv_cfg_norm_coef (and so the mirror) on those predictions.  The two launches per evaluation and lane count as elementwise."""
    spec, engs, data = rig
    eng, d = engs["f32"], data["ragged"]
    lens, N, M = d["lens"], d["N"], spec.n_mel
    Rc = sum(lens)
    g, per_item = (2.0, 1.5, 3.0), U.OPTION_SETS["both"]
    with _Plan(eng, "euler", lanes=1):
        pre = _pre(eng, d)
        eng.set_cfg_norm_report(True)
        _run(eng, d, pre, g, per_item)
        rep = eng.last_cfg_norm_report()
        assert rep.shape == (7, 3, 2) and (rep[:, :, 0] != 1.0).all() and (rep[:, :, 1] != 1.0).all()
        need = eng.norm_ws_bytes(3, N, lens)
        ws = torch.zeros(need, dtype=torch.uint8, device=DEV)
        starts = [0, lens[0], lens[0] + lens[1]]
        for e in (0, 3):
            _run(eng, d, pre, g, per_item, calls=[(0, e + 1)], ws=ws)
            part = eng.last_cfg_norm_report()
            assert np.array_equal(part[: e + 1], rep[: e + 1]) and not part[e + 1:].any()      # rows of evaluations outside the call are not written
            pred = _pred_rows(spec, ws, 2 * Rc)
            o = dict(B=3, Rc=Rc, Ru=Rc, start=starts, lens=lens, u_row=(Rc + torch.arange(Rc)).to(I32), pred=torch.from_numpy(pred.copy()), n_mel=M,
                     ldp=pred.shape[1])
            _, coef, _ = _coef_launch(eng, o, (N + U.TILE - 1) // U.TILE, g_item=g, star=(1.0,) * 3, resc=(U.PHI,) * 3)
            assert coef.tobytes() == rep[e].tobytes(), e
            for b in range(3):
                rows = slice(starts[b], starts[b] + lens[b])
                _, tot = U.gram_mirror(pred[rows, :M], pred[Rc + starts[b]: Rc + starts[b] + lens[b], :M])
                sm, fm = U.coef_from_sums(tot, lens[b] * M, g[b], True, U.PHI)
                assert abs(float(sm) - rep[e, b, 0]) <= EPS24 * abs(float(sm)) * 2 and abs(float(fm) - rep[e, b, 1]) <= EPS24 * 2
        eng.set_cfg_norm_report(False)
        from tests.test_cfg_reuse_gpu import _prof
        cfg = torch.tensor(list(g), dtype=torch.float32, device=DEV)
        ones = torch.ones((eng.n_evals, 3), dtype=torch.uint8)
        base = _prof(eng, lambda: (eng.transformer_steps_ex(d["noise"].clone(), pre, 0, eng.n_steps, _host(d), cfg, guide=ones), torch.cuda.synchronize()))
        on = _prof(eng, lambda: _run(eng, d, pre, g, per_item))
        assert on["elementwise"]["launches"] == base["elementwise"]["launches"] + 2 * eng.n_evals
        for cls in on:
            if cls != "elementwise":
                assert on[cls]["launches"] == base[cls]["launches"], cls
        eng.set_option("lanes", 2)
        on2 = _prof(eng, lambda: _run(eng, d, pre, g, per_item))
        base2 = _prof(eng, lambda: (eng.transformer_steps_ex(d["noise"].clone(), pre, 0, eng.n_steps, _host(d), cfg, guide=ones), torch.cuda.synchronize()))
        assert on2["elementwise"]["launches"] == base2["elementwise"]["launches"] + 2 * 2 * eng.n_evals      # per evaluation and lane


@pytest.mark.parametrize("plan,K", [("euler", 1), ("euler", 2), ("rk4", 1), ("ab2", 2)])
def test_zero_init_launches_fewer_evaluations(rig, plan, K):
    """cfg_zero_init = K: K s fewer evaluations, by the profiler's launch counts (every class: an evaluation's launches are the same)."""
    spec, engs, data = rig
    eng, d = engs["bf16"], data["ragged"]
    from tests.test_cfg_reuse_gpu import _prof
    counts = {}
    for skip in (0, K):
        with _Plan(eng, plan, skip, lanes=1):
            pre = _pre(eng, d)
            counts[skip] = (_prof(eng, lambda: _run(eng, d, pre, (2.0, 1.0, 3.0), U.OPTION_SETS["both"])), eng.n_evals, eng.plan.s)
    (full, E, s), (cut, Ec, _) = counts[0], counts[K]
    assert E - Ec == K * s
    for cls in ("gemm", "attention", "norm"):
        assert full[cls]["launches"] % E == 0 and cut[cls]["launches"] == full[cls]["launches"] // E * Ec, (cls, full[cls], cut[cls])


# ------------------------------------------------------------------------------------------------ 6. refusals
def test_refused_calls_leave_the_context_usable(rig):
    spec, engs, data = rig
    eng, d = engs["bf16"], data["ragged"]
    g, per_item = S.ITEM_G, U.OPTION_SETS["both"]
    with _Plan(eng, "euler"):
        pre = _pre(eng, d)
        x0 = _run(eng, d, pre, g, per_item)
        x = d["noise"].clone()
        cfg = torch.tensor(list(g), dtype=torch.float32, device=DEV)
        norm = _norm(eng, per_item)
        a = rt.vv_steps_args()
        a.B, a.N, a.seq_len, a.x, a.seq_len_host = 3, d["N"], pre["seq_len"].data_ptr(), x.data_ptr(), C.cast(_host(d), C.c_void_p)
        a.cat_mel_text, a.cat_mel_text_drop, a.rope_cos_q, a.rope_sin_q, a.rope_cos_k, a.rope_sin_k = rt._pre_ptrs(pre)
        a.step0, a.n_steps, a.cfg_item = 0, eng.n_steps, cfg.data_ptr()
        q = rt.vv_cfg_norm_args(norm[0].data_ptr(), norm[1].data_ptr(), None)
        st = stream()
        two = eng.guidance_mask(None, list(g), 2)
        assert bool((two == 2).any())
        assert eng.lib.vv_transformer_steps_norm(eng.ctx, C.byref(a), two.data_ptr(), 3, C.byref(q), st) == -22          # a 2 in the mask: guidance reuse
        assert b"guidance reuse" in eng.lib.vv_last_error(eng.ctx)
        late = torch.ones((eng.n_evals, 3), dtype=torch.uint8)
        late[6, 0] = 2
        a.n_steps = 3                                                                                                  # wherever the 2 stands
        assert eng.lib.vv_transformer_steps_norm(eng.ctx, C.byref(a), late.data_ptr(), 3, C.byref(q), st) == -22
        a.n_steps = eng.n_steps
        ones = torch.ones((eng.n_evals, 3), dtype=torch.uint8)
        narrow = ones[:, :2].contiguous()
        assert eng.lib.vv_transformer_steps_norm(eng.ctx, C.byref(a), narrow.data_ptr(), 2, C.byref(q), st) == -22       # ld_guide < B
        a.step0 = 5
        assert eng.lib.vv_transformer_steps_norm(eng.ctx, C.byref(a), ones.data_ptr(), 3, C.byref(q), st) == -22         # steps outside the grid
        a.step0 = 0
        bad = rt.vv_cfg_norm_args(norm[0].data_ptr() + 2, norm[1].data_ptr(), None)
        assert eng.lib.vv_transformer_steps_norm(eng.ctx, C.byref(a), ones.data_ptr(), 3, C.byref(bad), st) == -22       # star is no float array
        a.seq_len_host, a.ws, a.ws_bytes = None, x.data_ptr(), 1 << 20
        assert eng.lib.vv_transformer_steps_norm(eng.ctx, C.byref(a), ones.data_ptr(), 3, C.byref(q), st) == -22         # a workspace block needs the host lengths
        a.seq_len_host, a.ws, a.ws_bytes = C.cast(_host(d), C.c_void_p), None, 0
        try:
            eng.set_option("split_k_tail", 1)
            assert eng.lib.vv_transformer_steps_norm(eng.ctx, C.byref(a), ones.data_ptr(), 3, C.byref(q), st) == -22     # what the guided call refuses
            assert eng.lib.vv_transformer_steps_norm(eng.ctx, C.byref(a), None, 0, C.byref(q), st) == -22
        finally:
            eng.set_option("split_k_tail", 0)
        need = eng.norm_ws_bytes(3, d["N"], d["lens"])
        ws = torch.empty((need,), dtype=torch.uint8, device=DEV)
        with pytest.raises(RuntimeError, match="too small"):
            _run(eng, d, pre, g, per_item, ws=ws[: need - 256], x=x)
        # the routing's own refusals, each in its own words
        mask2 = eng.guidance_mask(None, list(g), 2)
        with pytest.raises(ValueError, match="guidance reuse"):
            eng.transformer_steps_ex(x, pre, 0, eng.n_steps, _host(d), cfg, guide=mask2, cfg_norm=norm)
        with pytest.raises(ValueError, match="projected guidance"):
            eng.transformer_steps_ex(x, pre, 0, eng.n_steps, _host(d), cfg, apg=eng.apg_tensors([0.5] * 3, [None] * 3), cfg_norm=norm)
        with pytest.raises(ValueError, match="block caching"):
            eng.transformer_steps(x, pre, 0, eng.n_steps, cfg=cfg, block_cache=(1, 3, 2), cfg_norm=norm)
        with pytest.raises(ValueError, match="pair"):
            eng.transformer_steps_ex(x, pre, 0, eng.n_steps, _host(d), cfg, cfg_norm=(norm[0].cpu(), None))
        torch.cuda.synchronize()
        assert torch.equal(x, d["noise"])                                                                              # nothing ran
        check(eng, eng.lib.vv_transformer_steps_norm(eng.ctx, C.byref(a), None, 0, C.byref(q), st))                      # no mask: every item guided everywhere
        torch.cuda.synchronize()
        xm = _run(eng, d, pre, g, per_item, ws=ws)
        assert torch.equal(xm, x0)
        # item 1 has strength 0: guided everywhere with g = 0 its slope is p_c times f = 1 -- the unmasked call gives the masked call's bits
        assert torch.equal(x, x0)


# ------------------------------------------------------------------------------------------------ 7. the engine and the front end
LONG = "Hôm nay trời đẹp quá, chúng ta cùng nhau đi dạo quanh hồ nhé. " * 4


def _engine(tmp, **kw):
    from vietvoice_tts_amd.core import ModelConfig, TTSEngine
    cfg = ModelConfig(model_cache_dir=str(tmp), synthetic_model=True, model_spec="tiny", nfe_step=8, acoustic_dtype="fp32", max_chunk_duration=8.0, **kw)
    return TTSEngine(cfg)


def _lsb(a, b):
    return int(np.abs(a.astype(np.int32) - b.astype(np.int32)).max())


def test_engine_session_and_device_paths(tmp_path):
    """The device path, the session path, the stream and an edit honour the engine's values; the <= 2 LSB figure is the tolerance of the
    same comparisons of N7 / N8 / N21 (the session path carries the state through the host between its calls)."""
    opts = dict(cfg_zero_star=True, cfg_rescale=0.7, cfg_zero_init=1, cfg_strength=3.0)
    e = _engine(tmp_path, cfg_norm_report=True, **opts)
    wave, _ = e.synthesize(LONG)
    reports, n_chunks = e.last_cfg_norm_report, len(e._last_plan)
    assert n_chunks > 1 and len(reports) >= 1 and sum(r.shape[1] for r in reports) == n_chunks
    for rep in reports:
        assert rep.shape[0] == 6 and rep.shape[2] == 2 and rep.dtype == np.float32          # 8 points, one step skipped: 6 evaluations
        assert (rep[:, :, 0] != 1.0).all() and (rep[:, :, 1] != 1.0).all() and np.isfinite(rep).all()      # every item guided at every evaluation, both on
    e.cleanup()
    e = _engine(tmp_path, **opts)                                                           # a fresh engine each: the same seeded noise stream from its start
    ref, txt = e.model_session_manager.select_sample()
    waves = e._synthesize_sessions(e._prepare_inputs(ref, txt, LONG))
    got = e.audio_processor.concatenate_with_crossfade_improved(waves, e.config.cross_fade_duration, e.config.sample_rate)
    e.cleanup()
    assert got.shape == wave.shape and _lsb(got, wave) <= 2
    e = _engine(tmp_path, **opts)
    streamed = np.concatenate(list(e.synthesize_stream(LONG, chunks_per_step=1)))
    e.cleanup()
    assert streamed.shape == wave.shape and _lsb(streamed, wave) <= 2
    seen = [wave]
    for drop in ("cfg_zero_star", "cfg_rescale", "cfg_zero_init"):                          # each of the three is honoured: without it, other audio
        kw = {k: v for k, v in opts.items() if k != drop}
        e2 = _engine(tmp_path, **kw)
        w2, _ = e2.synthesize(LONG)
        assert e2.last_cfg_norm_report == []
        e2.cleanup()
        assert w2.shape == wave.shape and all(_lsb(w2, w) > 2 for w in seen), drop
        seen.append(w2)
    with pytest.raises(ValueError, match="block_cache"):
        _engine(tmp_path, cfg_zero_star=True, block_cache=(0, 2, 2))


def test_engine_edit_speech_honours_the_options(tmp_path):
    e0, e1 = _engine(tmp_path, cfg_strength=3.0), _engine(tmp_path, cfg_strength=3.0, cfg_zero_star=True, cfg_rescale=0.7, cfg_norm_report=True)
    clip, _ = e0.synthesize("Xin chào các bạn, hôm nay trời đẹp quá.")
    dur = clip.size / e0.config.sample_rate
    text = "Xin chào các anh, hôm nay trời đẹp quá."
    a, _ = e0.edit_speech(clip, text, [(0.3 * dur, 0.5 * dur)], seed=11)
    b, _ = e1.edit_speech(clip, text, [(0.3 * dur, 0.5 * dur)], seed=11)
    assert len(e1.last_cfg_norm_report) == 1 and e1.last_cfg_norm_report[0].shape == (7, 1, 2)
    assert a.shape == b.shape and _lsb(a, b) > 2
    e0.cleanup()
    e1.cleanup()


def test_batching_frontend_per_request_options(tmp_path):
    from vietvoice_tts_amd.batching import BatchingFrontend
    e = _engine(tmp_path)
    fe = BatchingFrontend(e, max_wait_ms=300.0, max_requests=8)
    text = "Xin chào các bạn, hôm nay thế nào?"
    try:
        star = fe.submit(text, speed=1.0, serial=7, cfg_zero_star=True, cfg_strength=3.0).result(timeout=300)[0]
        resc = fe.submit(LONG, speed=0.8, serial=9, cfg_rescale=0.7, cfg_strength=3.0).result(timeout=300)[0]
        default = fe.submit(text, speed=1.0, serial=7, cfg_strength=3.0).result(timeout=300)[0]
        n0 = fe.batches_run
        futs = [fe.submit(text, speed=1.0, serial=7, cfg_zero_star=True, cfg_strength=3.0),
                fe.submit(LONG, speed=0.8, serial=9, cfg_rescale=0.7, cfg_strength=3.0),
                fe.submit(text, speed=1.0, serial=7, cfg_strength=3.0),
                fe.submit(LONG, speed=0.8, serial=10, apg_eta=0.5),             # projected guidance beside it: another request of the batch
                fe.submit("Tạm biệt và hẹn gặp lại.", speed=1.3, serial=8, gender="male", cfg_reuse=2)]
        outs = [f.result(timeout=300)[0] for f in futs]
        assert fe.batches_run == n0 + 1
        assert outs[0].shape == star.shape and _lsb(outs[0], star) <= 2                     # two requests with different options equal themselves alone
        assert outs[1].shape == resc.shape and _lsb(outs[1], resc) <= 2
        assert outs[2].shape == default.shape and _lsb(outs[2], default) <= 2
        assert default.shape == star.shape and _lsb(default, star) > 2
        with pytest.raises(ValueError, match="apg_eta / apg_norm"):
            fe.submit(text, cfg_zero_star=True, apg_eta=0.5).result(timeout=5)
        with pytest.raises(ValueError, match="cfg_reuse > 1"):
            fe.submit(text, cfg_rescale=0.5, cfg_reuse=2).result(timeout=5)
    finally:
        fe.close()
        e.cleanup()
