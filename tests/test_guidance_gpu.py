"""-m gpu: N8, the guidance interval: an item that is not guided at an evaluation has no unconditional rows there.

The guided stage kernel against float64 numpy; the masked entry against the unmasked ones bit for bit wherever the two must agree
(all-ones mask, a zero strength, split calls with a zero strength outside the window); a window whose edges fall inside a Runge-Kutta
step against a reference solver written here around ``Oracle.dit_forward``; the structure properties bit for bit; the rows the
profiler counts; the error paths; the engine level.  No test claims a quality gain: the synthetic weights cannot show one."""
import ctypes as C

import numpy as np
import pytest
import torch

from tests.test_e2e_gpu import make_batch

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
LONG = "Hôm nay trời đẹp quá, chúng ta cùng nhau đi dạo quanh hồ nhé. " * 4
RAGGED = dict(a=[256 * 20, 256 * 12 + 100, 256 * 30], t=[30, 11, 47], g=[24, 9, 40])     # the ragged batch of test_ode_gpu.py
TOL = 1e-3            # max-abs state error in units of the reference's range: test_ode_gpu.py's bound (from test_e2e_gpu.py) for this run length
# the evaluations e_lo, e_hi of the window of test_window_inside_a_runge_kutta_step: lo lies between the times of evaluations e_lo - 1 and
# e_lo, hi between e_hi and e_hi + 1, so evaluations [e_lo, e_hi] are guided -- both edges INSIDE a step (midpoint: steps 1 and 2 of 4,
# rk4: steps 0 and 1 of 2)
WINDOW = {"midpoint": (5, 3, 4), "rk4": (3, 2, 5)}    # name: (nfe, e_lo, e_hi)


def _mods():
    from vietvoice_tts_amd import runtime as rt
    from vietvoice_tts_amd.model_spec import ODE_METHODS, guidance_mask, ode_plan
    return rt, ODE_METHODS, ode_plan, guidance_mask


@pytest.fixture(scope="module")
def own(tiny_setup):
    """Engines of this module's own (hip_tiny is shared: its plan is never changed here) and an Oracle whose t_grid is ours to set."""
    from oracle.vv_oracle import Oracle
    from vietvoice_tts_amd.runtime import HipSynth
    spec, w, _ = tiny_setup
    engs = {"f32": HipSynth(spec, w, acoustic_dtype="fp32", nfe_step=8), "bf16": HipSynth(spec, w, acoustic_dtype="bf16", nfe_step=8)}
    yield engs, Oracle(spec, w, nfe_step=8)
    for e in engs.values():
        e.close()


def _dev(batch):
    d = {k: (v.to(DEV) if torch.is_tensor(v) else v) for k, v in batch.items()}
    d["lens"] = [int(v) for v in batch["seq_len"]]          # on the host: nothing is read back inside a call (or a capture)
    return d


def _pre(eng, d):
    return eng.preprocess(d["audio"], d["audio_len"], d["ids"], d["text_len"], d["seq_len"], d["N"], seq_len_host=d["lens"])


def _host(d):
    return (C.c_int32 * len(d["lens"]))(*d["lens"])


def _run(eng, d, pre, guide=None, cfg=None, step0=0, n=None, ws=None, x=None):
    """One call of the struct entry (masked when ``guide`` is given) on a copy of the batch's noise, or on ``x`` in place."""
    x = d["noise"].clone() if x is None else x
    eng.transformer_steps_ex(x, pre, step0, eng.n_steps - step0 if n is None else n, _host(d), cfg, ws=ws, guide=guide)
    return x


def _one(spec, d, batch, b):
    """Item b of a batch as a batch of its own."""
    sl, la, lt = int(batch["seq_len"][b]), int(batch["audio_len"][b]), int(batch["text_len"][b])
    one = dict(audio=d["audio"][b: b + 1, :max(la, spec.n_fft)].contiguous(), audio_len=d["audio_len"][b: b + 1].contiguous(),
               ids=d["ids"][b: b + 1, :lt].contiguous(), text_len=d["text_len"][b: b + 1].contiguous(),
               seq_len=d["seq_len"][b: b + 1].contiguous(), N=sl, noise=d["noise"][b: b + 1, :sl].contiguous(), lens=[sl])
    return one, sl


def _err(x, ref):
    return float((x - ref).abs().max()) / float(ref.abs().max())


def _window_mask(n_evals, B, e_lo, e_hi):
    m = torch.zeros((n_evals, B), dtype=torch.uint8)
    m[e_lo: e_hi + 1] = 1
    return m


def ref_solve_guided(orc, pre, x, method, nfe_step, g, guided):
    """N7's reference solver with N8's rule, one item: k_i = pc + (pc - pu) g where guided[n * s + i], else pc (the unconditional
    branch is not evaluated at all)."""
    _, _, ode_plan, _ = _mods()
    plan = ode_plan(nfe_step, orc.spec.sway_coef, method)
    ropes = (pre["rope_cos_q"], pre["rope_sin_q"], pre["rope_cos_k"], pre["rope_sin_k"])
    for n in range(plan.dt.numel()):
        h, k = float(plan.dt[n]), []
        for i in range(plan.s):
            xi = x
            for j in range(i):
                if plan.a[i][j] != 0.0:
                    xi = xi + (h * plan.a[i][j]) * k[j]
            orc.t_grid = [float(plan.t[n * plan.s + i])]
            pc = orc.dit_forward(xi, pre["cat_mel_text"], ropes, 0)
            if guided[n * plan.s + i]:
                pu = orc.dit_forward(xi, pre["cat_mel_text_drop"], ropes, 0)
                k.append(pc + (pc - pu) * g)
            else:
                k.append(pc)
        for j in range(plan.s):
            if plan.b[j] != 0.0:
                x = x + (h * plan.b[j]) * k[j]
    return x


def window_interval(plan, e_lo, e_hi):
    """(lo, hi) half way between the evaluation times around the window's first and last evaluation."""
    t = [float(v) for v in plan.t]
    return (t[e_lo - 1] + t[e_lo]) / 2, (t[e_hi] + t[e_hi + 1]) / 2


# ------------------------------------------------------------------------------------------------ 1. the guided stage kernel
def _stage_guided(eng, x, pred, ldp, Rc, M, n_prev, k_prev, coef, k_out, x_out, g, row_src, u_row, plain=False):
    rt = _mods()[0]
    a = rt.vv_ode_stage_args()
    a.x, a.pred, a.ldp, a.Rc, a.n_mel, a.n_prev = x.data_ptr(), pred.data_ptr(), ldp, Rc, M, n_prev
    for j in range(3):
        a.k_prev[j] = k_prev[j].data_ptr() if j < len(k_prev) and k_prev[j] is not None else None
    for j, v in enumerate(coef):
        a.coef[j] = v
    a.k_out = None if k_out is None else k_out.data_ptr()
    a.x_out = None if x_out is None else x_out.data_ptr()
    a.g, a.g_item, a.seq_n = g, None, 0
    a.row_src = row_src.data_ptr()
    st = torch.cuda.current_stream().cuda_stream
    if plain:
        return eng.lib.vv_ode_stage(eng.ctx, C.byref(a), st)
    return eng.lib.vv_ode_stage_guided(eng.ctx, C.byref(a), u_row.data_ptr(), st)


@pytest.mark.parametrize("subset", ["mixed", "none", "all"])
@pytest.mark.parametrize("name", ["euler", "midpoint", "rk4"])
def test_guided_stage_against_float64(hip_tiny, name, subset):
    """Every stage of three methods on ragged rows (lengths 40 / 17 / 29, n_mel 100, ldp 128).  ``mixed``: items 0 and 2 guided, the
    last 5 rows of item 2 unmapped as well, item 1 without an unconditional row; ``none``: Ru = 0, pred holds the conditional rows
    alone; ``all``: every row mapped, which must be vv_ode_stage bit for bit.
    Bound per element, N7's derivation: 8 * 2^-24 * (|x| + sum_j |h a_ij| K_j) with K = |pc| + |g| (|pc| + |pu|) for a guided row's
    fresh slope and K = |pc| for an unguided row's (its slope is pc itself); k_out within 4 * 2^-24 * K."""
    ODE_METHODS = _mods()[1]
    eng = hip_tiny["f32"]
    a_t, b_t = ODE_METHODS[name]
    s = len(b_t)
    gen = torch.Generator().manual_seed(300 + s)
    B, N, M, ldp, h, g = 3, 40, 100, 128, 0.07, 2.0
    lens = [40, 17, 29]
    row_src = torch.cat([b * N + torch.arange(n) for b, n in enumerate(lens)]).to(torch.int32)
    Rc = int(row_src.numel())
    u_row = torch.full((Rc,), -1, dtype=torch.int32)
    if subset == "mixed":
        u_row[:40] = Rc + torch.arange(40, dtype=torch.int32)
        u_row[57: 57 + 24] = Rc + 40 + torch.arange(24, dtype=torch.int32)
    elif subset == "all":
        u_row[:] = Rc + torch.arange(Rc, dtype=torch.int32)
    Ru = int((u_row >= 0).sum())
    assert Ru == {"mixed": 64, "none": 0, "all": Rc}[subset]
    has_u = u_row >= 0
    eps = 2.0 ** -24
    for i in range(s):
        last = i == s - 1
        coef = [np.float32(h * float(b_t[j] if last else a_t[i + 1][j])) for j in range(i + 1)]
        x = torch.randn(B * N, M, generator=gen)
        pred = torch.randn(Rc + Ru, ldp, generator=gen)
        k_prev = [torch.randn(Rc, M, generator=gen) for _ in range(i)]
        dx, dp = x.clone().to(DEV), pred.to(DEV)
        dk = [k.to(DEV) if coef[j] != 0 else None for j, k in enumerate(k_prev)]
        k_out = torch.full((Rc, M), 7.0, device=DEV)
        x_out = None if last else torch.full((Rc, M), 7.0, device=DEV)
        rc = _stage_guided(eng, dx, dp, ldp, Rc, M, i, dk, [float(c) for c in coef], k_out, x_out, g, row_src.to(DEV), u_row.to(DEV))
        assert rc == 0, eng.lib.vv_last_error(eng.ctx).decode()
        torch.cuda.synchronize()
        rs = row_src.long()
        pc = pred[:Rc, :M].double()
        pu = torch.zeros_like(pc)
        pu[has_u] = pred[u_row[has_u].long(), :M].double()
        k = torch.where(has_u[:, None], pc + (pc - pu) * g, pc)
        K = torch.where(has_u[:, None], pc.abs() + abs(g) * (pc.abs() + pu.abs()), pc.abs())
        acc, mag = x[rs].double(), x[rs].double().abs()
        for j in range(i):
            if coef[j] != 0:
                acc = acc + float(coef[j]) * k_prev[j].double()
                mag = mag + abs(float(coef[j])) * k_prev[j].double().abs()
        if coef[i] != 0:
            acc = acc + float(coef[i]) * k
            mag = mag + abs(float(coef[i])) * K
        got = (dx.cpu()[rs] if last else x_out.cpu()).double()
        excess = float(((got - acc).abs() - 8 * eps * mag).max())
        print(f"{name} stage {i} {subset}: max excess over the bound {excess:.3e}")
        assert excess <= 0.0, (name, i, subset, excess)
        assert float(((k_out.cpu().double() - k).abs() - 4 * eps * K).max()) <= 0.0, (name, i, subset)
        assert torch.equal(k_out.cpu()[~has_u], pred[:Rc, :M][~has_u])           # an unguided row's slope IS pc
        mask = torch.ones(B * N, dtype=torch.bool)
        mask[rs] = False
        assert torch.equal(dx.cpu()[mask], x[mask])
        if not last:
            assert torch.equal(dx.cpu(), x)
        if subset == "all":                                                      # every row mapped: the plain kernel's bits
            px = x.clone().to(DEV)
            pk = torch.full((Rc, M), 7.0, device=DEV)
            pxo = None if last else torch.full((Rc, M), 7.0, device=DEV)
            assert _stage_guided(eng, px, dp, ldp, Rc, M, i, dk, [float(c) for c in coef], pk, pxo, g, row_src.to(DEV), None, plain=True) == 0
            torch.cuda.synchronize()
            assert torch.equal(px, dx) and torch.equal(pk, k_out) and (last or torch.equal(pxo, x_out))


# ------------------------------------------------------------------------------------------------ 2. all ones == unmasked
@pytest.mark.parametrize("name", ["euler", "rk4"])
@pytest.mark.parametrize("dt", ["f32", "bf16"])
def test_all_ones_mask_equals_the_unmasked_entries(own, tiny_setup, dt, name):
    spec = tiny_setup[0]
    eng = own[0][dt]
    d = _dev(make_batch(spec, RAGGED["a"], RAGGED["t"], RAGGED["g"], seed=3))
    try:
        eng.set_nfe(8 if name == "euler" else 3, name)
        pre = _pre(eng, d)
        ones = torch.ones((eng.n_evals, 3), dtype=torch.uint8)
        for lanes in (1, 2):
            eng.set_option("lanes", lanes)
            x0 = d["noise"].clone()
            eng.transformer_steps(x0, pre, 0, eng.n_steps)                     # vv_transformer_steps_h
            x1 = _run(eng, d, pre)                                               # vv_transformer_steps_ex
            x2 = _run(eng, d, pre, guide=ones)
            x3 = d["noise"].clone()
            eng.transformer_steps(x3, pre, 0, eng.n_steps, guide=torch.ones((eng.n_evals, 5), dtype=torch.uint8))   # ld_guide > B
            torch.cuda.synchronize()
            assert torch.equal(x1, x0) and torch.equal(x2, x0) and torch.equal(x3, x0), (dt, name, lanes)
    finally:
        eng.set_option("lanes", 0)


# ------------------------------------------------------------------------------------------------ 3. unguided == strength zero
@pytest.mark.parametrize("dt", ["f32", "bf16"])
def test_unguided_item_equals_strength_zero(own, tiny_setup, dt):
    spec = tiny_setup[0]
    eng = own[0][dt]
    g = float(spec.cfg_strength)
    d = _dev(make_batch(spec, RAGGED["a"], RAGGED["t"], RAGGED["g"], seed=4))
    for name, nfe in (("euler", 8), ("midpoint", 5)):
        eng.set_nfe(nfe, name)
        pre = _pre(eng, d)
        for b in range(3):
            m = torch.ones((eng.n_evals, 3), dtype=torch.uint8)
            m[:, b] = 0
            gs = [g] * 3
            gs[b] = 0.0
            xm = _run(eng, d, pre, guide=m)
            xz = _run(eng, d, pre, cfg=torch.tensor(gs, dtype=torch.float32, device=DEV))
            xg = _run(eng, d, pre)
            torch.cuda.synchronize()
            assert torch.equal(xm, xz), (dt, name, b)
            sl = int(d["seq_len"][b])
            apart = _err(xm[b, :sl].cpu(), xg[b, :sl].cpu())
            print(f"{dt} {name} item {b}: unguided vs guided {apart:.3e} of range")
            assert apart > 1e-2, (dt, name, b, apart)
            for o in range(3):
                if o != b:
                    assert torch.equal(xm[o], xg[o])


# ------------------------------------------------------------------------------------------------ 4. an Euler window == split calls
@pytest.mark.parametrize("dt", ["f32", "bf16"])
def test_euler_window_equals_split_calls(own, tiny_setup, dt):
    """Guidance at steps 2..4 of 7: three vv_transformer_steps_ex calls whose strengths are 0 outside the window and g inside."""
    spec = tiny_setup[0]
    eng = own[0][dt]
    g = float(spec.cfg_strength)
    d = _dev(make_batch(spec, RAGGED["a"], RAGGED["t"], RAGGED["g"], seed=5))
    eng.set_nfe(8, "euler")
    pre = _pre(eng, d)
    xm = _run(eng, d, pre, guide=_window_mask(7, 3, 2, 4))
    zero, full = torch.zeros(3, dtype=torch.float32, device=DEV), torch.full((3,), g, dtype=torch.float32, device=DEV)
    xs = d["noise"].clone()
    _run(eng, d, pre, cfg=zero, step0=0, n=2, x=xs)
    _run(eng, d, pre, cfg=full, step0=2, n=3, x=xs)
    _run(eng, d, pre, cfg=zero, step0=5, n=2, x=xs)
    xg = _run(eng, d, pre)
    torch.cuda.synchronize()
    assert torch.equal(xm, xs), dt
    assert not torch.equal(xm, xg)


# ------------------------------------------------------------------------------------------------ 5. a window inside a Runge-Kutta step
@pytest.mark.parametrize("name", ["midpoint", "rk4"])
def test_window_inside_a_runge_kutta_step(own, tiny_setup, name):
    spec = tiny_setup[0]
    engs, orc = own
    eng = engs["f32"]
    _, _, ode_plan, guidance_mask = _mods()
    nfe, e_lo, e_hi = WINDOW[name]
    plan = ode_plan(nfe, spec.sway_coef, name)
    interval = window_interval(plan, e_lo, e_hi)
    g = float(spec.cfg_strength)
    mask = guidance_mask(plan, interval, [g] * 3)
    assert mask.tolist() == _window_mask(plan.t.numel(), 3, e_lo, e_hi).tolist()
    col = [int(v) for v in mask[:, 0]]
    steps = [col[n * plan.s: (n + 1) * plan.s] for n in range(plan.dt.numel())]
    assert sum(1 for st in steps if 0 < sum(st) < plan.s) == 2                   # both edges cut a step: its stages differ in guidance
    batch = make_batch(spec, RAGGED["a"], RAGGED["t"], RAGGED["g"], seed=3)
    d = _dev(batch)
    eng.set_nfe(nfe, name)
    x = _run(eng, d, _pre(eng, d), guide=mask).cpu()
    torch.cuda.synchronize()
    for b in range(3):
        la, lt, sl = int(batch["audio_len"][b]), int(batch["text_len"][b]), int(batch["seq_len"][b])
        pre = orc.preprocess(batch["audio"][b, :la], batch["ids"][b, :lt], sl, batch["noise"][b, :sl])
        ref = ref_solve_guided(orc, pre, pre["noise"], name, nfe, g, col)
        ref_full = ref_solve_guided(orc, pre, pre["noise"], name, nfe, g, [1] * len(col))
        err, apart = _err(x[b, :sl], ref), _err(ref_full, ref)
        print(f"{name} window {interval[0]:.4f}..{interval[1]:.4f} item {b}: err {err:.3e} of range; windowed vs fully guided reference {apart:.3e}")
        assert apart > 1e-2, (name, b, apart)
        assert err < TOL, (name, b, err)


# ------------------------------------------------------------------------------------------------ 6. structure, bit for bit
def _masks(n_evals):
    win = torch.zeros((n_evals, 3), dtype=torch.uint8)           # a window per item: the subset changes four times along the run
    win[2:6, 0] = 1
    win[3:5, 1] = 1
    win[1:7, 2] = 1
    return {"all": torch.ones((n_evals, 3), dtype=torch.uint8), "none": torch.zeros((n_evals, 3), dtype=torch.uint8), "window": win}


@pytest.mark.parametrize("kind", ["all", "none", "window"])
@pytest.mark.parametrize("dt,name", [("f32", "midpoint"), ("bf16", "euler")])
def test_structure_is_bit_identical(own, tiny_setup, dt, name, kind):
    spec = tiny_setup[0]
    eng = own[0][dt]
    batch = make_batch(spec, RAGGED["a"], RAGGED["t"], RAGGED["g"], seed=11)
    d = _dev(batch)
    eng.set_nfe(5 if name == "midpoint" else 9, name)
    assert eng.n_evals == 8
    mask = _masks(8)[kind]
    cfg = torch.tensor([2.0, 0.75, 3.25], dtype=torch.float32, device=DEV)
    pre = _pre(eng, d)
    try:
        eng.set_option("lanes", 1)
        x1 = _run(eng, d, pre, guide=mask, cfg=cfg)
        # lanes
        eng.set_option("lanes", 2)
        x2 = _run(eng, d, pre, guide=mask, cfg=cfg)
        torch.cuda.synchronize()
        assert torch.equal(x1, x2), "lanes"
        # each item alone with its column: one lane, and its two branches as the lanes (forked only where the item is guided)
        for b in range(3):
            one, sl = _one(spec, d, batch, b)
            col = mask[:, b: b + 1].contiguous()
            for lanes in (1, 2):
                eng.set_option("lanes", lanes)
                xa = _run(eng, one, _pre(eng, one), guide=col, cfg=cfg[b: b + 1].contiguous())
                torch.cuda.synchronize()
                assert torch.equal(xa[0], x1[b, :sl]), ("alone", b, lanes)
        eng.set_option("lanes", 0)
        # split calls read the same table
        xs = d["noise"].clone()
        half = eng.n_steps // 2
        _run(eng, d, pre, guide=mask, cfg=cfg, step0=0, n=half, x=xs)
        _run(eng, d, pre, guide=mask, cfg=cfg, step0=half, n=eng.n_steps - half, x=xs)
        torch.cuda.synchronize()
        assert torch.equal(xs, x1), "split"
        # a caller-owned workspace of the size the library names, the same for every mask and larger than the plain call's
        lens = [int(v) for v in batch["seq_len"]]
        need = eng.guided_ws_bytes(3, d["N"], lens)
        nb = C.c_uint64()
        eng._check(eng.lib.vv_transformer_ws_bytes(eng.ctx, 3, d["N"], _host(d), C.byref(nb)))
        assert need > int(nb.value)
        ws = torch.empty((need,), dtype=torch.uint8, device=DEV)
        xw = _run(eng, d, pre, guide=mask, cfg=cfg, ws=ws)
        torch.cuda.synchronize()
        assert torch.equal(xw, x1), "ws"
        with pytest.raises(RuntimeError, match="too small"):
            _run(eng, d, pre, guide=mask, cfg=cfg, ws=ws[: int(nb.value)])
        # captured into a hipGraph: no synchronisation, nothing that moves
        xg = d["noise"].clone()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            _run(eng, d, pre, guide=mask, cfg=cfg, ws=ws, x=xg)
        xg.copy_(d["noise"])
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(xg, x1), "graph"
        del graph
    finally:
        eng.set_option("lanes", 0)


# ------------------------------------------------------------------------------------------------ 7. the rows the profiler counts
@pytest.mark.parametrize("lanes", [1, 2])
def test_gemm_flops_follow_the_rows_launched(own, tiny_setup, lanes):
    spec = tiny_setup[0]
    eng = own[0]["bf16"]
    batch = make_batch(spec, RAGGED["a"], RAGGED["t"], RAGGED["g"], seed=6)
    d = _dev(batch)
    lens = [int(v) for v in batch["seq_len"]]
    Rc = sum(lens)
    eng.set_nfe(9, "euler")
    pre = _pre(eng, d)
    masks = _masks(8)
    try:
        eng.set_option("lanes", lanes)
        flops = {}
        for kind in (None, "all", "none", "window"):
            eng.prof_enable(True)
            eng.prof_collect()
            _run(eng, d, pre, guide=None if kind is None else masks[kind])
            flops[kind] = eng.prof_collect()["gemm"]["flops"]
            eng.prof_enable(False)
        assert flops["all"] == flops[None]
        assert flops["none"] / flops[None] == 0.5
        want = sum(Rc + sum(lens[b] for b in range(3) if masks["window"][e, b]) for e in range(8)) / (8 * 2 * Rc)
        got = flops["window"] / flops[None]
        print(f"window: GEMM flops ratio {got:.12f}, rows ratio {want:.12f}")
        assert abs(got - want) <= 1e-9 * want
    finally:
        eng.prof_enable(False)
        eng.set_option("lanes", 0)


# ------------------------------------------------------------------------------------------------ 8. errors
def test_refused_calls_leave_the_context_usable(own, tiny_setup):
    spec = tiny_setup[0]
    eng = own[0]["bf16"]
    d = _dev(make_batch(spec, RAGGED["a"], RAGGED["t"], RAGGED["g"], seed=8))
    eng.set_nfe(8, "euler")
    pre = _pre(eng, d)
    mask = _window_mask(7, 3, 2, 4)
    x0 = _run(eng, d, pre, guide=mask)
    x = d["noise"].clone()
    with pytest.raises(RuntimeError, match="ld_guide"):
        _run(eng, d, pre, guide=mask[:, :2].contiguous(), x=x)                 # ld_guide = 2 < B = 3
    with pytest.raises(ValueError):
        _run(eng, d, pre, guide=mask[:5].contiguous(), x=x)                    # not the plan's evaluations
    try:
        eng.set_option("split_k_tail", 1)
        with pytest.raises(RuntimeError, match="split_k_tail"):
            _run(eng, d, pre, guide=mask, x=x)
    finally:
        eng.set_option("split_k_tail", 0)
    torch.cuda.synchronize()
    assert torch.equal(x, d["noise"])                                          # nothing ran
    x1 = _run(eng, d, pre, guide=mask)
    torch.cuda.synchronize()
    assert torch.equal(x1, x0)


# ------------------------------------------------------------------------------------------------ 9. engine level
def _engine(tmp, **kw):
    from vietvoice_tts_amd.core import ModelConfig, TTSEngine
    cfg = ModelConfig(model_cache_dir=str(tmp), synthetic_model=True, model_spec="tiny", nfe_step=8, acoustic_dtype="fp32",
                      max_chunk_duration=8.0, **kw)
    return TTSEngine(cfg)


def _lsb(a, b):
    return int(np.abs(a.astype(np.int32) - b.astype(np.int32)).max())


def test_engine_interval_device_session_and_stream_paths(tmp_path):
    """The <= 2 LSB figures are the N2 / N7 tolerances of the same comparisons without an interval."""
    e1 = _engine(tmp_path, cfg_interval=(0.2, 0.8))
    m = e1.model_session_manager.engine.guidance_mask((0.2, 0.8), [None])
    assert m is not None and 0 < int(m.sum()) < m.numel()                        # the interval cuts this plan
    wave_dev, _ = e1.synthesize(LONG)
    assert len(e1._last_plan) > 1
    e1.cleanup()
    for fuse in (1, 2):
        e2 = _engine(tmp_path, cfg_interval=(0.2, 0.8), fuse_nfe=fuse)
        ref, txt = e2.model_session_manager.select_sample()
        waves = e2._synthesize_sessions(e2._prepare_inputs(ref, txt, LONG))
        wave_ses = e2.audio_processor.concatenate_with_crossfade_improved(waves, e2.config.cross_fade_duration, e2.config.sample_rate)
        e2.cleanup()
        assert wave_ses.shape == wave_dev.shape and _lsb(wave_ses, wave_dev) <= 2, fuse
    e3 = _engine(tmp_path, cfg_interval=(0.2, 0.8))
    got = np.concatenate(list(e3.synthesize_stream(LONG, chunks_per_step=1)))
    e3.cleanup()
    assert got.shape == wave_dev.shape and _lsb(got, wave_dev) <= 2
    e4 = _engine(tmp_path)                                                       # no interval, same seed: another trajectory
    wave_all, _ = e4.synthesize(LONG)
    e4.cleanup()
    assert wave_all.shape == wave_dev.shape and _lsb(wave_all, wave_dev) > 2
    e5 = _engine(tmp_path, cfg_interval=(0.0, 1.0))                              # the whole range: the unmasked call
    wave_01, _ = e5.synthesize(LONG)
    e5.cleanup()
    assert np.array_equal(wave_01, wave_all)


def test_batching_frontend_per_request_interval(tmp_path):
    from vietvoice_tts_amd.batching import BatchingFrontend
    e = _engine(tmp_path)
    fe = BatchingFrontend(e, max_wait_ms=300.0, max_requests=8)
    text = "Xin chào các bạn, hôm nay thế nào?"
    try:
        alone = fe.submit(text, speed=1.0, serial=7, cfg_interval=(0.2, 0.8)).result(timeout=300)[0]
        default = fe.submit(text, speed=1.0, serial=7).result(timeout=300)[0]
        n0 = fe.batches_run
        futs = [fe.submit("Tạm biệt và hẹn gặp lại.", speed=1.3, serial=8, gender="male", cfg_interval=(0.5, 1.0)),
                fe.submit(text, speed=1.0, serial=7, cfg_interval=(0.2, 0.8)),
                fe.submit(LONG, speed=0.8, serial=9, cfg_strength=0.0),
                fe.submit(LONG, speed=0.8, serial=10)]
        outs = [f.result(timeout=300)[0] for f in futs]
        assert fe.batches_run == n0 + 1
        assert outs[1].shape == alone.shape and _lsb(outs[1], alone) <= 2
        assert default.shape == alone.shape and _lsb(default, alone) > 2
        with pytest.raises(ValueError):
            fe.submit(text, cfg_interval=(0.9, 0.1)).result(timeout=5)
    finally:
        fe.close()
        e.cleanup()


def test_engine_edit_speech_with_an_interval(tmp_path):
    from vietvoice_tts_amd.pack import MAX_POS
    from vietvoice_tts_amd.speech_edit import plan_edit
    e = _engine(tmp_path, cfg_interval=(0.2, 0.8))
    e0 = _engine(tmp_path)
    sr = e.config.sample_rate
    clip, _ = e.synthesize("Xin chào các bạn, hôm nay trời đẹp quá.")
    dur = clip.size / sr
    parts, fix, text = [(0.3 * dur, 0.5 * dur)], [0.3 * dur], "Xin chào các anh, hôm nay trời đẹp quá."
    out, _ = e.edit_speech(clip, text, parts, fix_duration=fix, seed=11)
    base, _ = e0.edit_speech(clip, text, parts, fix_duration=fix, seed=11)
    plan = plan_edit(clip.size, parts, fix, sr, e.config.hop_length, e.model_session_manager.spec.n_fft, MAX_POS)
    e.cleanup()
    e0.cleanup()
    assert out.dtype == np.int16 and out.size == plan.spliced_len
    assert base.shape == out.shape and _lsb(base, out) > 2
