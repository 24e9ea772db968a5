"""-m gpu: N21, guidance reuse: the unconditional branch runs at every k-th guided evaluation of an item; in between the
stored guidance difference D = p_c - p_u is combined with the fresh p_c.

The reuse form of the stage kernel against float64 numpy; a mask without a 2 through the new entry against N8's entry bit for bit; fp32
runs against a reference solver written around ``Oracle.dit_forward`` that keeps D itself; the structure properties bit for bit; the rows
and launches the profiler counts; the drift report against its numpy mirror bit for bit; the refusals; the engine level.  No test claims a
quality gain or loss: the synthetic model's guidance difference is arbitrary."""
import ctypes as C
import math

import numpy as np
import pytest
import torch

from tests import cfg_reuse_util as U
from tests.test_e2e_gpu import make_batch

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
LONG = "Hôm nay trời đẹp quá, chúng ta cùng nhau đi dạo quanh hồ nhé. " * 4
# three ragged items of 31, 32 and 45 frames: below, at and above a VV_APG_TILE (32-frame) boundary
RAGGED = dict(a=[256 * 12, 256 * 14 + 100, 256 * 20], t=[20, 11, 30], g=[18, 17, 24])
TOL = 1e-3            # max-abs state error in units of the reference's range: the project's bound for N7 / N8 / N20 at these run lengths


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


@pytest.fixture(scope="module")
def ragged(tiny_setup):
    batch = make_batch(tiny_setup[0], RAGGED["a"], RAGGED["t"], RAGGED["g"], seed=3)
    assert [int(v) for v in batch["seq_len"]] == [31, 32, 45]
    return batch


def _dev(batch):
    d = {k: (v.to(DEV) if torch.is_tensor(v) else v) for k, v in batch.items()}
    d["lens"] = [int(v) for v in batch["seq_len"]]          # on the host: nothing is read back inside a call (or a capture)
    return d


def _pre(eng, d):
    return eng.preprocess(d["audio"], d["audio_len"], d["ids"], d["text_len"], d["seq_len"], d["N"], seq_len_host=d["lens"])


def _host(d):
    return (C.c_int32 * len(d["lens"]))(*d["lens"])


def _run(eng, d, pre, guide=None, cfg=None, step0=0, n=None, ws=None, x=None, entry=None):
    """One call of the struct entry on a copy of the batch's noise, or on ``x`` in place.  entry: True = vv_transformer_steps_reuse,
    False = vv_transformer_steps_guided, None = the runtime's own routing (a 2 in the mask, or the report on)."""
    x = d["noise"].clone() if x is None else x
    eng.transformer_steps_ex(x, pre, step0, eng.n_steps - step0 if n is None else n, _host(d), cfg, ws=ws, guide=guide, reuse_entry=entry)
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


# ------------------------------------------------------------------------------------------------ 1. the reuse form of the stage kernel
def _stage(eng, x, pred, ldp, Rc, M, n_prev, k_prev, coef, k_out, x_out, g, seq_n, row_src, u_row, d_buf=None, modes=None):
    """vv_ode_stage_reuse (modes given) or vv_ode_stage_guided on device tensors; -> rc."""
    rt = _mods()[0]
    a = rt.vv_ode_stage_args()
    a.x, a.pred, a.ldp, a.Rc, a.n_mel, a.n_prev = x.data_ptr(), pred.data_ptr(), ldp, Rc, M, n_prev
    for j in range(3):
        a.k_prev[j] = k_prev[j].data_ptr() if j < len(k_prev) and k_prev[j] is not None else None
    for j, v in enumerate(coef):
        a.coef[j] = v
    a.k_out = None if k_out is None else k_out.data_ptr()
    a.x_out = None if x_out is None else x_out.data_ptr()
    a.g, a.g_item, a.seq_n = g, None, seq_n
    a.row_src = row_src.data_ptr()
    st = torch.cuda.current_stream().cuda_stream
    if modes is None:
        return eng.lib.vv_ode_stage_guided(eng.ctx, C.byref(a), u_row.data_ptr(), st)
    m = (C.c_uint8 * len(modes))(*modes)
    r = rt.vv_reuse_stage_args(d_buf.data_ptr(), C.cast(m, C.c_void_p), len(modes))
    return eng.lib.vv_ode_stage_reuse(eng.ctx, C.byref(a), u_row.data_ptr(), C.byref(r), st)


@pytest.mark.parametrize("subset", ["mixed", "none", "plain"])
@pytest.mark.parametrize("name", ["euler", "rk4"])
def test_reuse_stage_against_float64(hip_tiny, name, subset):
    """Every stage of two methods on ragged rows (lengths 40 / 17 / 29 / 12, n_mel 100, ldp 128).
    ``mixed``: item 0 computed with store, item 1 reused, item 2 computed without store (its LOAD bit is set as well: a mapped row is
    computed whatever LOAD says), item 3 not guided.  ``none``: Ru = 0, pred holds the conditional rows alone; items 0 and 2 reuse, 1 and 3
    are not guided.  ``plain``: every row computed, no store: vv_ode_stage_guided bit for bit.
    Bound per element, N7's derivation: 8 * 2^-24 * (|x| + sum_j |h a_ij| K_j) with K = |pc| + |g| |D| for a guided row's fresh slope (D the
    float64 difference where computed, the stored fp32 value where reused) and K = |pc| for an unguided row's; k_out within 4 * 2^-24 * K.
    The stored D must be the fp32 pc - pu exactly, and d_buf untouched everywhere else."""
    rt, ODE_METHODS = _mods()[:2]
    eng = hip_tiny["f32"]
    a_t, b_t = ODE_METHODS[name]
    s = len(b_t)
    gen = torch.Generator().manual_seed(2100 + s)
    B, N, M, ldp, h, g = 4, 40, 100, 128, 0.07, 2.0
    lens = [40, 17, 29, 12]
    row_src = torch.cat([b * N + torch.arange(n) for b, n in enumerate(lens)]).to(torch.int32)
    item = torch.cat([torch.full((n,), b) for b, n in enumerate(lens)])
    Rc = int(row_src.numel())
    u_row = torch.full((Rc,), -1, dtype=torch.int32)
    L, S = rt.REUSE_LOAD, rt.REUSE_STORE
    if subset == "mixed":
        u_row[:40] = Rc + torch.arange(40, dtype=torch.int32)
        u_row[57: 86] = Rc + 40 + torch.arange(29, dtype=torch.int32)
        modes = [S, L, L, 0]
    elif subset == "none":
        modes = [L | S, 0, L, 0]                      # a STORE bit on a row without p_u stores nothing
    else:
        u_row[:] = Rc + torch.arange(Rc, dtype=torch.int32)
        modes = [0, 0, 0, 0]
    Ru = int((u_row >= 0).sum())
    assert Ru == {"mixed": 69, "none": 0, "plain": Rc}[subset]
    has_u = u_row >= 0
    loads = (~has_u) & torch.tensor([bool(modes[int(b)] & L) for b in item])
    stores = has_u & torch.tensor([bool(modes[int(b)] & S) for b in item])
    assert int(loads.sum()) == {"mixed": 17, "none": 69, "plain": 0}[subset] and int(stores.sum()) == {"mixed": 40, "none": 0, "plain": 0}[subset]
    eps = 2.0 ** -24
    for i in range(s):
        last = i == s - 1
        coef = [np.float32(h * float(b_t[j] if last else a_t[i + 1][j])) for j in range(i + 1)]
        x = torch.randn(B * N, M, generator=gen)
        pred = torch.randn(Rc + Ru, ldp, generator=gen)
        d_old = torch.randn(Rc, M, generator=gen)
        k_prev = [torch.randn(Rc, M, generator=gen) for _ in range(i)]
        dx, dp, dd = x.clone().to(DEV), pred.to(DEV), d_old.clone().to(DEV)
        dk = [k.to(DEV) if coef[j] != 0 else None for j, k in enumerate(k_prev)]
        k_out = torch.full((Rc, M), 7.0, device=DEV)
        x_out = None if last else torch.full((Rc, M), 7.0, device=DEV)
        rc = _stage(eng, dx, dp, ldp, Rc, M, i, dk, [float(c) for c in coef], k_out, x_out, g, N, row_src.to(DEV), u_row.to(DEV), dd, modes)
        assert rc == 0, eng.lib.vv_last_error(eng.ctx).decode()
        torch.cuda.synchronize()
        rs = row_src.long()
        pc32 = pred[:Rc, :M]
        pu32 = torch.zeros_like(pc32)
        pu32[has_u] = pred[u_row[has_u].long(), :M]
        pc = pc32.double()
        D = torch.where(has_u[:, None], pc - pu32.double(), d_old.double())
        guided = has_u | loads
        k = torch.where(guided[:, None], pc + D * g, pc)
        K = torch.where(guided[:, None], pc.abs() + abs(g) * D.abs(), pc.abs())
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
        assert torch.equal(k_out.cpu()[~guided], pc32[~guided])                      # an unguided row's slope IS pc
        want_d = d_old.clone()
        want_d[stores] = (pc32 - pu32)[stores]                                       # one fp32 subtraction, stored as it is
        assert torch.equal(dd.cpu(), want_d), (name, i, subset)
        mask = torch.ones(B * N, dtype=torch.bool)
        mask[rs] = False
        assert torch.equal(dx.cpu()[mask], x[mask])
        if not last:
            assert torch.equal(dx.cpu(), x)
        if subset != "none":                                                         # the computed rows: N8's kernel on the same inputs, bit for bit
            px = x.clone().to(DEV)
            pk = torch.full((Rc, M), 7.0, device=DEV)
            pxo = None if last else torch.full((Rc, M), 7.0, device=DEV)
            assert _stage(eng, px, dp, ldp, Rc, M, i, dk, [float(c) for c in coef], pk, pxo, g, N, row_src.to(DEV), u_row.to(DEV)) == 0
            torch.cuda.synchronize()
            same = has_u | ~guided                                                   # and the unguided ones; a reused row has no N8 counterpart
            assert torch.equal(pk.cpu()[same], k_out.cpu()[same])
            if last:
                assert torch.equal(px.cpu()[rs][same], dx.cpu()[rs][same])
            else:
                assert torch.equal(pxo.cpu()[same], x_out.cpu()[same])
            if subset == "plain":
                assert torch.equal(px, dx) and torch.equal(pk, k_out) and (last or torch.equal(pxo, x_out))


def test_reuse_stage_refusals(hip_tiny):
    rt = _mods()[0]
    eng = hip_tiny["f32"]
    Rc, M, ldp, N = 8, 100, 128, 8
    x, pred, d_buf, k_out = (torch.zeros(s, device=DEV) for s in ((Rc, M), (2 * Rc, ldp), (Rc, M), (Rc, M)))
    row_src = torch.arange(Rc, dtype=torch.int32, device=DEV)
    u_row = (Rc + torch.arange(Rc, dtype=torch.int32)).to(DEV)
    go = lambda **kw: _stage(eng, x, pred, ldp, Rc, M, 0, [], [0.1], k_out, None, 2.0, kw.pop("seq_n", N), row_src, u_row,
                             kw.pop("d_buf", d_buf), kw.pop("modes", [rt.REUSE_STORE]))
    assert go() == 0
    assert go(seq_n=0) == -22                                # the item of a row needs the padded sequence length
    assert go(modes=[4]) == -22                              # an item mode is LOAD | STORE at the most
    assert go(d_buf=k_out) == -22                            # d_buf aliases an output of the launch
    assert go(d_buf=d_buf.view(-1)[1:]) == -22               # not 16-byte aligned
    assert go() == 0
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------------ 2. off is today's call
def _window_masks(n_evals):
    win = torch.zeros((n_evals, 3), dtype=torch.uint8)           # a window per item: the subset changes along the run
    win[1: n_evals - 1, 0] = 1
    win[2: n_evals - 2, 1] = 1
    win[0: n_evals - 3, 2] = 1
    return {"ones": torch.ones((n_evals, 3), dtype=torch.uint8), "zeros": torch.zeros((n_evals, 3), dtype=torch.uint8), "window": win}


@pytest.mark.parametrize("dt", ["f32", "bf16"])
@pytest.mark.parametrize("name,nfe", [("euler", 8), ("rk4", 3), ("ab2", 8)])
def test_a_mask_without_a_2_is_the_guided_call(own, ragged, dt, name, nfe):
    eng = own[0][dt]
    d = _dev(ragged)
    try:
        eng.set_nfe(nfe, name)
        pre = _pre(eng, d)
        for kind, mask in _window_masks(eng.n_evals).items():
            for lanes in (1, 2):
                eng.set_option("lanes", lanes)
                ws = torch.empty((eng.guided_ws_bytes(3, d["N"], d["lens"]),), dtype=torch.uint8, device=DEV)     # the figure of this lane plan
                x0 = _run(eng, d, pre, guide=mask, entry=False)                # vv_transformer_steps_guided
                x1 = _run(eng, d, pre, guide=mask, entry=True)                 # vv_transformer_steps_reuse
                x2 = _run(eng, d, pre, guide=mask, entry=True, ws=ws)          # ... in a caller's block of the GUIDED size
                torch.cuda.synchronize()
                assert torch.equal(x1, x0) and torch.equal(x2, x0), (dt, name, kind, lanes)
    finally:
        eng.set_option("lanes", 0)
        eng.set_nfe(8, "euler")


# ------------------------------------------------------------------------------------------------ 3. against a reference solver
CASES = {
    # name: (method, nfe, reuse, interval, strengths)
    "euler k=2": ("euler", 8, 2, None, None),
    "rk4 k=3": ("rk4", 4, 3, None, None),
    "ab2 k=2": ("ab2", 8, 2, None, None),
    "per-item k=(1,2,3) in one interval": ("euler", 8, (1, 2, 3), (0.05, 0.7), None),
    "a strength-0 item": ("euler", 8, 2, None, (2.0, 0.0, 3.0)),
}


@pytest.mark.parametrize("case", list(CASES))
def test_fp32_matches_reference_solver(own, tiny_setup, ragged, case):
    """The device against the test's own solver (cfg_reuse_util.ref_solve_reuse) per item, within TOL of the state's range; and the
    reference with reuse against the reference without it (the same N8 column, every guided evaluation computed): more than ten times
    the device-vs-reference error measured here, so the bound would notice a device that ignored the reuse.  Seeds and strengths were
    chosen on the CPU oracle: the two references are 3e-2 ... 5e-2 of the range apart for every item that reuses."""
    spec = tiny_setup[0]
    engs, orc = own
    eng = engs["f32"]
    _, _, ode_plan, guidance_mask = _mods()
    method, nfe, reuse, interval, gs = CASES[case]
    gs = [float(spec.cfg_strength)] * 3 if gs is None else list(gs)
    plan = ode_plan(nfe, spec.sway_coef, method)
    mask = guidance_mask(plan, interval, gs, reuse)
    base = guidance_mask(plan, interval, gs)
    base = torch.ones_like(mask) if base is None else base
    assert mask is not None and int((mask == 2).sum()) > 0
    d = _dev(ragged)
    try:
        eng.set_nfe(nfe, method)
        cfg = torch.tensor(gs, dtype=torch.float32, device=DEV)
        x = _run(eng, d, _pre(eng, d), guide=mask, cfg=cfg).cpu()
        torch.cuda.synchronize()
    finally:
        eng.set_nfe(8, "euler")
    for b in range(3):
        la, lt, sl = int(ragged["audio_len"][b]), int(ragged["text_len"][b]), int(ragged["seq_len"][b])
        pre = orc.preprocess(ragged["audio"][b, :la], ragged["ids"][b, :lt], sl, ragged["noise"][b, :sl])
        col = [int(v) for v in mask[:, b]]
        ref = U.ref_solve_reuse(orc, pre, pre["noise"], method, nfe, gs[b], col)
        ref_n8 = U.ref_solve_reuse(orc, pre, pre["noise"], method, nfe, gs[b], [int(v) for v in base[:, b]])
        err, apart = _err(x[b, :sl], ref), _err(ref_n8, ref)
        print(f"{case} item {b} column {col}: err {err:.3e} of range; reference with reuse vs without {apart:.3e}")
        assert err < TOL, (case, b, err)
        if 2 in col:
            assert apart > 10 * err, (case, b, apart, err)
        else:
            assert apart == 0.0, (case, b)


# ------------------------------------------------------------------------------------------------ 4. structure, bit for bit
@pytest.mark.parametrize("dt,name,nfe", [("f32", "rk4", 3), ("bf16", "euler", 9), ("f32", "ab2", 9)])
def test_structure_is_bit_identical(own, tiny_setup, ragged, dt, name, nfe):
    spec = tiny_setup[0]
    eng = own[0][dt]
    d = _dev(ragged)
    guidance_mask = _mods()[3]
    eng.set_nfe(nfe, name)
    assert eng.n_evals == 8
    cfg = torch.tensor([2.0, 0.75, 3.25], dtype=torch.float32, device=DEV)
    mask = eng.guidance_mask(None, [2.0, 0.75, 3.25], (1, 2, 3))
    assert [int(v) for v in mask[:, 1]] == [1, 2] * 4 and [int(v) for v in mask[:, 2]] == [1, 2, 2, 1, 2, 2, 1, 2] and bool((mask[:, 0] == 1).all())
    pre = _pre(eng, d)
    try:
        eng.set_option("lanes", 1)
        x1 = _run(eng, d, pre, guide=mask, cfg=cfg)
        # the same call twice with another call's differences left in the workspace in between: a call reads nothing an earlier one left
        _run(eng, d, pre, guide=eng.guidance_mask(None, [1.0] * 3, 4), cfg=cfg.flip(0).contiguous())
        assert torch.equal(_run(eng, d, pre, guide=mask, cfg=cfg), x1), "again"
        # lanes
        eng.set_option("lanes", 2)
        x2 = _run(eng, d, pre, guide=mask, cfg=cfg)
        torch.cuda.synchronize()
        assert torch.equal(x1, x2), "lanes"
        # each item alone with its column: one lane, and its two branches as the lanes (forked only where the item is computed)
        for b in range(3):
            one, sl = _one(spec, d, ragged, b)
            col = mask[:, b: b + 1].contiguous()
            for lanes in (1, 2):
                eng.set_option("lanes", lanes)
                xa = _run(eng, one, _pre(eng, one), guide=col, cfg=cfg[b: b + 1].contiguous())
                torch.cuda.synchronize()
                assert torch.equal(xa[0], x1[b, :sl]), ("alone", b, lanes)
        eng.set_option("lanes", 0)
        # the item with k = 1 among items that reuse is itself under N8 (no mask at all: every item guided everywhere)
        xn8 = _run(eng, d, pre, cfg=cfg)
        torch.cuda.synchronize()
        assert torch.equal(xn8[0], x1[0]) and not torch.equal(xn8[1], x1[1]) and not torch.equal(xn8[2], x1[2])
        # a caller-owned workspace of the size the library names: the same for every mask, the guided figure plus one D buffer per lane
        need, guided = eng.reuse_ws_bytes(3, d["N"], d["lens"]), eng.guided_ws_bytes(3, d["N"], d["lens"])
        one_buf = (sum(d["lens"]) * spec.n_mel * 4 + 255) // 256 * 256
        assert need == guided + one_buf                                         # one lane here (216 packed rows: under the threshold of two)
        ws = torch.empty((need,), dtype=torch.uint8, device=DEV)
        xw = _run(eng, d, pre, guide=mask, cfg=cfg, ws=ws)
        torch.cuda.synchronize()
        assert torch.equal(xw, x1), "ws"
        with pytest.raises(RuntimeError, match="too small"):
            _run(eng, d, pre, guide=mask, cfg=cfg, ws=ws[:guided])
        # captured into a hipGraph: the mask travels as kernel arguments, no synchronisation, nothing that moves
        xg = d["noise"].clone()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            _run(eng, d, pre, guide=mask, cfg=cfg, ws=ws, x=xg)
        xg.copy_(d["noise"])
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(xg, x1), "graph"
        del graph
        # the engine's own captured step graphs (no mask: GraphedSteps carries none) go stale with the plan as ever, reuse calls or not
        if dt == "f32" and name == "rk4":
            gs = eng.capture_steps(3, d["N"], d["lens"], ragged["t_gen_max"])
            assert not gs.stale()
            _run(eng, d, pre, guide=mask, cfg=cfg)
            assert not gs.stale()
            eng.set_nfe(nfe, "euler")
            assert gs.stale()
            with pytest.raises(RuntimeError, match="stale"):
                gs(d["noise"], pre)
    finally:
        eng.set_option("lanes", 0)
        eng.set_nfe(8, "euler")


# ------------------------------------------------------------------------------------------------ 5. the rows and launches the profiler counts
def _prof(eng, fn):
    eng.prof_enable(True)
    eng.prof_collect()
    fn()
    out = eng.prof_collect()
    eng.prof_enable(False)
    return out


@pytest.mark.parametrize("lanes", [1, 2])
def test_gemm_flops_follow_the_rows_launched(own, ragged, lanes):
    """k = 2, full guidance, E = 8 evaluations: Rc (E + ceil(E / 2)) rows against 2 Rc E; per-item k = (1, 2, 3) by the mask's own count."""
    eng = own[0]["bf16"]
    d = _dev(ragged)
    lens, Rc = d["lens"], sum(d["lens"])
    eng.set_nfe(9, "euler")
    E = eng.n_evals
    pre = _pre(eng, d)
    try:
        eng.set_option("lanes", lanes)
        full = _prof(eng, lambda: _run(eng, d, pre))["gemm"]["flops"]
        m2 = eng.guidance_mask(None, [None] * 3, 2)
        got = _prof(eng, lambda: _run(eng, d, pre, guide=m2))["gemm"]["flops"] / full
        want = Rc * (E + math.ceil(E / 2)) / (2 * Rc * E)
        print(f"k = 2: GEMM flops ratio {got:.12f}, rows ratio {want:.12f}")
        assert want == 0.75 and abs(got - want) <= 1e-9 * want
        m123 = eng.guidance_mask(None, [None] * 3, (1, 2, 3))
        got = _prof(eng, lambda: _run(eng, d, pre, guide=m123))["gemm"]["flops"] / full
        want = sum(Rc + sum(lens[b] for b in range(3) if m123[e, b] == 1) for e in range(E)) / (2 * Rc * E)
        print(f"k = (1, 2, 3): GEMM flops ratio {got:.12f}, rows ratio {want:.12f}")
        assert abs(got - want) <= 1e-9 * want
    finally:
        eng.prof_enable(False)
        eng.set_option("lanes", 0)
        eng.set_nfe(8, "euler")


def test_an_evaluation_where_every_item_reuses_launches_no_side_stream_work(own, tiny_setup, ragged):
    """One item, its two branches as the lanes: an evaluation forks and launches the block kernels a second time (on the side stream)
    only where the item has unconditional rows.  With k = 2 that is ceil(E / 2) of the E evaluations -- the launch counts of the GEMM and
    attention classes lie exactly there between the all-zero mask's (never) and the all-ones mask's (always)."""
    spec = tiny_setup[0]
    eng = own[0]["bf16"]
    d = _dev(ragged)
    one, _ = _one(spec, d, ragged, 2)
    eng.set_nfe(9, "euler")
    E = eng.n_evals
    pre = _pre(eng, one)
    try:
        eng.set_option("lanes", 2)
        count = lambda m: _prof(eng, lambda: _run(eng, one, pre, guide=m))
        zeros, ones = count(torch.zeros((E, 1), dtype=torch.uint8)), count(torch.ones((E, 1), dtype=torch.uint8))
        k2 = count(eng.guidance_mask(None, [None], 2))
        for cls in ("gemm", "attention" if "attention" in zeros else "attn"):
            z, o, r = zeros[cls]["launches"], ones[cls]["launches"], k2[cls]["launches"]
            assert o == 2 * z and (o - z) % E == 0, (cls, z, o)
            assert r == z + (o - z) // E * math.ceil(E / 2), (cls, z, o, r)
    finally:
        eng.prof_enable(False)
        eng.set_option("lanes", 0)
        eng.set_nfe(8, "euler")


# ------------------------------------------------------------------------------------------------ 6. the drift report
KL_LENS = [0, 1, U.TILE - 1, U.TILE, U.TILE + 1, 2 * U.TILE + 3]
KL_M = 100


def _drift(eng, pc, pu, d_old, lens, computed, has_old, order=None, n_tiles=None, M=KL_M):
    """vv_cfg_drift_reduce on host arrays given in item order: the items' conditional rows packed back to back in ``order``, the
    unconditional rows of the ``computed`` items compacted behind them in the same order; -> (rc, report [B][2] in item order)."""
    rt = _mods()[0]
    B = len(lens)
    order = list(range(B)) if order is None else order
    src = {b: sum(lens[:b]) for b in range(B)}
    starts, pos = {}, 0
    for b in order:
        starts[b] = pos
        pos += lens[b]
    Rc = max(pos, 1)
    Ru = sum(lens[b] for b in order if computed[b])
    ldp = (M + 127) // 128 * 128
    pred = torch.zeros(Rc + Ru, ldp)
    dbuf = torch.full((Rc, M), float("nan"))
    u_row = torch.full((Rc,), -1, dtype=torch.int32)
    upos = Rc
    for b in order:
        rows = slice(src[b], src[b] + lens[b])
        pred[starts[b]: starts[b] + lens[b], :M] = torch.from_numpy(pc[rows])
        if has_old[b]:
            dbuf[starts[b]: starts[b] + lens[b]] = torch.from_numpy(d_old[rows])
        if computed[b]:
            pred[upos: upos + lens[b], :M] = torch.from_numpy(pu[rows])
            u_row[starts[b]: starts[b] + lens[b]] = upos + torch.arange(lens[b], dtype=torch.int32)
            upos += lens[b]
    n_tiles = -(-max(lens) // U.TILE) if n_tiles is None else n_tiles
    dp, dd, du = pred.to(DEV), dbuf.to(DEV), u_row.to(DEV)
    row_start = torch.tensor([starts[b] for b in order], dtype=torch.int32, device=DEV)
    ln = torch.tensor([lens[b] for b in order], dtype=torch.int32, device=DEV)
    partials = torch.full((B, n_tiles, 2), float("nan"), dtype=torch.float64, device=DEV)
    report = torch.full((B, 2), float("nan"), dtype=torch.float64, device=DEV)
    old = (C.c_uint8 * B)(*[1 if has_old[b] else 0 for b in order])
    a = rt.vv_cfg_drift_args()
    a.pred, a.ldp, a.Rc, a.n_mel, a.u_row, a.d_buf, a.has_old_host = dp.data_ptr(), ldp, Rc, M, du.data_ptr(), dd.data_ptr(), C.cast(old, C.c_void_p)
    a.B, a.n_tiles, a.row_start, a.len, a.partials, a.report = B, n_tiles, row_start.data_ptr(), ln.data_ptr(), partials.data_ptr(), report.data_ptr()
    rc = eng.lib.vv_cfg_drift_reduce(eng.ctx, C.byref(a), torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    out = np.empty((B, 2))
    out[order] = report.cpu().numpy()
    return rc, out


def test_drift_reduce_equals_the_mirror_bit_for_bit(hip_tiny):
    eng = hip_tiny["f32"]
    rng = np.random.default_rng(21)
    R, B = sum(KL_LENS), len(KL_LENS)
    pc = rng.standard_normal((R, KL_M)).astype(np.float32)
    pu = rng.standard_normal((R, KL_M)).astype(np.float32)
    d_old = (pc - pu + 0.25 * rng.standard_normal((R, KL_M))).astype(np.float32)
    off = np.concatenate([[0], np.cumsum(KL_LENS)])
    rows = lambda b: slice(off[b], off[b + 1])
    computed, has_old = [1] * B, [1] * B
    want = np.array([U.drift_mirror(pc[rows(b)], pu[rows(b)], d_old[rows(b)]) for b in range(B)])
    rc, got = _drift(eng, pc, pu, d_old, KL_LENS, computed, has_old)
    assert rc == 0, eng.lib.vv_last_error(eng.ctx).decode()
    assert np.array_equal(got, want), (got, want)
    assert got[0].tolist() == [0.0, 0.0] and (got[1:] > 0).all()
    plain = np.array([U.drift_plain(pc[rows(b)], pu[rows(b)], d_old[rows(b)]) for b in range(B)])
    assert np.allclose(got, plain, rtol=1e-12, atol=0.0)
    # every item at another place of the batch, and with more tiles than it needs: the same bits
    for order, n_tiles in (([5, 4, 3, 2, 1, 0], None), ([3, 0, 5, 1, 4, 2], 7)):
        rc, moved = _drift(eng, pc, pu, d_old, KL_LENS, computed, has_old, order=order, n_tiles=n_tiles)
        assert rc == 0 and np.array_equal(moved, want), order
    # a subset: items 2 and 4 reuse or are not guided (no unconditional rows): {0, 0}; items 3 and 5 have nothing stored yet (d_buf holds
    # NaN for them and is not read): {0, sum D^2}; the others as before
    computed, has_old = [1, 1, 0, 1, 0, 1], [1, 1, 1, 0, 1, 0]
    rc, sub = _drift(eng, pc, pu, d_old, KL_LENS, computed, has_old, order=[1, 5, 2, 0, 4, 3])
    assert rc == 0
    for b in range(B):
        if not computed[b]:
            assert sub[b].tolist() == [0.0, 0.0], b
        elif not has_old[b]:
            assert sub[b].tolist() == [0.0, want[b, 1]], b
        else:
            assert sub[b].tolist() == want[b].tolist(), b
    # refused before any launch
    assert _drift(eng, pc[:, :98], pu[:, :98], d_old[:, :98], KL_LENS, computed, has_old, M=98)[0] == -22      # n_mel % 4
    assert _drift(eng, pc, pu, d_old, KL_LENS, computed, has_old, n_tiles=0)[0] == -22
    rc, again = _drift(eng, pc, pu, d_old, KL_LENS, [1] * B, [1] * B)
    assert rc == 0 and np.array_equal(again, want)


@pytest.mark.parametrize("M", [4, 100])
def test_drift_reduce_at_the_host_check_edges(hip_tiny, M):
    """The batch tools/elementwise_host_check.py runs on exact-size buffers (an empty item, 31, 32, 33 and 45 frames, one tile of partials
    more than the longest needs, one item reusing, one with nothing stored yet, n_mel 4 and 100): the mirror's bits."""
    eng = hip_tiny["f32"]
    pc, pu, d_old = U.edge_predictions(M)
    lens = list(U.EDGE_LENS)
    off = np.concatenate([[0], np.cumsum(lens)])
    rc, got = _drift(eng, pc, pu, d_old, lens, list(U.EDGE_COMPUTED), list(U.EDGE_HAS_OLD), n_tiles=U.EDGE_TILES, M=M)
    assert rc == 0, eng.lib.vv_last_error(eng.ctx).decode()
    for b in range(len(lens)):
        rows = slice(off[b], off[b + 1])
        want = U.drift_mirror(pc[rows], pu[rows], d_old[rows] if U.EDGE_HAS_OLD[b] else None) if U.EDGE_COMPUTED[b] else (0.0, 0.0)
        assert got[b].tolist() == list(want), (b, got[b], want)


REUSE_STAGE = U.reuse_stage_cases()


@pytest.mark.parametrize("case", REUSE_STAGE, ids=[c.name for c in REUSE_STAGE])
def test_reuse_stage_at_the_host_check_shapes(hip_tiny, case):
    """The launches tools/elementwise_host_check.py runs on exact-size buffers: n_mel 4 and 100, ldp tight and + 4, 1 / 3 / 86 rows, the
    three subsets; the bounds and the exact parts of test_reuse_stage_against_float64 (cfg_reuse_util.ReuseStageCase.ref)."""
    eng = hip_tiny["f32"]
    o = case.ops()
    r = case.ref(o)
    Rc, M, i = o.Rc, case.n_mel, case.stage
    dx, dp, dd = o.x.clone().to(DEV), o.pred.to(DEV), o.d_old.clone().to(DEV)
    dk = [k.to(DEV) if o.coef[j] != 0 else None for j, k in enumerate(o.k_prev)]
    k_out = torch.full((Rc, M), 7.0, device=DEV)
    x_out = None if o.last else torch.full((Rc, M), 7.0, device=DEV)
    rc = _stage(eng, dx, dp, case.ldp, Rc, M, i, dk, [float(c) for c in o.coef], k_out, x_out, case.g, case.N, o.row_src.to(DEV), o.u_row.to(DEV), dd, o.modes)
    assert rc == 0, eng.lib.vv_last_error(eng.ctx).decode()
    torch.cuda.synchronize()
    eps = 2.0 ** -24
    rs = o.row_src.long()
    got = (dx.cpu()[rs] if o.last else x_out.cpu()).double()
    assert float(((got - r["acc"]).abs() - 8 * eps * r["mag"]).max()) <= 0.0, case.name
    assert float(((k_out.cpu().double() - r["k"]).abs() - 4 * eps * r["K"]).max()) <= 0.0, case.name
    assert torch.equal(k_out.cpu()[~r["guided"]], r["pc32"][~r["guided"]])
    assert torch.equal(dd.cpu(), r["want_d"]), case.name
    mask = torch.ones(o.x.shape[0], dtype=torch.bool)
    mask[rs] = False
    assert torch.equal(dx.cpu()[mask], o.x[mask]) and (o.last or torch.equal(dx.cpu(), o.x))


def _pred_offset(spec, R):
    """Byte offset of the DiT's output in a one-lane fp32 workspace: the lane's buffers in the order the plan takes them (packed
    conditioning, three activations, the residual stream, qkv, attention, the MLP's middle), each 256-byte aligned."""
    al = lambda v: (v + 255) // 256 * 256
    D, FF, KP = spec.dim, spec.dim * spec.ff_mult, (2 * spec.n_mel + spec.text_dim + 63) // 64 * 64
    off = 0
    for n in (R * KP, R * D, R * D, R * D, R * D, R * 3 * D, R * D, R * FF):
        off = al(off) + 4 * n
    return al(off)


def test_pipeline_report_equals_the_mirror(own, tiny_setup, ragged):
    """last_cfg_reuse_report() of a 4-evaluation Euler call with k = 2 (columns 1, 2, 1, 2) against the mirror applied to the two
    predictions of the same inputs: a call that stops behind evaluation e leaves the DiT's output of e in a caller-owned workspace (fp32
    rows [Rc + Ru][pad128(n_mel)] behind the lane's activation buffers; every item is computed at e = 0 and e = 2, so p_u of row r is row
    Rc + r).  In the batch and for an item alone; the report changes nothing in the state; off, nothing is allocated or launched."""
    spec = tiny_setup[0]
    eng = own[0]["f32"]
    d = _dev(ragged)
    lens, N, M = d["lens"], d["N"], spec.n_mel
    Rc, MP = sum(lens), (M + 127) // 128 * 128
    eng.set_nfe(5, "euler")
    mask = eng.guidance_mask(None, [None] * 3, 2)
    assert mask[:, 0].tolist() == [1, 2, 1, 2]
    assert eng.last_cfg_reuse_report() is None
    try:
        eng.set_option("lanes", 1)
        pre = _pre(eng, d)
        x_off = _run(eng, d, pre, guide=mask)
        off_launches = _prof(eng, lambda: _run(eng, d, pre, guide=mask))["elementwise"]["launches"]
        assert eng.last_cfg_reuse_report() is None
        eng.set_cfg_reuse_report(True)
        x = _run(eng, d, pre, guide=mask)
        rep = eng.last_cfg_reuse_report()
        assert torch.equal(x, x_off)
        assert rep.shape == (4, 3, 2) and rep.dtype == np.float64
        assert not rep[1].any() and not rep[3].any() and not rep[0, :, 0].any()          # {0, 0} where reused, {0, sum D^2} at the first computed one
        assert (rep[0, :, 1] > 0).all() and (rep[2] > 0).all()
        on_launches = _prof(eng, lambda: _run(eng, d, pre, guide=mask))["elementwise"]["launches"]
        assert on_launches == off_launches + 2 * 4                                       # two small launches per evaluation and lane
        # the workspace: the report's partial sums on top, and only when asked for
        need_on, need_off = eng.reuse_ws_bytes(3, N, lens, report=True), eng.reuse_ws_bytes(3, N, lens)
        assert need_on == need_off + (3 * ((N + U.TILE - 1) // U.TILE) * 2 * 8 + 255) // 256 * 256
        ws = torch.zeros(need_on, dtype=torch.uint8, device=DEV)
        D = {}
        for e in (0, 2):
            xk = d["noise"].clone()
            _run(eng, d, pre, guide=mask, n=e + 1, ws=ws, x=xk)
            torch.cuda.synchronize()
            part = eng.last_cfg_reuse_report()
            assert np.array_equal(part[: e + 1], rep[: e + 1]) and not part[e + 1:].any()
            o = _pred_offset(spec, 2 * Rc)
            pred = ws[o: o + 2 * Rc * MP * 4].view(torch.float32).reshape(2 * Rc, MP).cpu().numpy()
            D[e] = (pred[:Rc, :M].copy(), pred[Rc:, :M].copy())
        starts = [0, lens[0], lens[0] + lens[1]]
        for b in range(3):
            rows = slice(starts[b], starts[b] + lens[b])
            first = U.drift_mirror(D[0][0][rows], D[0][1][rows], None)
            d0 = (D[0][0][rows] - D[0][1][rows]).astype(np.float32)
            second = U.drift_mirror(D[2][0][rows], D[2][1][rows], d0)
            assert tuple(rep[0, b]) == first and tuple(rep[2, b]) == second, (b, rep[:, b], first, second)
        print(f"sqrt(E2 / N2) per item over two evaluations: {np.sqrt(rep[2, :, 0] / rep[2, :, 1]).round(4).tolist()}")
        # lanes, and an item alone: its report rows are its own
        eng.set_option("lanes", 2)
        _run(eng, d, pre, guide=mask)
        assert np.array_equal(eng.last_cfg_reuse_report(), rep)
        for b in range(3):
            one, _ = _one(spec, d, ragged, b)
            _run(eng, one, _pre(eng, one), guide=mask[:, b: b + 1].contiguous())
            assert np.array_equal(eng.last_cfg_reuse_report()[:, 0], rep[:, b]), b
        # a report of another shape is refused, and so is one without a mask
        rt = _mods()[0]
        xr = d["noise"].clone()
        a = rt.vv_steps_args()
        a.B, a.N, a.seq_len, a.x, a.seq_len_host = 3, N, pre["seq_len"].data_ptr(), xr.data_ptr(), C.cast(_host(d), C.c_void_p)
        a.cat_mel_text, a.cat_mel_text_drop, a.rope_cos_q, a.rope_sin_q, a.rope_cos_k, a.rope_sin_k = rt._pre_ptrs(pre)
        a.step0, a.n_steps = 0, eng.n_steps
        buf = torch.zeros((4, 3, 2), dtype=torch.float64, device=DEV)
        st = torch.cuda.current_stream().cuda_stream
        for r, g in ((rt.vv_reuse_args(buf.data_ptr(), 2, 4), mask), (rt.vv_reuse_args(buf.data_ptr(), 3, 5), mask), (rt.vv_reuse_args(buf.data_ptr(), 3, 4), None)):
            assert eng.lib.vv_transformer_steps_reuse(eng.ctx, C.byref(a), None if g is None else g.data_ptr(), 3, C.byref(r), st) == -22
        torch.cuda.synchronize()
        assert torch.equal(xr, d["noise"]) and not buf.any()
        assert eng.lib.vv_transformer_steps_reuse(eng.ctx, C.byref(a), mask.data_ptr(), 3, C.byref(rt.vv_reuse_args(buf.data_ptr(), 3, 4)), st) == 0
        torch.cuda.synchronize()
        assert torch.equal(xr, x) and np.array_equal(buf.cpu().numpy(), rep)
    finally:
        eng.set_cfg_reuse_report(False)
        eng.set_option("lanes", 0)
        eng.set_nfe(8, "euler")
    assert eng.last_cfg_reuse_report() is None


# ------------------------------------------------------------------------------------------------ 7. refusals
def test_refused_calls_leave_the_context_usable(own, ragged):
    eng = own[0]["bf16"]
    d = _dev(ragged)
    eng.set_nfe(8, "euler")
    pre = _pre(eng, d)
    mask = eng.guidance_mask(None, [None] * 3, 2)
    x0 = _run(eng, d, pre, guide=mask)
    x = d["noise"].clone()
    def refused(m=None, e0=0, e1=None, why=None):
        """The library's -22; where the mask itself is the reason, the host mirror names the same reason."""
        if m is not None:
            assert U.check_mask(m.tolist(), e0, e1) == why
        return pytest.raises(RuntimeError, match=r"\(-22\)")
    assert U.check_mask(mask.tolist()) is None
    early = mask.clone()
    early[0, 1], early[1, 1] = 2, 1                                            # item 1 reuses at evaluation 0, in front of its first 1
    with refused(early, why="2 before 1"):
        _run(eng, d, pre, guide=early, x=x)
    after_zero = mask.clone()
    after_zero[0, 2] = 0                                                       # item 2: 0, 2, ... -- a 0 is not a 1
    with refused(after_zero, why="2 before 1"):
        _run(eng, d, pre, guide=after_zero, x=x)
    three = mask.clone()
    three[4, 0] = 3
    with refused(three, why="value"):
        _run(eng, d, pre, guide=three, x=x, entry=True)
    with refused(mask, 2, 7, why="step0"):
        _run(eng, d, pre, guide=mask, x=x, step0=2)                            # a 2 in the mask and step0 != 0
    ones = torch.ones_like(mask)
    ones[6, 0] = 2                                                             # ... wherever the 2 stands, also outside the call's evaluations
    with refused(ones, 1, 4, why="step0"):
        _run(eng, d, pre, guide=ones, x=x, step0=1, n=3)
    with refused():
        _run(eng, d, pre, guide=mask[:, :2].contiguous(), x=x)                 # ld_guide = 2 < B = 3
    try:
        eng.set_option("split_k_tail", 1)
        with pytest.raises(RuntimeError, match="split_k_tail"):
            _run(eng, d, pre, guide=mask, x=x)
    finally:
        eng.set_option("split_k_tail", 0)
    need = eng.reuse_ws_bytes(3, d["N"], d["lens"])
    ws = torch.empty((need,), dtype=torch.uint8, device=DEV)
    with pytest.raises(RuntimeError, match="too small"):
        _run(eng, d, pre, guide=mask, x=x, ws=ws[: need - 256])
    apg = eng.apg_tensors([0.5] * 3, [None] * 3)
    with pytest.raises(ValueError, match="projected guidance"):                # no reuse together with APG: the runtime has no entry to send it to
        eng.transformer_steps(x, pre, 0, eng.n_steps, guide=mask, apg=apg)
    torch.cuda.synchronize()
    assert torch.equal(x, d["noise"])                                          # nothing ran
    x1 = _run(eng, d, pre, guide=mask, ws=ws)
    torch.cuda.synchronize()
    assert torch.equal(x1, x0)
    # without a 2 a call may start anywhere: the entry is N8's
    xs, xr = d["noise"].clone(), d["noise"].clone()
    win = _window_masks(7)["window"]
    _run(eng, d, pre, guide=win, x=xs, step0=2, n=3, entry=False)
    _run(eng, d, pre, guide=win, x=xr, step0=2, n=3, entry=True)
    torch.cuda.synchronize()
    assert torch.equal(xs, xr)


# ------------------------------------------------------------------------------------------------ 8. engine level
def _engine(tmp, **kw):
    from vietvoice_tts_amd.core import ModelConfig, TTSEngine
    cfg = ModelConfig(model_cache_dir=str(tmp), synthetic_model=True, model_spec="tiny", nfe_step=8, acoustic_dtype="fp32",
                      max_chunk_duration=8.0, **kw)
    return TTSEngine(cfg)


def _lsb(a, b):
    return int(np.abs(a.astype(np.int32) - b.astype(np.int32)).max())


@pytest.fixture(scope="module")
def wave_k2(tmp_path_factory):
    """The device path's audio with cfg_reuse = 2 and without it (shared by the engine tests), and the drift report of the first."""
    tmp = tmp_path_factory.mktemp("reuse")
    e1 = _engine(tmp, cfg_reuse=2, cfg_reuse_report=True)
    wave, _ = e1.synthesize(LONG)
    n_chunks, reports = len(e1._last_plan), e1.last_cfg_reuse_report
    e1.cleanup()
    e0 = _engine(tmp)
    base, _ = e0.synthesize(LONG)
    e0.cleanup()
    return tmp, wave, base, n_chunks, reports


def test_engine_device_path_report_and_off(wave_k2):
    """The <= 2 LSB figures are the N2 / N7 / N8 tolerances of the same comparisons without reuse."""
    tmp, wave, base, n_chunks, reports = wave_k2
    assert n_chunks > 1
    assert base.shape == wave.shape and _lsb(base, wave) > 2                     # reuse is another trajectory
    assert len(reports) >= 1 and sum(r.shape[1] for r in reports) == n_chunks
    for rep in reports:
        assert rep.shape[0] == 7 and rep.shape[2] == 2 and rep.dtype == np.float64
        assert not rep[1::2].any() and not rep[0, :, 0].any()                    # zeros where reused and for the first computed evaluation's drift
        assert (rep[0::2, :, 1] > 0).all() and (rep[2::2, :, 0] > 0).all()
    e2 = _engine(tmp, cfg_reuse=2)                                               # the report changes nothing
    w2, _ = e2.synthesize(LONG)
    assert e2.last_cfg_reuse_report == []
    e2.cleanup()
    assert np.array_equal(w2, wave)
    e3 = _engine(tmp, cfg_reuse=1)                                               # 1 is off: the bytes of the engine without the option
    w3, _ = e3.synthesize(LONG)
    e3.cleanup()
    assert np.array_equal(w3, base)


@pytest.mark.parametrize("fuse", [1, 2])
def test_engine_session_path(wave_k2, fuse):
    tmp, wave = wave_k2[:2]
    e = _engine(tmp, cfg_reuse=2, fuse_nfe=fuse)
    ref, txt = e.model_session_manager.select_sample()
    waves = e._synthesize_sessions(e._prepare_inputs(ref, txt, LONG))
    got = e.audio_processor.concatenate_with_crossfade_improved(waves, e.config.cross_fade_duration, e.config.sample_rate)
    e.cleanup()
    assert got.shape == wave.shape and _lsb(got, wave) <= 2, fuse


def test_engine_stream_path(wave_k2):
    tmp, wave = wave_k2[:2]
    e = _engine(tmp, cfg_reuse=2)
    got = np.concatenate(list(e.synthesize_stream(LONG, chunks_per_step=1)))
    e.cleanup()
    assert got.shape == wave.shape and _lsb(got, wave) <= 2


def test_batching_frontend_per_request_reuse(tmp_path):
    from vietvoice_tts_amd.batching import BatchingFrontend
    e = _engine(tmp_path)
    fe = BatchingFrontend(e, max_wait_ms=300.0, max_requests=8)
    text = "Xin chào các bạn, hôm nay thế nào?"
    try:
        alone = fe.submit(text, speed=1.0, serial=7, cfg_reuse=2).result(timeout=300)[0]
        default = fe.submit(text, speed=1.0, serial=7).result(timeout=300)[0]
        off = fe.submit(text, speed=1.0, serial=7, cfg_reuse=1).result(timeout=300)[0]
        n0 = fe.batches_run
        futs = [fe.submit("Tạm biệt và hẹn gặp lại.", speed=1.3, serial=8, gender="male", cfg_reuse=3, cfg_interval=(0.1, 0.9)),
                fe.submit(text, speed=1.0, serial=7, cfg_reuse=2),
                fe.submit(LONG, speed=0.8, serial=9, cfg_strength=0.0, cfg_reuse=2),
                fe.submit(LONG, speed=0.8, serial=10, apg_eta=0.5),              # projected guidance beside reuse: another request of the batch
                fe.submit(text, speed=1.0, serial=7)]
        outs = [f.result(timeout=300)[0] for f in futs]
        assert fe.batches_run == n0 + 1
        assert outs[1].shape == alone.shape and _lsb(outs[1], alone) <= 2
        assert outs[4].shape == default.shape and _lsb(outs[4], default) <= 2
        assert default.shape == alone.shape and _lsb(default, alone) > 2
        assert np.array_equal(off, default)
        with pytest.raises(ValueError, match="cfg_reuse must be an integer >= 1 or None"):
            fe.submit(text, cfg_reuse=0).result(timeout=5)
        with pytest.raises(ValueError, match="apg_eta"):
            fe.submit(text, cfg_reuse=2, apg_eta=0.5).result(timeout=5)
    finally:
        fe.close()
        e.cleanup()


def test_engine_edit_speech_with_reuse(tmp_path):
    from vietvoice_tts_amd.pack import MAX_POS
    from vietvoice_tts_amd.speech_edit import plan_edit
    e = _engine(tmp_path, cfg_reuse=2, cfg_reuse_report=True)
    e0 = _engine(tmp_path)
    sr = e.config.sample_rate
    clip, _ = e0.synthesize("Xin chào các bạn, hôm nay trời đẹp quá.")
    dur = clip.size / sr
    parts, fix, text = [(0.3 * dur, 0.5 * dur)], [0.3 * dur], "Xin chào các anh, hôm nay trời đẹp quá."
    out, _ = e.edit_speech(clip, text, parts, fix_duration=fix, seed=11)
    rep = e.last_cfg_reuse_report
    base, _ = e0.edit_speech(clip, text, parts, fix_duration=fix, seed=11)
    plan = plan_edit(clip.size, parts, fix, sr, e.config.hop_length, e.model_session_manager.spec.n_fft, MAX_POS)
    e.cleanup()
    e0.cleanup()
    assert out.dtype == np.int16 and out.size == plan.spliced_len
    assert base.shape == out.shape and _lsb(base, out) > 2
    assert len(rep) == 1 and rep[0].shape == (7, 1, 2) and not rep[0][1::2].any() and (rep[0][0::2, :, 1] > 0).all()
