"""-m gpu: N7, the Runge-Kutta solvers and the per-item guidance strength.

The stage kernel against float64 numpy; Euler bit-identical through every entry; each method against a reference solver written
here around ``Oracle.dit_forward`` (the oracle is evaluated at arbitrary times by assigning ``orc.t_grid``); the structure properties
(split calls, batch == alone, lanes, graph capture) bit for bit; the engine level; the error paths.  PARITY UNPINNED against
torchdiffeq (not available offline): the arithmetic of ISSUE / DESIGN N7 is the specification.  No test here claims a convergence
order or a quality gain on the synthetic model: its velocity field is too rough to show one."""
import ctypes as C

import numpy as np
import pytest
import torch

from tests.test_e2e_gpu import make_batch

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
LONG = "Hôm nay trời đẹp quá, chúng ta cùng nhau đi dạo quanh hồ nhé. " * 4
RAGGED = dict(a=[256 * 20, 256 * 12 + 100, 256 * 30], t=[30, 11, 47], g=[24, 9, 40])     # the batch of test_fp32_pipeline_matches_oracle
TOL = 1e-3            # max-abs state error in units of the reference's range: the bound test_e2e_gpu.py states for 7 Euler steps


def _mods():
    from vietvoice_tts_amd import runtime as rt
    from vietvoice_tts_amd.model_spec import ODE_METHODS, ode_plan
    return rt, ODE_METHODS, ode_plan


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
    return {k: (v.to(DEV) if torch.is_tensor(v) else v) for k, v in batch.items()}


def _pre(eng, d, host=True):
    lens = [int(v) for v in d["seq_len"].cpu()]
    return eng.preprocess(d["audio"], d["audio_len"], d["ids"], d["text_len"], d["seq_len"], d["N"], seq_len_host=lens if host else None)


def ref_solve(orc, pre, x, method, nfe_step, g):
    """The reference solver of N7 around the oracle, one item: x_i = x_n + h sum_j a_ij k_j, k_i = pc + (pc - pu) g at
    t_n + c_i h, x_{n+1} = x_n + h sum_j b_j k_j (sums over ascending j, zero coefficients skipped)."""
    _, _, ode_plan = _mods()
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
            pu = orc.dit_forward(xi, pre["cat_mel_text_drop"], ropes, 0)
            k.append(pc + (pc - pu) * g)
        for j in range(plan.s):
            if plan.b[j] != 0.0:
                x = x + (h * plan.b[j]) * k[j]
    return x


def ref_batch(orc, batch, method, nfe_step, gs):
    outs = []
    for b in range(batch["audio"].shape[0]):
        la, lt, sl = int(batch["audio_len"][b]), int(batch["text_len"][b]), int(batch["seq_len"][b])
        pre = orc.preprocess(batch["audio"][b, :la], batch["ids"][b, :lt], sl, batch["noise"][b, :sl])
        outs.append(ref_solve(orc, pre, pre["noise"], method, nfe_step, gs[b]))
    return outs


def _err(x, ref):
    return float((x - ref).abs().max()) / float(ref.abs().max())


# ------------------------------------------------------------------------------------------------ 1. the stage kernel
def _stage(eng, x, pred, ldp, Rc, M, n_prev, k_prev, coef, k_out, x_out, g, g_item, seq_n, row_src):
    rt, _, _ = _mods()
    a = rt.vv_ode_stage_args()
    a.x, a.pred, a.ldp, a.Rc, a.n_mel, a.n_prev = x.data_ptr(), pred.data_ptr(), ldp, Rc, M, n_prev
    for j in range(3):
        a.k_prev[j] = k_prev[j].data_ptr() if j < len(k_prev) and k_prev[j] is not None else None
    for j, v in enumerate(coef):
        a.coef[j] = v
    a.k_out = None if k_out is None else k_out.data_ptr()
    a.x_out = None if x_out is None else x_out.data_ptr()
    a.g, a.g_item, a.seq_n = g, None if g_item is None else g_item.data_ptr(), seq_n
    a.row_src = None if row_src is None else row_src.data_ptr()
    return eng.lib.vv_ode_stage(eng.ctx, C.byref(a), torch.cuda.current_stream().cuda_stream)


@pytest.mark.parametrize("per_item", [False, True])
@pytest.mark.parametrize("name", ["euler", "midpoint", "heun2", "heun3", "rk4"])
def test_ode_stage_against_float64(hip_tiny, name, per_item):
    """Every stage of every method on ragged rows.  Bound per element: 8 * 2^-24 * (|x| + sum_j |h a_ij| K_j), K = |pc| + |g| (|pc| +
    |pu|) for the fresh slope and |k_j| (which such a K_j bounds) for a stored one: a handful of fp32 roundings on terms of that
    size, the CFG difference included.  Derived, not measured."""
    _, ODE_METHODS, _ = _mods()
    eng = hip_tiny["f32"]
    a_t, b_t = ODE_METHODS[name]
    s = len(b_t)
    gen = torch.Generator().manual_seed(100 + s)
    B, N, M, ldp, h = 3, 40, 100, 128, 0.07
    lens = [40, 17, 29]
    row_src = torch.cat([b * N + torch.arange(n) for b, n in enumerate(lens)]).to(torch.int32)
    Rc = int(row_src.numel())
    g_sc = 2.0
    g_item = torch.tensor([2.0, -0.5, 3.5]) if per_item else None
    eps = 2.0 ** -24
    for i in range(s):
        last = i == s - 1
        coef = [np.float32(h * float(b_t[j] if last else a_t[i + 1][j])) for j in range(i + 1)]
        x = torch.randn(B * N, M, generator=gen)
        pred = torch.randn(2 * Rc, ldp, generator=gen)
        k_prev = [torch.randn(Rc, M, generator=gen) for _ in range(i)]
        dx, dp = x.clone().to(DEV), pred.to(DEV)
        dk = [k.to(DEV) if coef[j] != 0 else None for j, k in enumerate(k_prev)]        # a zero coefficient: no buffer at all
        k_out = torch.full((Rc, M), 7.0, device=DEV)
        x_out = None if last else torch.full((Rc, M), 7.0, device=DEV)
        rc = _stage(eng, dx, dp, ldp, Rc, M, i, dk, [float(c) for c in coef], k_out, x_out, g_sc,
                    None if g_item is None else g_item.to(DEV), N, row_src.to(DEV))
        assert rc == 0, eng.lib.vv_last_error(eng.ctx).decode()
        torch.cuda.synchronize()
        # float64 reference
        rs = row_src.long()
        gg = (g_item[rs // N].double()[:, None] if per_item else torch.tensor(g_sc, dtype=torch.float64))
        pc, pu = pred[:Rc, :M].double(), pred[Rc:, :M].double()
        k = pc + (pc - pu) * gg
        K = pc.abs() + gg.abs() * (pc.abs() + pu.abs())
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
        assert excess <= 0.0, (name, i, excess)
        assert float(((k_out.cpu().double() - k).abs() - 4 * eps * K).max()) <= 0.0, (name, i)
        # rows outside row_src are untouched; before the last stage x is not written at all
        mask = torch.ones(B * N, dtype=torch.bool)
        mask[rs] = False
        assert torch.equal(dx.cpu()[mask], x[mask])
        if not last:
            assert torch.equal(dx.cpu(), x)
    # the launcher refuses what the kernel cannot run
    x = torch.zeros(8, 100, device=DEV)
    pred = torch.zeros(16, 128, device=DEV)
    assert _stage(eng, x, pred, 128, 8, 100, 1, [None], [0.1, 0.1], None, None, 2.0, None, 0, None) == -22     # slope buffer missing
    assert _stage(eng, x, pred, 126, 8, 100, 0, [], [0.1], None, None, 2.0, None, 0, None) == -22             # ldp % 4
    assert _stage(eng, x, pred, 128, 8, 100, 0, [], [0.1], None, x, 2.0, None, 0, None) == -22                # x_out aliases x


# ------------------------------------------------------------------------------------------------ 2. Euler is unchanged
@pytest.mark.parametrize("dt", ["f32", "bf16"])
def test_euler_is_bit_identical_through_every_entry(own, tiny_setup, dt):
    spec = tiny_setup[0]
    eng = own[0][dt]
    d = _dev(make_batch(spec, RAGGED["a"], RAGGED["t"], RAGGED["g"], seed=3))
    lens = [int(v) for v in d["seq_len"].cpu()]
    host = (C.c_int32 * 3)(*lens)
    pre = _pre(eng, d)
    filled = torch.full((3,), float(spec.cfg_strength), dtype=torch.float32, device=DEV)
    outs = []
    for lanes in (1, 2):
        eng.set_option("lanes", lanes)
        eng.set_nfe(8, "euler")
        assert eng.ode_method == "euler" and eng.n_evals == eng.n_steps == 7
        x0 = d["noise"].clone()
        eng.transformer_steps(x0, pre, 0, 7)                               # vv_transformer_steps_h
        x1 = d["noise"].clone()
        eng._check(eng.lib.vv_transformer_steps(eng.ctx, 3, d["N"], d["seq_len"].data_ptr(), x1.data_ptr(), pre["cat_mel_text"].data_ptr(),
                                                pre["cat_mel_text_drop"].data_ptr(), pre["rope_cos_q"].data_ptr(), pre["rope_sin_q"].data_ptr(),
                                                pre["rope_cos_k"].data_ptr(), pre["rope_sin_k"].data_ptr(), 0, 7,
                                                torch.cuda.current_stream().cuda_stream))
        x2 = d["noise"].clone()
        eng.transformer_steps_ex(x2, pre, 0, 7, host, None)                # the struct entry, cfg = NULL
        x3 = d["noise"].clone()
        eng.transformer_steps_ex(x3, pre, 0, 7, None, None)                # ... lengths read back
        x4 = d["noise"].clone()
        eng.transformer_steps(x4, pre, 0, 7, cfg=filled)                   # the stage kernel with the model's strength per item
        torch.cuda.synchronize()
        for x in (x1, x2, x3, x4):
            assert torch.equal(x, x0), (dt, lanes)
        outs.append(x0)
    eng.set_option("lanes", 0)
    assert torch.equal(outs[0], outs[1])


def test_euler_workspace_is_unchanged_and_grows_with_the_stages(own, hip_tiny):
    """vv_transformer_ws_bytes: the Euler plan asks for what the shared (never re-planned) engine asks; s > 1 adds the stage state and
    the stored slopes, [Rc][n_mel] fp32 each, 256-byte aligned: midpoint 1 buffer, heun2 / heun3 2, rk4 4."""
    eng = own[0]["f32"]
    lens = [77, 30, 51]
    host = (C.c_int32 * 3)(*lens)

    def need(e):
        nb = C.c_uint64()
        e._check(e.lib.vv_transformer_ws_bytes(e.ctx, 3, 80, host, C.byref(nb)))
        return int(nb.value)
    eng.set_nfe(8, "euler")
    base = need(eng)
    assert base == need(hip_tiny["f32"])
    one = (sum(lens) * eng.spec.n_mel * 4 + 255) // 256 * 256
    for name, bufs in (("midpoint", 1), ("heun2", 2), ("heun3", 2), ("rk4", 4)):
        eng.set_nfe(8, name)
        assert need(eng) == base + bufs * one, name
    eng.set_nfe(8, "euler")
    assert need(eng) == base


# ------------------------------------------------------------------------------------------------ 3. / 4. against the oracle, fp32
@pytest.mark.parametrize("name,nfe", [("midpoint", 5), ("heun2", 5), ("heun3", 3), ("rk4", 3)])
def test_fp32_method_matches_reference_solver(own, tiny_setup, name, nfe):
    spec = tiny_setup[0]
    engs, orc = own
    eng = engs["f32"]
    batch = make_batch(spec, RAGGED["a"], RAGGED["t"], RAGGED["g"], seed=3)
    g = float(spec.cfg_strength)
    ref = ref_batch(orc, batch, name, nfe, [g] * 3)
    ref_euler = ref_batch(orc, batch, "euler", nfe, [g] * 3)
    others = {"heun3": "rk4", "rk4": "heun3"}
    ref_other = ref_batch(orc, batch, others[name], nfe, [g] * 3) if name in others else None
    d = _dev(batch)
    eng.set_nfe(nfe, name)
    assert eng.ode_method == name and eng.n_steps == nfe - 1 and eng.n_evals == (nfe - 1) * len(_mods()[1][name][1])
    x = d["noise"].clone()
    eng.transformer_steps(x, _pre(eng, d), 0, eng.n_steps)
    torch.cuda.synchronize()
    x = x.cpu()
    for b, r in enumerate(ref):
        sl = int(batch["seq_len"][b])
        err, apart = _err(x[b, :sl], r), _err(ref_euler[b], r)
        print(f"{name} nfe {nfe} item {b}: err {err:.3e} of range; reference vs euler on the same grid {apart:.3e}")
        # on the reference side alone: the method is distinguishable from Euler (and heun3 from rk4) far beyond the tolerance,
        # so a solver that silently ran another method fails
        assert apart > 10 * TOL, (name, b, apart)
        if ref_other is not None:
            assert _err(ref_other[b], r) > 10 * TOL, (name, b)
        assert err < TOL, (name, b, err)


def test_fp32_per_item_strength_matches_reference_solver(own, tiny_setup):
    spec = tiny_setup[0]
    engs, orc = own
    eng = engs["f32"]
    batch = make_batch(spec, RAGGED["a"], RAGGED["t"], RAGGED["g"], seed=3)
    gs = [2.0, 1.0, 3.5]
    ref = ref_batch(orc, batch, "midpoint", 5, gs)
    ref_same = ref_batch(orc, batch, "midpoint", 5, [2.0] * 3)
    d = _dev(batch)
    eng.set_nfe(5, "midpoint")
    pre = _pre(eng, d)
    x = d["noise"].clone()
    eng.transformer_steps(x, pre, 0, eng.n_steps, cfg=torch.tensor(gs, dtype=torch.float32, device=DEV))
    x2 = d["noise"].clone()
    eng.transformer_steps(x2, pre, 0, eng.n_steps)                          # the model's strength (2.0) for every item
    torch.cuda.synchronize()
    x, x2 = x.cpu(), x2.cpu()
    for b, r in enumerate(ref):
        sl = int(batch["seq_len"][b])
        err = _err(x[b, :sl], r)
        print(f"per-item strength {gs[b]} item {b}: err {err:.3e} of range")
        assert err < TOL, (b, err)
    sl = int(batch["seq_len"][1])
    apart_ref, apart_hip = _err(ref_same[1], ref[1]), _err(x2[1, :sl], x[1, :sl])
    print(f"item 1 at g = 1.0 vs g = 2.0: reference {apart_ref:.3e}, device {apart_hip:.3e} of range")
    assert apart_ref > 10 * TOL and apart_hip > 10 * TOL
    assert torch.equal(x[0], x2[0])                                          # item 0 keeps the model's strength: the same bits


# ------------------------------------------------------------------------------------------------ 5. bf16
BF16_EULER8_RMSE = 3.87e-3     # measured on the Euler path, which this change leaves bit-identical: see the docstring below


def test_bf16_midpoint_close_to_reference_solver(own, tiny_setup):
    """bf16 midpoint on a 5-point grid (8 evaluations), the 2-item batch of test_bf16_pipeline_close_to_oracle, state RMSE relative to
    the state RMS against the reference solver on the fp32 oracle.  Bound: 1.5 x the RMSE of bf16 EULER with the same 8 evaluations
    (9-point grid) against the fp32 oracle on this batch, and the project's 2e-2 class bound.  The margin is for the different
    trajectory, not for the stage kernel, which is fp32.
    Measured on the MI355X (profiles/ode/notes.md), RMSE / RMS per item: bf16 Euler, 8 steps 3.875e-3 and 3.892e-3 (the constant is
    the smaller one, rounded down); bf16 midpoint, 4 steps 4.156e-3 and 4.157e-3, 1.07x the Euler figure."""
    spec = tiny_setup[0]
    engs, orc = own
    eng = engs["bf16"]
    batch = make_batch(spec, [256 * 20, 256 * 14], [30, 21], [24, 17], seed=5)
    g = float(spec.cfg_strength)
    ref_mid = ref_batch(orc, batch, "midpoint", 5, [g] * 2)
    ref_eul = ref_batch(orc, batch, "euler", 9, [g] * 2)
    d = _dev(batch)
    rel = lambda x, r: float((x - r).pow(2).mean().sqrt() / r.pow(2).mean().sqrt())
    res = {}
    for name, nfe, ref in (("euler", 9, ref_eul), ("midpoint", 5, ref_mid)):
        eng.set_nfe(nfe, name)
        assert eng.n_evals == 8
        x = d["noise"].clone()
        eng.transformer_steps(x, _pre(eng, d), 0, eng.n_steps)
        torch.cuda.synchronize()
        res[name] = [rel(x[b, : int(batch["seq_len"][b])].cpu(), r) for b, r in enumerate(ref)]
        print(f"bf16 {name} ({nfe}-point grid, 8 evaluations): state RMSE / RMS per item {['%.3e' % v for v in res[name]]}")
    for v in res["midpoint"]:
        assert v < 1.5 * BF16_EULER8_RMSE and v < 2e-2, res


# ------------------------------------------------------------------------------------------------ 6. structure, bit for bit
def test_split_calls_and_batch_equals_alone(own, tiny_setup):
    spec = tiny_setup[0]
    eng = own[0]["f32"]
    batch = make_batch(spec, RAGGED["a"], RAGGED["t"], RAGGED["g"], seed=11)
    d = _dev(batch)
    cfg = torch.tensor([2.0, 0.75, 3.25], dtype=torch.float32, device=DEV)
    for name in ("rk4", "heun3"):
        eng.set_nfe(5, name)
        pre = _pre(eng, d)
        x1 = d["noise"].clone()
        eng.transformer_steps(x1, pre, 0, 4, cfg=cfg)
        x2 = d["noise"].clone()
        eng.transformer_steps(x2, pre, 0, 2, cfg=cfg)
        eng.transformer_steps(x2, pre, 2, 2, cfg=cfg)
        torch.cuda.synchronize()
        assert torch.equal(x1, x2), name
        for b in range(3):                                                   # each item alone, with its own strength
            sl, la, lt = int(batch["seq_len"][b]), int(batch["audio_len"][b]), int(batch["text_len"][b])
            one = dict(audio=d["audio"][b: b + 1, :max(la, spec.n_fft)].contiguous(), audio_len=d["audio_len"][b: b + 1].contiguous(),
                       ids=d["ids"][b: b + 1, :lt].contiguous(), text_len=d["text_len"][b: b + 1].contiguous(),
                       seq_len=d["seq_len"][b: b + 1].contiguous(), N=sl)
            xa = d["noise"][b: b + 1, :sl].contiguous().clone()
            eng.transformer_steps(xa, _pre(eng, one), 0, 4, cfg=cfg[b: b + 1].contiguous())
            torch.cuda.synchronize()
            assert torch.equal(xa[0], x1[b, :sl]), (name, b)


@pytest.mark.parametrize("dt", ["f32", "bf16"])
def test_lanes_are_bit_identical(own, tiny_setup, dt):
    """Option "lanes" 1 == 2: one item (its two CFG branches are the lanes, forked and joined once per EVALUATION) and a ragged batch
    of three with distinct strengths (item lanes with their own stage buffers)."""
    spec = tiny_setup[0]
    eng = own[0][dt]
    cases = [(([256 * 26], [41], [33]), None), ((RAGGED["a"], RAGGED["t"], RAGGED["g"]), [2.0, 0.5, 3.0])]
    try:
        for name in ("rk4", "midpoint"):
            eng.set_nfe(4, name)
            for (la, lt, gf), gs in cases:
                d = _dev(make_batch(spec, la, lt, gf, seed=20 + len(la)))
                pre = _pre(eng, d)
                cfg = None if gs is None else torch.tensor(gs, dtype=torch.float32, device=DEV)
                xs = []
                for lanes in (1, 2):
                    eng.set_option("lanes", lanes)
                    x = d["noise"].clone()
                    eng.transformer_steps(x, pre, 0, eng.n_steps, cfg=cfg)
                    xs.append(x)
                torch.cuda.synchronize()
                assert torch.equal(xs[0], xs[1]), (dt, name, len(la))
    finally:
        eng.set_option("lanes", 0)


def test_graph_capture_under_rk4_and_staleness(own, tiny_setup):
    spec = tiny_setup[0]
    eng = own[0]["f32"]
    batch = make_batch(spec, RAGGED["a"], RAGGED["t"], RAGGED["g"], seed=13)
    d = _dev(batch)
    lens = [int(v) for v in batch["seq_len"]]
    eng.set_nfe(4, "euler")
    pre = _pre(eng, d)
    g_euler = eng.capture_steps(3, d["N"], lens, batch["t_gen_max"])
    assert not g_euler.stale()
    eng.set_nfe(4, "rk4")                                                    # the same grid, another solver: the tables moved
    assert g_euler.stale()
    with pytest.raises(RuntimeError, match="stale"):
        g_euler(d["noise"], pre)
    x_e = d["noise"].clone()
    eng.transformer_steps(x_e, pre, 0, eng.n_steps)
    pcm_e, len_e = eng.decode(x_e, pre, batch["t_gen_max"])
    graph = eng.capture_steps(3, d["N"], lens, batch["t_gen_max"])           # sized with the plan in force
    x_g, pcm_g, len_g = graph(d["noise"], pre)
    torch.cuda.synchronize()
    assert torch.equal(x_g, x_e) and torch.equal(pcm_g, pcm_e) and torch.equal(len_g, len_e)
    eng.set_nfe(4, "rk4")                                                    # the same pair: nothing changes, the graph stays valid
    assert not graph.stale()


# ------------------------------------------------------------------------------------------------ 7. engine level
def _engine(tmp, **kw):
    from vietvoice_tts_amd.core import ModelConfig, TTSEngine
    cfg = ModelConfig(model_cache_dir=str(tmp), synthetic_model=True, model_spec="tiny", nfe_step=5, acoustic_dtype="fp32",
                      max_chunk_duration=8.0, **kw)
    return TTSEngine(cfg)


def _lsb(a, b):
    return int(np.abs(a.astype(np.int32) - b.astype(np.int32)).max())


def test_engine_midpoint_device_session_and_stream_paths(tmp_path):
    e1 = _engine(tmp_path, ode_method="midpoint")
    assert e1.model_session_manager.engine.ode_method == "midpoint" and e1.model_session_manager.engine.n_evals == 8
    wave_dev, _ = e1.synthesize(LONG)
    assert len(e1._last_plan) > 1
    e1.cleanup()
    for fuse in (1, 2):                        # the session path: one (or two) ODE steps per session.run, never a split step
        e2 = _engine(tmp_path, ode_method="midpoint", fuse_nfe=fuse)
        ref, txt = e2.model_session_manager.select_sample()
        waves = e2._synthesize_sessions(e2._prepare_inputs(ref, txt, LONG))
        wave_ses = e2.audio_processor.concatenate_with_crossfade_improved(waves, e2.config.cross_fade_duration, e2.config.sample_rate)
        e2.cleanup()
        assert wave_ses.shape == wave_dev.shape and _lsb(wave_ses, wave_dev) <= 2, fuse
    e3 = _engine(tmp_path)                     # the Euler engine, same seed: another trajectory
    wave_euler, _ = e3.synthesize(LONG)
    e3.cleanup()
    assert wave_euler.shape == wave_dev.shape and _lsb(wave_euler, wave_dev) > 2
    e4 = _engine(tmp_path, ode_method="midpoint")
    got = np.concatenate(list(e4.synthesize_stream(LONG, chunks_per_step=1)))
    e4.cleanup()
    assert got.shape == wave_dev.shape and _lsb(got, wave_dev) <= 2


def test_engine_config_strength_reaches_both_paths(tmp_path):
    """ModelConfig.cfg_strength: the device path and the session path agree (<= 2 LSB), and differ from the model's strength."""
    text = "Xin chào các bạn, hôm nay thế nào?"
    e1 = _engine(tmp_path, ode_method="heun2", cfg_strength=1.0)
    dev, _ = e1.synthesize(text)
    e1.cleanup()
    e2 = _engine(tmp_path, ode_method="heun2", cfg_strength=1.0)
    ref, txt = e2.model_session_manager.select_sample()
    ses = e2._synthesize_sessions(e2._prepare_inputs(ref, txt, text))[0].reshape(-1)
    e2.cleanup()
    e3 = _engine(tmp_path, ode_method="heun2")
    base, _ = e3.synthesize(text)
    e3.cleanup()
    assert ses.shape == dev.shape and _lsb(ses, dev) <= 2
    assert base.shape == dev.shape and _lsb(base, dev) > 2


def test_engine_edit_speech_under_midpoint(tmp_path, own, tiny_setup):
    from vietvoice_tts_amd.pack import MAX_POS
    from vietvoice_tts_amd.speech_edit import plan_edit
    e = _engine(tmp_path, ode_method="midpoint")
    sr = e.config.sample_rate
    clip, _ = e.synthesize("Xin chào các bạn, hôm nay trời đẹp quá.")
    dur = clip.size / sr
    parts, fix, text = [(0.3 * dur, 0.5 * dur)], [0.3 * dur], "Xin chào các anh, hôm nay trời đẹp quá."
    out, _ = e.edit_speech(clip, text, parts, fix_duration=fix, seed=11)
    plan = plan_edit(clip.size, parts, fix, sr, e.config.hop_length, e.model_session_manager.spec.n_fft, MAX_POS)
    assert out.dtype == np.int16 and out.size == plan.spliced_len
    assert e.model_session_manager.engine.ode_method == "midpoint"
    e.cleanup()
    # HipSynth.edit_batch under midpoint with a per-item strength: the kept frames are the conditioning's mel, bit for bit
    from tests.test_speech_edit_gpu import HOP, TWO, dev_args, make_edits
    spec = tiny_setup[0]
    eng = own[0]["f32"]
    eng.set_nfe(5, "midpoint")
    ed = make_edits(spec, TWO, seed=5)
    src, rows, L, ids, tl, keep = dev_args(ed)
    x, pcm, pcm_len = eng.edit_batch(src, rows, L, ids, tl, keep, ed["noise"].to(DEV), cfg=torch.tensor([1.5, 2.5], device=DEV))
    mal = max(max(L), spec.n_fft)
    frames = [v // HOP + 1 for v in L]
    i32 = lambda v: torch.tensor(v, dtype=torch.int32, device=DEV)
    pre = eng.preprocess_edit(eng.edit_splice(src, rows, len(L), (mal + 3) // 4 * 4), i32(L), ids, tl, i32(frames), ed["N"], keep, L,
                              max_audio_len=mal, seq_len_host=frames)
    torch.cuda.synchronize()
    for b, Lb in enumerate(L):
        n = Lb // HOP + 1
        k = torch.from_numpy(ed["keep"][b, :n].astype(bool))
        assert 0 < int(k.sum()) < n and int(pcm_len[b]) == Lb
        assert torch.equal(x[b, :n].cpu()[k], pre["cat_mel_text"][b, :n, : spec.n_mel].cpu()[k])
        assert not torch.equal(x[b, :n].cpu()[~k], ed["noise"][b, :n][~k])


def test_batching_frontend_per_request_strength(tmp_path):
    """A request with cfg_strength = 1.0 alone and inside a batch with two requests of other strengths: <= 2 LSB (the bound of
    test_batching_frontend_batch_composition_invariance), and not the audio of the same request at the default strength."""
    from vietvoice_tts_amd.batching import BatchingFrontend
    e = _engine(tmp_path, ode_method="midpoint")
    fe = BatchingFrontend(e, max_wait_ms=300.0, max_requests=8)
    text = "Xin chào các bạn, hôm nay thế nào?"
    try:
        alone = fe.submit(text, speed=1.0, serial=7, cfg_strength=1.0).result(timeout=300)[0]
        default = fe.submit(text, speed=1.0, serial=7).result(timeout=300)[0]
        n0 = fe.batches_run
        futs = [fe.submit("Tạm biệt và hẹn gặp lại.", speed=1.3, serial=8, gender="male", cfg_strength=3.0),
                fe.submit(text, speed=1.0, serial=7, cfg_strength=1.0),
                fe.submit(LONG, speed=0.8, serial=9)]
        outs = [f.result(timeout=300)[0] for f in futs]
        assert fe.batches_run == n0 + 1
        assert outs[1].shape == alone.shape and _lsb(outs[1], alone) <= 2
        assert default.shape == alone.shape and _lsb(default, alone) > 2
    finally:
        fe.close()
        e.cleanup()


# ------------------------------------------------------------------------------------------------ 8. errors
def test_plan_and_step_range_errors_leave_the_plan_in_force(own, tiny_setup):
    rt, ODE_METHODS, ode_plan = _mods()
    from vietvoice_tts_amd import pack
    spec = tiny_setup[0]
    eng = own[0]["f32"]
    eng.set_nfe(5, "midpoint")
    d = _dev(make_batch(spec, [256 * 16], [20], [12], seed=8))
    pre = _pre(eng, d)
    x0 = d["noise"].clone()
    eng.transformer_steps(x0, pre, 0, eng.n_steps)
    st = torch.cuda.current_stream().cuda_stream

    def set_plan(n_steps, a, b):
        s = len(b)
        sinus = torch.zeros(n_steps * s, spec.time_freq_dim)
        dt = torch.full((n_steps,), 1.0 / n_steps)
        aa = (C.c_double * (s * s))(*[float(v) for r in a for v in r])
        bb = (C.c_double * s)(*[float(v) for v in b])
        return eng.lib.vv_set_ode_plan(eng.ctx, sinus.data_ptr(), dt.data_ptr(), n_steps, s, aa, bb, st)
    assert set_plan(4, [[0, 0.5], [0.5, 0]], [0, 1]) == -22                    # not strictly lower triangular
    assert "triangular" in eng.lib.vv_last_error(eng.ctx).decode()
    assert set_plan(4, [[0.1, 0], [0.5, 0]], [0, 1]) == -22                    # a diagonal entry
    assert set_plan(4, [[0, 0], [0.5, 0]], [0.5, 0.6]) == -22                  # sum b != 1
    assert set_plan(4, [[0] * 5 for _ in range(5)], [1, 0, 0, 0, 0]) == -22    # s = 5
    assert set_plan(4, [[0, 0], [float("inf"), 0]], [0, 1]) == -22             # not finite
    assert set_plan(200, ODE_METHODS["heun3"][0], ODE_METHODS["heun3"][1]) == -22   # 600 evaluations > 512
    with pytest.raises(ValueError):
        eng.set_nfe(200, "rk4")
    assert (eng.nfe_step, eng.ode_method) == (5, "midpoint")
    # a step range outside the plan
    a = rt.vv_steps_args()
    x = d["noise"].clone()
    a.B, a.N, a.seq_len, a.x = 1, d["N"], pre["seq_len"].data_ptr(), x.data_ptr()
    a.cat_mel_text, a.cat_mel_text_drop = pre["cat_mel_text"].data_ptr(), pre["cat_mel_text_drop"].data_ptr()
    a.rope_cos_q, a.rope_sin_q, a.rope_cos_k, a.rope_sin_k = (pre[k].data_ptr() for k in ("rope_cos_q", "rope_sin_q", "rope_cos_k", "rope_sin_k"))
    a.step0, a.n_steps = 2, 3                                                  # the plan has 4 steps
    assert eng.lib.vv_transformer_steps_ex(eng.ctx, C.byref(a), st) == -22
    a.step0, a.n_steps = 0, 5
    assert eng.lib.vv_transformer_steps_ex(eng.ctx, C.byref(a), st) == -22
    assert eng.lib.vv_transformer_steps_ex(eng.ctx, None, st) == -22
    torch.cuda.synchronize()
    assert torch.equal(x, d["noise"])                                          # nothing ran
    # the previous plan is still in force: the same bits as before the refused calls
    x1 = d["noise"].clone()
    eng.transformer_steps(x1, pre, 0, eng.n_steps)
    torch.cuda.synchronize()
    assert torch.equal(x1, x0)
    # a custom tableau (Ralston's second-order method) runs through the same path
    eng.set_nfe(5, (((0, 0), (2 / 3, 0)), (0.25, 0.75)))
    assert eng.n_evals == 8
    x2 = d["noise"].clone()
    eng.transformer_steps(x2, pre, 0, eng.n_steps)
    torch.cuda.synchronize()
    assert bool(torch.isfinite(x2).all()) and not torch.equal(x2, x0)
