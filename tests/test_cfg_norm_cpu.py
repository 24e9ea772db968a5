"""CFG-Zero* / guidance rescale / zero-init without a GPU: the rule by hand in rationals, the truncated plan of zero-init,
the checks and refusals of ModelConfig, RequestOptions and BatchingFrontend.submit, the header against the binding, the numpy mirror of
the device's sums against extended precision under the derived bound, and -- before the device file fixes its inputs -- that the rule
moves the float64 reference of every guided item of the ragged three by more than sampler_util.MATTERS parity bounds."""
import ctypes as C
import math
import os
import re
from fractions import Fraction as F
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from tests import cfg_norm_util as U

HERE = os.path.dirname(os.path.abspath(__file__))
METHODS = ("euler", "midpoint", "heun2", "heun3", "rk4", "ab2", "ab3")
SWAY = -1.0


# ------------------------------------------------------------------------------------------------ 1. the rule by hand
PC = [F(1), F(-2), F(3), F(1, 2)]
PU = [F(2), F(1), F(-1), F(3)]


def test_star_off_and_phi_zero_is_plain_cfg():
    for g in (F(0), F(2), F(-1, 2)):
        r = U.rule_exact(PC, PU, g, star=False, phi=0)
        assert r["s"] == 1 and r["f_of_rho"](F(7, 3)) == 1                     # phi = 0: f is exactly 1 whatever rho
        assert r["k0"] == [c + (c - u) * g for c, u in zip(PC, PU)]


def test_by_hand_on_four_elements():
    # S_cu = 2 - 2 - 3 + 3/2 = -3/2, S_uu = 4 + 1 + 1 + 9 = 15: s = -1/10
    r = U.rule_exact(PC, PU, F(2), star=True, phi=1)
    assert r["s"] == F(-1, 10)
    assert r["k0"] == [c + (c + u / 10) * 2 for c, u in zip(PC, PU)]
    assert r["var_k"] == U.variance(r["k0"])                                    # a^2 V_cc + 2 a c V_cu + c^2 V_uu IS the variance of k0
    assert r["V_cc"] == U.variance(PC)


@pytest.mark.parametrize("lam", [F(1, 2), F(3), F(-2)])
@pytest.mark.parametrize("g", [F(0), F(2), F(7, 2)])
def test_parallel_predictions_give_the_conditional_one(lam, g):
    pu = [lam * c for c in PC]
    r = U.rule_exact(PC, pu, g, star=True, phi=0)
    assert r["s"] == 1 / lam and r["k0"] == PC


@pytest.mark.parametrize("star", [False, True])
def test_full_rescale_restores_the_conditional_std(star):
    r = U.rule_exact(PC, PU, F(3), star=star, phi=1)
    # f = rho at phi = 1: var(f k0) = rho^2 var(k0) = V_cc
    assert r["f_of_rho"](F(5, 7)) == F(5, 7)
    assert r["rho2"] * U.variance(r["k0"]) == U.variance(PC)


def test_degenerate_sums_fall_back_to_one():
    r = U.rule_exact(PC, [F(0)] * 4, F(2), star=True, phi=1)
    assert r["s"] == 1                                                          # S_uu == 0
    flat = [F(5)] * 4
    r = U.rule_exact(flat, flat, F(2), star=False, phi=1)
    assert r["var_k"] == 0 and r["rho2"] == 1                                   # var_k == 0 (and V_cc == 0)
    s, f = U.coef_from_sums([0.0, 0.0, 30.0, 0.0, 0.0], 4, 2.0, True, 1.0)
    assert float(s) == 1.0 and f == np.float32(1.0 / 3.0)                       # S_uu == 0 in the float64 formula: s = 1, rho = sqrt(7.5 / 67.5)
    s, f = U.coef_from_sums([100.0, 100.0, 100.0, 20.0, 20.0], 4, 2.0, False, 0.7)      # every element 5: all variances 0
    assert (float(s), float(f)) == (1.0, 1.0)


def test_float64_rule_agrees_with_the_rationals():
    pc, pu = np.array([float(v) for v in PC]), np.array([float(v) for v in PU])
    s, f, k = U.rule64(pc.reshape(1, 4), pu.reshape(1, 4), 2.0, True, 0.7)
    r = U.rule_exact(PC, PU, F(2), True, F(7, 10))
    rho = math.sqrt(float(r["rho2"]))
    assert abs(float(s) - float(r["s"])) <= 2.0 ** -24 * abs(float(r["s"]))
    assert abs(float(f) - (0.7 * rho + 0.3)) <= 2.0 ** -23
    want = np.array([float(f) * float(c + (c - F(float(s)) * u) * 2) for c, u in zip(PC, PU)])
    assert np.allclose(k.ravel(), want, rtol=1e-15, atol=0)


# ------------------------------------------------------------------------------------------------ 2. the mirror of the device's sums
@pytest.mark.parametrize("frames,n_mel", [(1, 4), (31, 100), (32, 100), (33, 100), (97, 100), (45, 4)])
def test_mirror_sums_lie_within_the_derived_bound_of_extended_precision(frames, n_mel):
    rng = np.random.default_rng(frames * 131 + n_mel)
    pc = rng.standard_normal((frames, n_mel)).astype(np.float32)
    pu = (0.6 * pc + 0.5 * rng.standard_normal((frames, n_mel))).astype(np.float32)
    parts, tot = U.gram_mirror(pc, pu)
    assert parts.shape == (-(-frames // 32), 5)
    S, T = U.sums64(pc, pu)
    gam = U.chain(frames, n_mel) * U.EPS53
    assert np.all(np.abs(tot - S) <= gam * T + 1e-300)
    for g, star, phi in ((2.0, True, None), (3.0, False, 0.7), (2.0, True, 1.0)):
        s, f, bs, bf = U.coef_exact(pc, pu, g, star, phi)
        sm, fm = U.coef_from_sums(tot, pc.size, g, star, phi)
        assert abs(float(sm) - float(s)) <= bs and abs(float(fm) - float(f)) <= bf
        assert bs <= 4 * U.EPS24 * max(abs(float(s)), 1.0) and bf <= 4 * U.EPS24 * max(abs(float(f)), 1.0)      # the bound is about one fp32 rounding


# ------------------------------------------------------------------------------------------------ 3. zero-init: the plan
def _restated(nfe, sway, method):
    """ode_plan as it was before ``skip`` existed, restated: the grid, the steps and the evaluation times in float64, cast once."""
    from vietvoice_tts_amd.model_spec import ODE_METHODS, ODE_MULTISTEP, multistep_weights
    t = torch.linspace(0.0, 1.0, nfe, dtype=torch.float64)
    t = t + sway * (torch.cos(math.pi / 2 * t) - 1.0 + t)
    dt = t[1:] - t[:-1]
    multi = method in ODE_MULTISTEP
    a, b = ODE_METHODS["euler" if multi else method]
    a, b = tuple(tuple(float(v) for v in r) for r in a), tuple(float(v) for v in b)
    c = torch.tensor([sum(r) for r in a], dtype=torch.float64)
    te = t[:-1, None] + c[None, :] * dt[:, None]
    if len(b) > 1:
        te = te.clamp(0.0, 1.0)
    beta = multistep_weights(t, ODE_MULTISTEP[method]) if multi else None
    return t, te.reshape(-1).to(torch.float32), dt.to(torch.float32), a, b, beta


@pytest.mark.parametrize("method", METHODS)
def test_skip_zero_is_todays_plan_bit_for_bit(method):
    from vietvoice_tts_amd.model_spec import ode_plan
    for nfe in (2, 3, 8, 32):
        _, te, dt, a, b, beta = _restated(nfe, SWAY, method)
        for p in (ode_plan(nfe, SWAY, method), ode_plan(nfe, SWAY, method, skip=0), ode_plan(nfe, SWAY, method, 0)):
            assert torch.equal(p.t, te) and torch.equal(p.dt, dt) and p.t.dtype == torch.float32
            assert p.a == a and p.b == b and p.s == len(b) and p.beta == beta


@pytest.mark.parametrize("method", METHODS)
@pytest.mark.parametrize("K", [1, 2, 6])
def test_skip_takes_the_rows_of_the_full_plan_from_step_K(method, K):
    from vietvoice_tts_amd.model_spec import ODE_MULTISTEP, multistep_weights, ode_plan
    nfe = 8
    full, cut = ode_plan(nfe, SWAY, method), ode_plan(nfe, SWAY, method, skip=K)
    s = full.s
    assert int(cut.dt.numel()) == nfe - 1 - K and torch.equal(cut.dt, full.dt[K:]) and torch.equal(cut.t, full.t[K * s:])
    assert (cut.a, cut.b, cut.s) == (full.a, full.b, full.s)
    if method in ODE_MULTISTEP:
        q = ODE_MULTISTEP[method]
        grid = _restated(nfe, SWAY, method)[0]
        assert cut.beta == multistep_weights(grid[K:], q)                       # the weights of the grid points from K on
        assert cut.beta[0] == (1.0,) + (0.0,) * (q - 1)                         # the ramp restarts: the first step that exists is an Euler step
        if len(cut.beta) > 1:
            assert cut.beta[1][1] != 0.0 and all(v == 0.0 for v in cut.beta[1][2:])
            assert cut.beta[1] != full.beta[K + 1] or q == 2                    # ... and is not the full plan's row (ab3: that one has three terms)
        if q == 3 and len(cut.beta) > 2:
            assert cut.beta[2] == full.beta[K + 2]                              # from the third step on the same nodes, the same weights
    else:
        assert cut.beta is None


def _solve64(plan, f, x, t64):
    """A float64 solver on a plan: Runge-Kutta by the tableau, or Adams-Bashforth in Newton form on the float64 grid ``t64`` of its steps."""
    from tests.sampler_util import _ab_step
    n, s = int(plan.dt.numel()), plan.s
    if plan.beta is not None:
        q, hist = len(plan.beta[0]), []
        for st in range(n):
            hist.append(f(float(np.float32(t64[st])), x))
            x = _ab_step(x, t64, st, hist, min(q, st + 1))
            hist = hist[-3:]
        return x
    for st in range(n):
        h, ks = float(plan.dt[st]), []
        for i in range(s):
            xi = x
            for j in range(i):
                if plan.a[i][j] != 0.0:
                    xi = xi + (h * plan.a[i][j]) * ks[j]
            ks.append(f(float(plan.t[st * s + i]), xi))
        for j in range(s):
            if plan.b[j] != 0.0:
                x = x + (h * plan.b[j]) * ks[j]
    return x


@pytest.mark.parametrize("method", METHODS)
@pytest.mark.parametrize("K", [1, 3])
def test_skip_equals_integrating_from_t_K(method, K):
    """The truncated plan from the start noise = the float64 solver started at (t_K, noise) on the grid points K ... n - 1: for a
    Runge-Kutta method the steps K ... of the full plan, for Adams-Bashforth a fresh start at t_K."""
    from tests.sampler_util import grid64
    from vietvoice_tts_amd.model_spec import OdePlan, ode_plan
    nfe = 9
    f = lambda t, x: np.cos(3.0 * t) * x + np.sin(x) * t - 0.25
    x0 = np.array([0.3, -1.2, 2.0])
    g64 = grid64(nfe, SWAY)
    cut = ode_plan(nfe, SWAY, method, skip=K)
    got = _solve64(cut, f, x0, g64[K:])
    # the same integration written from the grid alone: points t_K ... t_{n-1}, the method's own rows recomputed on them
    _, te, dt, a, b, beta = _restated(nfe, SWAY, method)
    s = len(b)
    from vietvoice_tts_amd.model_spec import ODE_MULTISTEP, multistep_weights
    tail_beta = multistep_weights(torch.from_numpy(g64[K:]), ODE_MULTISTEP[method]) if method in ODE_MULTISTEP else None
    want = _solve64(OdePlan(te[K * s:], dt[K:], a, b, s, tail_beta), f, x0, g64[K:])
    assert np.array_equal(got, want)
    full = _solve64(ode_plan(nfe, SWAY, method), f, x0, g64)
    assert not np.array_equal(got, full)                                        # and it is not the full integration


def test_check_cfg_zero_init():
    from vietvoice_tts_amd.model_spec import check_cfg_zero_init, ode_plan
    assert [check_cfg_zero_init(k, 8) for k in (0, 1, 6)] == [0, 1, 6]
    assert check_cfg_zero_init(0, 2) == 0 and check_cfg_zero_init(np.int64(3), 8) == 3
    for bad in (-1, 7, 8, 100):
        with pytest.raises(ValueError, match="cfg_zero_init must satisfy 0 <= K <= nfe_step - 2"):
            check_cfg_zero_init(bad, 8)
    for bad in (True, 1.0, "1", None):
        with pytest.raises(ValueError, match="cfg_zero_init must be an integer"):
            check_cfg_zero_init(bad, 8)
    with pytest.raises(ValueError, match="cfg_zero_init"):
        ode_plan(8, SWAY, "euler", skip=7)
    assert int(ode_plan(8, SWAY, "rk4", skip=6).dt.numel()) == 1


# ------------------------------------------------------------------------------------------------ 4. config, options, front end
def test_check_cfg_norm():
    from vietvoice_tts_amd.model_spec import check_cfg_norm
    assert check_cfg_norm(None, None) is None and check_cfg_norm(False, None) is None
    assert check_cfg_norm(True, None) == (True, 0.0) and check_cfg_norm(False, 0.7) == (False, 0.7) and check_cfg_norm(None, 1) == (False, 1.0)
    for bad in (0, 0.0, -0.1, 1.0001, math.nan, math.inf):
        with pytest.raises(ValueError, match="cfg_rescale must satisfy 0 < phi <= 1"):
            check_cfg_norm(None, bad)
    for bad in (True, "0.5"):
        with pytest.raises(ValueError, match="cfg_rescale must be a number or None"):
            check_cfg_norm(None, bad)
    for bad in (1, 0, "yes", 1.0):
        with pytest.raises(ValueError, match="cfg_zero_star must be a bool or None"):
            check_cfg_norm(bad, None)


REFUSALS = [(dict(apg_eta=0.5), "apg_eta / apg_norm"), (dict(apg_norm=2.0), "apg_eta / apg_norm"), (dict(cfg_reuse=2), "cfg_reuse > 1")]
ON = [dict(cfg_zero_star=True), dict(cfg_rescale=0.7), dict(cfg_zero_star=True, cfg_rescale=1.0)]


def test_model_config_fields(tmp_path):
    import json
    from vietvoice_tts_amd.core import ModelConfig
    kw = dict(model_cache_dir=str(tmp_path), synthetic_model=True, model_spec="tiny")
    cfg = ModelConfig(**kw)
    assert cfg.cfg_zero_star is False and cfg.cfg_rescale is None and cfg.cfg_zero_init == 0 and cfg.cfg_norm_report is False
    cfg = ModelConfig(cfg_zero_star=True, cfg_rescale=1, cfg_zero_init=2, cfg_norm_report=True, cfg_interval=(0.1, 0.9), cfg_strength=3.0, **kw)
    assert cfg.cfg_zero_star is True and cfg.cfg_rescale == 1.0 and type(cfg.cfg_rescale) is float and cfg.cfg_zero_init == 2
    d = cfg.to_dict()
    assert ModelConfig.from_dict(json.loads(json.dumps(d))).to_dict() == d
    for bad in (0, 1.5, -1.0, math.nan):
        with pytest.raises(ValueError, match="cfg_rescale"):
            ModelConfig(cfg_rescale=bad, **kw)
    with pytest.raises(ValueError, match="cfg_zero_star must be a bool"):
        ModelConfig(cfg_zero_star=1, **kw)
    for bad in (-1, 31, True, 1.5):
        with pytest.raises(ValueError, match="cfg_zero_init"):
            ModelConfig(cfg_zero_init=bad, **kw)
    assert ModelConfig(cfg_zero_init=30, **kw).cfg_zero_init == 30 and ModelConfig(nfe_step=8, cfg_zero_init=6, **kw).cfg_zero_init == 6
    with pytest.raises(ValueError, match="cfg_zero_init"):
        ModelConfig(nfe_step=8, cfg_zero_init=7, **kw)
    with pytest.raises(ValueError, match="cfg_norm_report needs cfg_zero_star or cfg_rescale"):
        ModelConfig(cfg_norm_report=True, **kw)
    seen = set()
    for on in ON:
        for other, word in REFUSALS + [(dict(block_cache=(0, 2, 2)), "block_cache")]:
            with pytest.raises(ValueError) as ei:
                ModelConfig(**on, **other, **kw)
            assert "cfg_zero_star / cfg_rescale" in str(ei.value) and word in str(ei.value)
            seen.add(str(ei.value))
    assert len(seen) == 3                                                       # a sentence of its own each
    # zero-init is a plan: it combines with everything, block caching included
    assert ModelConfig(cfg_zero_init=2, block_cache=(0, 2, 2), **kw).cfg_zero_init == 2
    assert ModelConfig(cfg_zero_init=2, cfg_reuse=2, **kw).cfg_zero_init == 2 and ModelConfig(cfg_zero_init=1, apg_eta=0.5, ode_method="ab3", **kw)
    # "off" values refuse nothing
    assert ModelConfig(cfg_zero_star=True, cfg_reuse=1, apg_eta=1.0, **kw).cfg_zero_star is True


def test_request_options(tmp_path):
    from vietvoice_tts_amd.core import ModelConfig
    from vietvoice_tts_amd.request_options import MarkedRequestOptions, NormedRequestOptions, RequestOptions, column
    assert RequestOptions().cfg_zero_star is None and RequestOptions().cfg_rescale is None
    assert type(RequestOptions.checked()) is RequestOptions and type(RequestOptions.checked(watermark_payload=5)) is MarkedRequestOptions
    o = RequestOptions.checked(cfg_zero_star=True, cfg_rescale=1)
    assert isinstance(o, RequestOptions) and type(o) is NormedRequestOptions
    assert o.cfg_zero_star is True and o.cfg_rescale == 1.0 and type(o.cfg_rescale) is float and o.watermark_payload is None
    assert list(vars(o))[-2:] == ["cfg_zero_star", "cfg_rescale"]               # the two trailing fields
    assert RequestOptions.checked(cfg_zero_star=False).cfg_zero_star is False
    assert RequestOptions.checked(cfg_rescale=0.5, watermark_payload=7).watermark_payload == 7
    with pytest.raises(ValueError, match="cfg_rescale must satisfy 0 < phi <= 1"):
        RequestOptions.checked(cfg_rescale=0.0)
    with pytest.raises(ValueError, match="cfg_zero_star must be a bool or None"):
        RequestOptions.checked(cfg_zero_star=1)
    with pytest.raises(ValueError, match="cfg_interval"):                       # the existing fields' errors come first
        RequestOptions.checked(cfg_interval=(0.9, 0.1), cfg_rescale=2.0)
    kw = dict(model_cache_dir=str(tmp_path), synthetic_model=True, model_spec="tiny")
    plain, eng = ModelConfig(**kw), ModelConfig(cfg_zero_star=True, cfg_rescale=0.7, cfg_strength=2.5, **kw)
    assert type(RequestOptions().resolved(plain)) is RequestOptions
    r = RequestOptions().resolved(eng)
    assert (r.cfg_zero_star, r.cfg_rescale, r.cfg_strength) == (True, 0.7, 2.5) and r.resolved(eng) == r
    r = RequestOptions.checked(cfg_zero_star=False, cfg_rescale=0.25).resolved(eng)
    assert (r.cfg_zero_star, r.cfg_rescale) == (False, 0.25) and r.resolved(eng) == r      # an explicit "off" beats the engine's
    r = RequestOptions.checked(cfg_rescale=0.5, pitch=2.0).resolved(plain)
    assert (r.cfg_zero_star, r.cfg_rescale, r.pitch) == (None, 0.5, 2.0) and r.wants_output_stage()
    assert not RequestOptions.checked(cfg_zero_star=True).wants_output_stage()
    assert column([RequestOptions(), o], "cfg_rescale") == [None, 1.0] and column([RequestOptions()], "cfg_zero_star") is None


def test_batching_frontend_refuses(tmp_path):
    from vietvoice_tts_amd.batching import BatchingFrontend
    from vietvoice_tts_amd.core import ModelConfig
    import inspect
    sig = inspect.signature(BatchingFrontend.submit).parameters
    assert "cfg_zero_star" in sig and "cfg_rescale" in sig and "cfg_zero_init" not in sig       # zero-init is the engine's alone
    fe = BatchingFrontend(engine=None, overlap=False)
    try:
        with pytest.raises(ValueError, match="cfg_rescale must satisfy 0 < phi <= 1"):
            fe.submit("x", cfg_rescale=1.5).result(timeout=5)
        with pytest.raises(ValueError, match="cfg_zero_star must be a bool or None"):
            fe.submit("x", cfg_zero_star="on").result(timeout=5)
        for on in ON:
            for other, word in REFUSALS:
                with pytest.raises(ValueError) as ei:
                    fe.submit("x", **on, **other).result(timeout=5)
                assert "cfg_zero_star / cfg_rescale" in str(ei.value) and word in str(ei.value)
    finally:
        fe.close()
    kw = dict(model_cache_dir=str(tmp_path), synthetic_model=True, model_spec="tiny")
    for config, own, word in ((ModelConfig(block_cache=(0, 2, 2), **kw), dict(cfg_zero_star=True), "block_cache"),
                              (ModelConfig(apg_eta=0.5, **kw), dict(cfg_rescale=0.7), "apg_eta / apg_norm"),
                              (ModelConfig(cfg_zero_star=True, **kw), dict(cfg_reuse=3), "cfg_reuse > 1")):      # the engine's value counts as the request's
        fe = BatchingFrontend(engine=SimpleNamespace(config=config), overlap=False)
        try:
            with pytest.raises(ValueError) as ei:
                fe.submit("x", **own).result(timeout=5)
            assert "cfg_zero_star / cfg_rescale" in str(ei.value) and word in str(ei.value)
        finally:
            fe.close()


def test_sessions_carry_the_fields():
    from vietvoice_tts_amd.core.model import HipSession
    s = HipSession(None, "transformer", None, cfg_zero_star=True, cfg_rescale=0.7)
    assert s.cfg_zero_star is True and s.cfg_rescale == 0.7
    s = HipSession(None, "transformer", None)
    assert s.cfg_zero_star is False and s.cfg_rescale is None


# ------------------------------------------------------------------------------------------------ 5. header, map, exports
def test_header_map_and_binding_agree():
    from vietvoice_tts_amd import runtime
    root = os.path.dirname(HERE)
    hdr = open(os.path.join(root, "include", "vvtts.h")).read()
    declared = set(re.findall(r"\b(vv_[a-z0-9_]+)\s*\(", hdr))
    lib = runtime.load_library()
    for name in ("vv_transformer_steps_norm", "vv_transformer_norm_ws_bytes", "vv_cfg_norm_coef", "vv_ode_stage_norm"):
        assert name in declared and name in runtime.EXPORTS and hasattr(lib, name)
    vmap = open(os.path.join(root, "vietvoice-tts_amd", "csrc", "vvtts.map")).read()
    assert re.search(r"global:\s*vv_\*;", vmap) and re.search(r"local:\s*\*;", vmap)            # every vv_* leaves the library, nothing else
    assert C.sizeof(runtime.vv_cfg_norm_args) == 24 and C.sizeof(runtime.vv_cfg_norm_coef_args) == 112
    m = re.search(r"typedef struct vv_cfg_norm_coef_args \{(.*?)\} vv_cfg_norm_coef_args;", hdr, re.S)
    names = re.findall(r"[\s*]([A-Za-z_0-9]+)\s*[,;]", m.group(1))
    assert names == [f[0] for f in runtime.vv_cfg_norm_coef_args._fields_]
    m = re.search(r"typedef struct vv_cfg_norm_args \{(.*?)\} vv_cfg_norm_args;", hdr, re.S)
    assert re.findall(r"\*\s*([a-z]+);", m.group(1)) == [f[0] for f in runtime.vv_cfg_norm_args._fields_] == ["star", "rescale", "report"]
    src = open(os.path.join(root, "vietvoice-tts_amd", "csrc", "vv_elementwise.hip")).read()
    for kernel in ("cfg_gram_reduce_kernel", "cfg_norm_coef_kernel"):
        assert f"void {kernel}(" in src
    assert "template <bool GUIDED, bool APG, bool REUSE = false, bool NORM = false>" in src
    assert re.search(r"static_assert\(!NORM \|\| \(GUIDED && !APG && !REUSE\)", src)


# ------------------------------------------------------------------------------------------------ 6. the rule matters on the device file's inputs
@pytest.fixture(scope="module")
def refs():
    from tests import sampler_util as S
    S.setup()
    return S


@pytest.mark.parametrize("plan", list(U.NORM_PLANS))
def test_the_rule_moves_the_reference_of_every_guided_item(refs, plan):
    """The device file's last condition, checked here before its inputs are fixed: on sampler_util's model seed the same solver with the
    rule off lies more than MATTERS bounds away for every guided item, and s* is not within 1e-2 of 1."""
    S = refs
    for name, per_item in U.OPTION_SETS.items():
        for b, g in enumerate(S.ITEM_G):
            star, phi = per_item[b]
            if g == 0.0 or not (star or phi):
                continue
            log = []
            r64 = U.reference("f64", plan, b, g, star, phi, log=log)
            _, y, bd = U.parity_refs(plan, b, g, star, phi)
            off = U.reference("f64", plan, b, g, False, None)
            moved = S.err(off, r64)
            ss, ff = [v[1] for v in log], [v[2] for v in log]
            print(f"CFG_NORM_MATTERS {plan} {name} item {b} moved {moved:.3e} bound {bd:.3e} ratio {moved / bd:.1f} "
                  f"s [{min(ss):.4f}, {max(ss):.4f}] f [{min(ff):.4f}, {max(ff):.4f}]")
            assert moved > S.MATTERS * bd, (plan, name, b, moved, bd)
            if star:
                assert min(abs(v - 1.0) for v in ss) > 1e-2, (plan, name, b, ss)
            if phi:
                assert max(abs(v - 1.0) for v in ff) > 1e-2, (plan, name, b, ff)


def test_rule_off_is_the_sampler_matrix_solver_bit_for_bit(refs):
    """ref_solve_norm with both options off is sampler_util.ref_solve_all: the new solver adds the slope and nothing else."""
    S = refs
    spec, _, _, orcs, pres = S.setup()
    from vietvoice_tts_amd.model_spec import ode_plan
    for plan_level, (method, nfe) in U.NORM_PLANS.items():
        plan = ode_plan(nfe, spec.sway_coef, method)
        pre = pres["f32", 2]
        a = U.ref_solve_norm(orcs["f32"], pre, pre["noise"], plan, g=3.0)
        b = S.ref_solve_all(orcs["f32"], pre, pre["noise"], plan, g=3.0)
        assert torch.equal(a, b), plan_level


def test_zero_init_moves_the_reference(refs):
    S = refs
    for b, g in ((0, 2.0), (2, 3.0)):
        r0 = U.reference("f64", "euler", b, g, True, U.PHI)
        r2, y, bd = U.parity_refs("euler", b, g, True, U.PHI, skip=2)
        assert S.err(r0, r2) > S.MATTERS * bd
