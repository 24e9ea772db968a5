"""N7 host side (no GPU): the Runge-Kutta tableaus in exact fractions, the plan on the sway-sampled time grid, each method's order
on a SMOOTH scalar problem (the synthetic model's velocity field is too rough to show an order: no test claims one on it), and
the build-only config fields."""
import os
import re
from fractions import Fraction as F

import numpy as np
import pytest
import torch

from vietvoice_tts_amd.model_spec import ODE_METHODS, ModelSpec, ode_plan, ode_tableau, time_grid

HERE = os.path.dirname(os.path.abspath(__file__))
ORDER = {"euler": 1, "midpoint": 2, "heun2": 2, "heun3": 3, "rk4": 4}


def test_builtin_methods_are_the_documented_set():
    assert set(ODE_METHODS) == set(ORDER)
    assert [len(ODE_METHODS[m][1]) for m in ("euler", "midpoint", "heun2", "heun3", "rk4")] == [1, 2, 2, 3, 4]


@pytest.mark.parametrize("name", sorted(ORDER))
def test_tableau_order_conditions_in_exact_fractions(name):
    a, b = ODE_METHODS[name]
    s, p = len(b), ORDER[name]
    assert len(a) == s and all(len(r) == s for r in a)
    assert all(isinstance(v, F) for r in a for v in r) and all(isinstance(v, F) for v in b)
    assert all(a[i][j] == 0 for i in range(s) for j in range(i, s)), "strictly lower triangular"
    c = [sum(r) for r in a]
    R = range(s)
    assert sum(b) == 1
    if p >= 2:
        assert sum(b[i] * c[i] for i in R) == F(1, 2)
    if p >= 3:
        assert sum(b[i] * c[i] ** 2 for i in R) == F(1, 3)
        assert sum(b[i] * a[i][j] * c[j] for i in R for j in R) == F(1, 6)
    if p >= 4:
        assert sum(b[i] * c[i] ** 3 for i in R) == F(1, 4)
        assert sum(b[i] * c[i] * a[i][j] * c[j] for i in R for j in R) == F(1, 8)
        assert sum(b[i] * a[i][j] * c[j] ** 2 for i in R for j in R) == F(1, 12)
        assert sum(b[i] * a[i][j] * a[j][k] * c[k] for i in R for j in R for k in R) == F(1, 24)
    # and NOT the next order's first condition: the declared order is the method's own
    assert sum(b[i] * c[i] ** p for i in R) != F(1, p + 1)


@pytest.mark.parametrize("n", [2, 5, 9, 32])
@pytest.mark.parametrize("sway", [-1.0, 0.0, 0.5])
def test_euler_plan_is_the_time_grid_bit_for_bit(n, sway):
    plan = ode_plan(n, sway, "euler")
    t, dt = time_grid(n, sway)
    assert plan.s == 1 and plan.t.dtype == torch.float32 and plan.dt.dtype == torch.float32
    assert torch.equal(plan.t, t) and torch.equal(plan.dt, dt)
    assert torch.equal(ode_plan(n, sway).t, t)                      # the default method


@pytest.mark.parametrize("name", sorted(ORDER))
def test_plan_evaluation_times(name):
    n, sway = 9, -1.0
    plan = ode_plan(n, sway, name)
    a, b = ODE_METHODS[name]
    s = len(b)
    assert plan.s == s and plan.t.shape == ((n - 1) * s,) and plan.dt.shape == (n - 1,)
    assert plan.a == tuple(tuple(float(v) for v in r) for r in a) and plan.b == tuple(float(v) for v in b)
    t, dt = time_grid(n, sway)
    assert torch.equal(plan.dt, dt)
    # t_n + c_i h_n in float64 on the float64 grid, then fp32
    g = torch.linspace(0.0, 1.0, n, dtype=torch.float64)
    g = g + sway * (torch.cos(np.pi / 2 * g) - 1.0 + g)
    c = [float(sum(r)) for r in a]
    want = torch.stack([g[:-1] + ci * (g[1:] - g[:-1]) for ci in c], dim=1).clamp(0.0, 1.0).reshape(-1).to(torch.float32)
    assert torch.equal(plan.t, want)
    te = plan.t.reshape(n - 1, s)
    assert torch.equal(te[:, 0], t)
    assert bool((te[:, 1:] >= te[:, :-1]).all()), "non-decreasing within a step"
    assert float(plan.t.min()) >= 0.0 and float(plan.t.max()) <= 1.0


def test_custom_tableau_and_refusals():
    ralston = (((0, 0), (F(2, 3), 0)), (F(1, 4), F(3, 4)))
    plan = ode_plan(5, -1.0, ralston)
    assert plan.s == 2 and plan.b == (0.25, 0.75) and plan.a[1][0] == float(F(2, 3))
    assert ode_tableau("midpoint") == (((0.0, 0.0), (0.5, 0.0)), (0.0, 1.0))
    for bad in ("nope", (((0, 1), (0, 0)), (0.5, 0.5)), (((0, 0), (1, 0)), (0.5, 0.6)), (((0.5,),), (1.0,)),
                (tuple(tuple(0 for _ in range(5)) for _ in range(5)), (1, 0, 0, 0, 0)), (((0, 0), (float("nan"), 0)), (0.5, 0.5)), 3):
        with pytest.raises(ValueError):
            ode_plan(5, -1.0, bad)


def _integrate(plan, f, x0):
    """numpy interpreter of a plan: x_i = x_n + h sum_j a_ij k_j, k_i = f(t_n + c_i h, x_i), x_{n+1} = x_n + h sum_j b_j k_j."""
    s = plan.s
    t = plan.t.double().numpy().reshape(-1, s)
    x = float(x0)
    for n, h in enumerate(plan.dt.double().numpy()):
        k = []
        for i in range(s):
            xi = x + h * sum(plan.a[i][j] * k[j] for j in range(i) if plan.a[i][j] != 0.0)
            k.append(f(t[n, i], xi))
        x = x + h * sum(plan.b[j] * k[j] for j in range(s) if plan.b[j] != 0.0)
    return x


@pytest.mark.parametrize("name", sorted(ORDER))
def test_order_on_a_smooth_scalar_problem(name):
    """x' = cos(3 t) x - 2 t, x(0) = 1 on the sway-sampled grid (sway_coef = -1): halving the grid divides the error by about 2^p.
    Error against rk4 on 4097 points.  Measured: 2.06, 4.38 (midpoint), 3.58 (heun2), 8.88, 15.4.  (The plan's times and steps are
    fp32 values of the float64 grid; their 6e-8 rounding shows only in rk4, whose error on 33 points is 1.6e-7: 15.4 here against
    15.8 on the float64 grid, well inside the band.)"""
    f = lambda t, x: np.cos(3.0 * t) * x - 2.0 * t
    ref = _integrate(ode_plan(4097, -1.0, "rk4"), f, 1.0)
    e17 = abs(_integrate(ode_plan(17, -1.0, name), f, 1.0) - ref)
    e33 = abs(_integrate(ode_plan(33, -1.0, name), f, 1.0) - ref)
    ratio = e17 / e33
    print(f"{name}: err(17) = {e17:.3e}, err(33) = {e33:.3e}, ratio = {ratio:.2f}")
    p = ORDER[name]
    assert 0.75 * 2 ** p <= ratio <= 1.25 * 2 ** p, (name, ratio)


def test_model_config_fields(tmp_path):
    from vietvoice_tts_amd.core import ModelConfig
    kw = dict(model_cache_dir=str(tmp_path), synthetic_model=True, model_spec="tiny")
    cfg = ModelConfig(**kw)
    assert cfg.ode_method == "euler" and cfg.cfg_strength is None
    with pytest.raises(ValueError):
        ModelConfig(ode_method="nope", **kw)
    with pytest.raises(ValueError):
        ModelConfig(cfg_strength=float("nan"), **kw)
    cfg = ModelConfig(ode_method="rk4", cfg_strength=1.5, **kw)
    d = cfg.to_dict()
    assert d["ode_method"] == "rk4" and d["cfg_strength"] == 1.5
    back = ModelConfig.from_dict(d)
    assert back.to_dict() == d
    # the reference's fields, order and defaults come first, unchanged
    names = list(d)
    assert names[:4] == ["model_url", "model_cache_dir", "model_filename", "nfe_step"] and names.index("ode_method") > names.index("device")


def test_header_and_binding_declare_the_new_entries():
    from vietvoice_tts_amd import runtime
    hdr = open(os.path.join(os.path.dirname(HERE), "include", "vvtts.h")).read()
    declared = set(re.findall(r"\b(vv_[a-z0-9_]+)\s*\(", hdr))
    for name in ("vv_set_ode_plan", "vv_transformer_steps_ex", "vv_ode_stage"):
        assert name in declared and name in runtime.EXPORTS
    assert "typedef struct vv_steps_args" in hdr and "const float* cfg_item" in hdr
    # the ctypes mirrors have the C layouts' sizes (LP64: pointers 8-byte aligned)
    import ctypes as C
    assert C.sizeof(runtime.vv_steps_args) == 8 + 9 * 8 + 8 + 8 + 8 + 8
    assert C.sizeof(runtime.vv_ode_stage_args) == 8 + 8 + 16 + 24 + 16 + 8 + 8 + 8 + 8 + 8 + 8
    assert hasattr(runtime.load_library(), "vv_transformer_steps_ex")


def test_batching_frontend_refuses_a_non_finite_strength():
    from vietvoice_tts_amd.batching import BatchingFrontend
    fe = BatchingFrontend(engine=None, overlap=False)
    try:
        with pytest.raises(ValueError):
            fe.submit("x", cfg_strength=float("inf")).result(timeout=5)
    finally:
        fe.close()
