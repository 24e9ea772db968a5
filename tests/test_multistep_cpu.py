"""N20 host side (no GPU): the Adams-Bashforth weights in exact rationals, the multistep plan on the sway-sampled grid, the orders on
the smooth scalar problem of test_ode_cpu.py, the config fields, the C ABI's new entries and the report mirror."""
import ctypes
import os
import re
from fractions import Fraction as F

import numpy as np
import pytest
import torch

from tests import multistep_util as mu
from vietvoice_tts_amd.model_spec import ODE_METHODS, ODE_MULTISTEP, guidance_mask, multistep_weights, ode_plan

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_EXPORTS = ["vv_set_ode_multistep", "vv_ode_diff_reduce"]


def _exact_weights(t, q):
    """The integrals of the Lagrange basis over [t_n, t_{n+1}] / h_n in exact rationals, written out per order (not the general
    polynomial product of model_spec): k = 1: 1; k = 2: 1 + w, -w, w = h / (2 a); k = 3 from the Newton form's two integrals."""
    tq = [F(float(v)) for v in t]
    rows = []
    for n in range(len(tq) - 1):
        h = tq[n + 1] - tq[n]
        k = min(q, n + 1)
        if k == 1:
            row = [F(1)]
        elif k == 2:
            w = h / (2 * (tq[n] - tq[n - 1]))
            row = [1 + w, -w]
        else:
            a, b = tq[n] - tq[n - 1], tq[n - 1] - tq[n - 2]
            i1, i2 = h / 2, (h * h / 3 + a * h / 2)            # the integrals of s and s (s + a), each divided by h
            # f[n, n-1] = (f0 - f1) / a;  f[n, n-1, n-2] = ((f0 - f1) / a - (f1 - f2) / b) / (a + b)
            c0 = 1 + i1 / a + i2 / (a * (a + b))
            c1 = -i1 / a - i2 / (a + b) * (1 / a + 1 / b)
            c2 = i2 / (b * (a + b))
            row = [c0, c1, c2]
        rows.append(tuple(float(v) for v in row) + (0.0,) * (q - k))
    return tuple(rows)


def test_multistep_names():
    assert ODE_MULTISTEP == {"ab2": 2, "ab3": 3} and not set(ODE_MULTISTEP) & set(ODE_METHODS)


@pytest.mark.parametrize("sway", [-1.0, 0.0, 0.5])
@pytest.mark.parametrize("q", [1, 2, 3])
def test_weights_are_the_exact_integrals_rounded_once(q, sway):
    for n in (2, 3, 9, 32):
        t = mu.grid64(n, sway)
        got = multistep_weights(t, q)
        assert got == _exact_weights(t, q), (q, sway, n)
        assert len(got) == n - 1 and all(len(r) == q for r in got)
        for i, r in enumerate(got):
            assert abs(sum(r) - 1.0) <= 1e-15, (i, r)
            assert all(v == 0.0 for v in r[min(q, i + 1):]), "no weight on a slope from before step 0"
            assert all(v != 0.0 for v in r[:min(q, i + 1)])
        assert got[0][0] == 1.0                                           # step 0 is Euler


def test_uniform_grid_gives_the_textbook_weights():
    t = np.arange(9, dtype=np.float64) / 8.0                              # exactly representable: the rationals are the textbook's
    assert multistep_weights(t, 1) == ((1.0,),) * 8
    w2 = multistep_weights(t, 2)
    assert w2[0] == (1.0, 0.0) and all(r == (1.5, -0.5) for r in w2[1:])
    w3 = multistep_weights(t, 3)
    assert w3[0] == (1.0, 0.0, 0.0) and w3[1] == (1.5, -0.5, 0.0)
    assert all(r == (float(F(23, 12)), float(F(-4, 3)), float(F(5, 12))) for r in w3[2:])


@pytest.mark.parametrize("sway", [-1.0, 0.0, 0.5])
def test_ab2_closed_form_on_the_sway_grid(sway):
    t = mu.grid64(17, sway)
    w2 = multistep_weights(t, 2)
    for n in range(1, 16):
        w = F(float(t[n + 1])) - F(float(t[n]))
        w = w / (2 * (F(float(t[n])) - F(float(t[n - 1]))))
        assert w2[n] == (float(1 + w), float(-w)), n


def test_weights_refuse_what_they_cannot_do():
    for bad_q in (0, 4):
        with pytest.raises(ValueError):
            multistep_weights([0.0, 0.5, 1.0], bad_q)
    for bad_t in ([0.0], [0.0, 0.5, 0.5], [0.0, 0.6, 0.5]):
        with pytest.raises(ValueError):
            multistep_weights(bad_t, 2)


@pytest.mark.parametrize("name", ["ab2", "ab3"])
@pytest.mark.parametrize("sway", [-1.0, 0.0])
def test_plan_is_eulers_with_the_weights(name, sway):
    for n in (2, 3, 9):
        plan, e = ode_plan(n, sway, name), ode_plan(n, sway, "euler")
        assert plan.s == 1 and torch.equal(plan.t, e.t) and torch.equal(plan.dt, e.dt) and plan.a == e.a and plan.b == e.b
        assert e.beta is None and plan.beta == multistep_weights(mu.grid64(n, sway), ODE_MULTISTEP[name])
        for interval, g in (((0.2, 0.7), [2.0, 0.0, 1.0]), (None, [2.0, 0.0]), (((0.0, 0.4), (0.5, 1.0)), [1.0, 1.0])):
            m, me = guidance_mask(plan, interval, g), guidance_mask(e, interval, g)
            assert (m is None and me is None) or torch.equal(m, me)
    assert ode_plan(9, -1.0, "midpoint").beta is None                    # the Runge-Kutta plans carry none
    with pytest.raises(ValueError):
        ode_plan(9, -1.0, "ab4")


def _scalar_error(name, n, sway, ref):
    f = lambda t, x: np.cos(3.0 * t) * x - 2.0 * t
    t = mu.grid64(n, sway)
    beta = ode_plan(n, sway, name).beta if name != "euler" else tuple((1.0,) for _ in range(n - 1))
    x, hist = 1.0, []
    for i in range(n - 1):                                                # the plan's own weights, on the float64 grid
        hist.insert(0, f(t[i], x))
        x = x + (t[i + 1] - t[i]) * sum(b * hist[j] for j, b in enumerate(beta[i]) if b != 0.0)
    return abs(x - ref)


def _scalar_ref():
    from tests.test_ode_cpu import _integrate
    return _integrate(ode_plan(4097, -1.0, "rk4"), lambda t, x: np.cos(3.0 * t) * x - 2.0 * t, 1.0)


@pytest.mark.parametrize("name,sway,p", [("ab2", -1.0, 2), ("ab3", -1.0, 3), ("ab2", 0.0, 2), ("ab3", 0.0, 2)])
def test_order_on_a_smooth_scalar_problem(name, sway, p):
    """x' = cos(3 t) x - 2 t, x(0) = 1 (test_ode_cpu.py's problem and margin: the error ratio of 17 against 33 points is at least
    0.75 * 2^p).  With the Euler start ab3 has order 3 on the sway -1 grid (its first step is O(n^-2) long) and order 2 on the uniform
    grid; ab2 has order 2 on both."""
    ref = _scalar_ref()
    e17, e33 = _scalar_error(name, 17, sway, ref), _scalar_error(name, 33, sway, ref)
    ratio = e17 / e33
    print(f"{name} sway {sway}: err(17) = {e17:.3e}, err(33) = {e33:.3e}, ratio = {ratio:.2f}")
    assert ratio >= 0.75 * 2 ** p, (name, sway, ratio)
    if name == "ab2":
        assert e17 < _scalar_error("euler", 17, sway, ref) and e33 < _scalar_error("euler", 33, sway, ref)


@pytest.mark.parametrize("q", [1, 2, 3])
def test_reference_solver_agrees_with_the_weights(q):
    """The Newton-form solver of multistep_util and a solver that applies multistep_weights are the same method: equal to rounding."""
    f = lambda t, x: np.cos(3.0 * t) * x - 2.0 * t
    for sway in (-1.0, 0.0):
        t = mu.grid64(17, sway)
        beta = multistep_weights(t, q)
        x, hist = 1.0, []
        for i in range(16):
            hist.insert(0, f(t[i], x))
            x = x + (t[i + 1] - t[i]) * sum(b * hist[j] for j, b in enumerate(beta[i]) if b != 0.0)
        assert abs(mu.integrate_scalar(t, q, f, 1.0) - x) < 1e-13


def test_model_config_fields(tmp_path):
    from vietvoice_tts_amd.core import ModelConfig
    kw = dict(model_cache_dir=str(tmp_path), synthetic_model=True, model_spec="tiny")
    for name in ("ab2", "ab3"):
        cfg = ModelConfig(ode_method=name, **kw)
        assert cfg.ode_method == name and cfg.ode_report is False
        assert ModelConfig(ode_method=name, ode_report=True, **kw).ode_report is True
    with pytest.raises(ValueError):
        ModelConfig(ode_method="ab4", **kw)
    for name in ("euler", "midpoint"):
        with pytest.raises(ValueError, match="ode_report"):
            ModelConfig(ode_method=name, ode_report=True, **kw)
    d = ModelConfig(ode_method="ab3", ode_report=True, **kw).to_dict()
    assert d["ode_method"] == "ab3" and d["ode_report"] is True and ModelConfig.from_dict(d).to_dict() == d
    assert ModelConfig(**kw).ode_report is False


def test_header_version_script_and_exports_agree_for_the_new_entries():
    from vietvoice_tts_amd import runtime
    hdr = open(os.path.join(ROOT, "include", "vvtts.h")).read()
    declared = set(re.findall(r"VV_API\s+[\w\s\*]+?\b(vv_\w+)\s*\(", hdr))
    assert declared == set(runtime.EXPORTS), declared ^ set(runtime.EXPORTS)
    ver = open(os.path.join(ROOT, "vietvoice-tts_amd", "csrc", "vvtts.map")).read()
    globs = [g.strip() for g in re.findall(r"global:\s*([^;]+);", ver)]
    lib = runtime.load_library()
    for name, n_args in (("vv_set_ode_multistep", 7), ("vv_ode_diff_reduce", 3), ("vv_set_ode_report", 4)):
        assert name in declared and len(runtime.EXPORTS[name][1]) == n_args
        assert any(re.fullmatch(g.replace("*", ".*"), name) for g in globs) and hasattr(lib, name)
        args = [None if t is ctypes.c_void_p or isinstance(t, type(ctypes.POINTER(ctypes.c_int))) else 0 for t in runtime.EXPORTS[name][1]]
        assert getattr(lib, name)(*args) == -22                                       # no context: refused before anything else
    assert len(runtime.EXPORTS["vv_set_ode_plan"][1]) == 8                            # the old entry keeps its arguments
    assert "typedef struct vv_ode_diff_args" in hdr
    assert ctypes.sizeof(runtime.vv_ode_diff_args) == 8 + 8 + 4 * 4 + 4 * 8
    assert ctypes.sizeof(runtime.vv_steps_args) == 8 + 9 * 8 + 8 + 8 + 8 + 8          # untouched
    m = re.match(rb"vvtts-hip (\d+)\.(\d+) ", lib.vv_version())
    assert m and (int(m.group(1)), int(m.group(2))) >= (0, 13)                        # bumped with the additive entries
    assert int(re.search(r"#define\s+VV_APG_TILE\s+(\d+)", hdr).group(1)) == mu.TILE


@pytest.mark.parametrize("frames", [0, 1, 31, 32, 33, 67, 200])
def test_report_mirror_against_a_plain_float64_sum(frames):
    """The mirror only reorders float64 additions of non-negative terms: within n * 2^-53 relative of any other order, 1e-12 here."""
    rng = np.random.default_rng(frames)
    f = rng.standard_normal((frames, 100)).astype(np.float32)
    p = (f + 0.1 * rng.standard_normal((frames, 100))).astype(np.float32)
    for prev in (p, None):
        (d2, f2), (pd2, pf2) = mu.report_mirror(f, prev), mu.report_plain(f, prev)
        assert abs(d2 - pd2) <= 1e-12 * pd2 and abs(f2 - pf2) <= 1e-12 * pf2
        if prev is None or frames == 0:
            assert d2 == 0.0
        else:
            assert d2 > 0.0 and f2 > 0.0
    if frames > mu.TILE:                                                  # an item's sums do not depend on the rows behind it
        assert mu.report_mirror(f[:mu.TILE], p[:mu.TILE]) != mu.report_mirror(f, p)
        g = np.concatenate([f, f[:5]])
        assert mu.report_mirror(g[:frames], p) == mu.report_mirror(f, p)
