"""N21 host side (no GPU): the three-valued guidance mask on hand-worked plans, ``reuse`` off against the N8 mask case by case, the checks,
the config fields, the request options, the front end's validation, the numpy mirror of the drift report and the mask validator."""
import json
import os
import re

import numpy as np
import pytest
import torch

from tests import cfg_reuse_util as U
from vietvoice_tts_amd.model_spec import OdePlan, check_cfg_reuse, guidance_mask, ode_plan

HERE = os.path.dirname(os.path.abspath(__file__))


def _plan(t, s=1):
    t = torch.tensor(t, dtype=torch.float32)
    return OdePlan(t, torch.full((t.numel() // s,), 0.25), ((0.0,),) * s, (1.0,) + (0.0,) * (s - 1), s)


def _col(m, b=0):
    return [int(v) for v in m[:, b]]


# ------------------------------------------------------------------------------------------------ 1. worked masks
def test_euler_on_eight_points():
    """7 evaluations, every one guided: the unconditional branch at evaluations 0, k, 2k, ..."""
    plan = ode_plan(8, -1.0, "euler")
    assert plan.s == 1 and plan.t.numel() == 7
    assert guidance_mask(plan, None, [2.0], 1) is None                                         # k = 1 is off: the unmasked call
    assert _col(guidance_mask(plan, None, [2.0], 2)) == [1, 2, 1, 2, 1, 2, 1]
    assert _col(guidance_mask(plan, None, [2.0], 3)) == [1, 2, 2, 1, 2, 2, 1]
    assert _col(guidance_mask(plan, None, [2.0], 7)) == [1, 2, 2, 2, 2, 2, 2]
    assert _col(guidance_mask(plan, None, [2.0], 100)) == [1, 2, 2, 2, 2, 2, 2]
    m = guidance_mask(plan, None, [2.0, 2.0], 2)
    assert m.dtype == torch.uint8 and m.shape == (7, 2) and _col(m, 0) == _col(m, 1)


def test_the_count_starts_at_the_first_guided_evaluation():
    """Times that fp32 holds exactly; the interval leaves out evaluation 0 and evaluations 5, 6."""
    plan = _plan([0.0, 0.125, 0.25, 0.375, 0.5, 0.625, 0.75])
    assert _col(guidance_mask(plan, (0.125, 0.5), [2.0])) == [0, 1, 1, 1, 1, 0, 0]
    assert _col(guidance_mask(plan, (0.125, 0.5), [2.0], 2)) == [0, 1, 2, 1, 2, 0, 0]
    assert _col(guidance_mask(plan, (0.125, 0.5), [2.0], 3)) == [0, 1, 2, 2, 1, 0, 0]
    assert _col(guidance_mask(plan, (0.125, 0.5), [2.0], 4)) == [0, 1, 2, 2, 2, 0, 0]
    assert _col(guidance_mask(plan, (0.5, 0.5), [2.0], 2)) == [0, 0, 0, 0, 1, 0, 0]
    assert _col(guidance_mask(plan, (0.55, 0.6), [2.0], 2)) == [0] * 7                          # nothing inside: all zero, not None


def test_strength_zero_and_one_k_per_item():
    plan = _plan([0.0, 0.125, 0.25, 0.375, 0.5, 0.625, 0.75])
    m = guidance_mask(plan, None, [2.0, 0.0, 3.0], 2)
    assert _col(m, 1) == [0] * 7                                                                # a zero strength is never guided: nothing to reuse
    assert _col(m, 0) == _col(m, 2) == [1, 2, 1, 2, 1, 2, 1]
    m = guidance_mask(plan, None, [2.0, 2.0, 2.0], (1, 2, 3))
    assert _col(m, 0) == [1] * 7 and _col(m, 1) == [1, 2, 1, 2, 1, 2, 1] and _col(m, 2) == [1, 2, 2, 1, 2, 2, 1]
    m = guidance_mask(plan, [(0.0, 0.25), None, (0.5, 1.0)], [1.0, 1.0, 1.0], [2, None, 2])    # its own interval and its own k per item
    assert _col(m, 0) == [1, 2, 1, 0, 0, 0, 0] and _col(m, 1) == [1] * 7 and _col(m, 2) == [0, 0, 0, 0, 1, 2, 1]
    with pytest.raises(ValueError, match="one cfg_reuse per item"):
        guidance_mask(plan, None, [1.0, 1.0], [2, 2, 2])
    # the rule restated on its own
    for k in (1, 2, 3, 5):
        assert _col(guidance_mask(plan, (0.125, 0.625), [2.0], k if k > 1 else 2)) == U.reuse_column([0, 1, 1, 1, 1, 1, 0], k if k > 1 else 2)


def test_rk4_counts_evaluations_not_steps():
    """rk4 on 4 points: 3 steps of 4 stages = 12 evaluations, numbered over the stages."""
    plan = ode_plan(4, 0.0, "rk4")
    assert plan.s == 4 and plan.t.numel() == 12
    assert _col(guidance_mask(plan, None, [2.0], 2)) == [1, 2] * 6
    assert _col(guidance_mask(plan, None, [2.0], 3)) == [1, 2, 2] * 4                           # computed at stages 0, 3 | 2 | 1 of the steps
    assert _col(guidance_mask(plan, None, [2.0], 5)) == [1, 2, 2, 2, 2, 1, 2, 2, 2, 2, 1, 2]
    # an interval that starts inside step 0 (stage times 0, 1/9, 2/9, 1/3, ...): the count starts there
    t = [float(v) for v in plan.t]
    lo = (t[1] + t[2]) / 2
    assert _col(guidance_mask(plan, (lo, 1.0), [2.0], 2)) == [0, 0] + [1, 2] * 5
    for name in ("ab2", "ab3"):                                                                 # a multistep plan: one evaluation per step, as Euler
        p = ode_plan(8, -1.0, name)
        assert _col(guidance_mask(p, None, [2.0], 2)) == [1, 2, 1, 2, 1, 2, 1]


# ------------------------------------------------------------------------------------------------ 2. off is today's function
@pytest.mark.parametrize("reuse", [None, 1, [1, None], (None, 1)])
def test_reuse_off_returns_todays_mask(reuse):
    """The cases of the N8 host tests, written out: with reuse off the function returns what it returns without the argument."""
    plan = _plan([0.0, 0.25, 0.5, 0.75])
    cases = [
        (plan, (0.25, 0.5), [2.0, 2.0], [[0, 0], [1, 1], [1, 1], [0, 0]]),
        (plan, None, [2.0, 1.0], None),
        (plan, (0.0, 1.0), [2.0, 1.0], None),
        (plan, None, [2.0, 0.0], [[1, 0]] * 4),
        (plan, (0.25, 0.75), [0.0, 2.0], [[0, 0], [0, 1], [0, 1], [0, 1]]),
        (plan, [(0.0, 0.25), (0.5, 1.0)], [1.0, 1.0], [[1, 0], [1, 0], [0, 1], [0, 1]]),
        (plan, (0.26, 0.49), [2.0, 2.0], [[0, 0]] * 4),
        (ode_plan(3, 0.0, "midpoint"), (0.2, 0.6), [2.0, 2.0], [[0, 0], [1, 1], [1, 1], [0, 0]]),
        (ode_plan(2, 0.0, "rk4"), (0.3, 0.7), [2.0, 0.0], [[0, 0], [1, 0], [1, 0], [0, 0]]),
    ]
    for p, iv, g, want in cases:
        got = guidance_mask(p, iv, g, reuse)
        base = guidance_mask(p, iv, g)
        assert (got is None) == (base is None) == (want is None)
        if want is not None:
            assert got.dtype == torch.uint8 and got.tolist() == want and torch.equal(got, base)


# ------------------------------------------------------------------------------------------------ 3. the checks
def test_check_cfg_reuse():
    assert check_cfg_reuse(None) is None
    assert check_cfg_reuse(1) == 1 and check_cfg_reuse(4) == 4 and check_cfg_reuse(np.int64(3)) == 3
    for bad in (0, -2, True, False, 2.0, 1.5, "2", (2,), float("nan")):
        with pytest.raises(ValueError) as ei:
            check_cfg_reuse(bad)
        assert str(ei.value) == "cfg_reuse must be an integer >= 1 or None"
    plan = _plan([0.0, 0.25])
    for bad in (0, True, 2.5, [2, 0]):
        with pytest.raises(ValueError, match="cfg_reuse must be an integer >= 1 or None"):
            guidance_mask(plan, None, [1.0, 1.0], bad)


def test_mask_validator_restates_the_librarys_refusals():
    """cfg_reuse_util.check_mask on hand-made masks: what vv_transformer_steps_reuse refuses of a mask (test_cfg_reuse_gpu.py holds the
    two side by side)."""
    ok = [[1, 0, 1], [2, 0, 1], [1, 1, 2], [2, 2, 2]]
    assert U.check_mask(ok) is None and U.check_mask([[1, 0], [0, 1]]) is None
    assert U.check_mask([[2, 1], [1, 1]]) == "2 before 1"
    assert U.check_mask([[0], [2], [1]]) == "2 before 1"                                        # a 0 is not a 1
    assert U.check_mask([[1], [2], [0], [2]]) is None                                           # after a gap the stored difference still stands
    assert U.check_mask([[1], [3]]) == "value"
    assert U.check_mask(ok, 1, 4) == "step0"                                                    # a 2 in the mask and a call that starts later
    assert U.check_mask([[1, 0], [0, 1]], 1, 2) is None                                         # without a 2 a call may start anywhere
    assert U.check_mask([[1], [2], [1], [2]], 0, 1) is None                                     # the call's own evaluations are what is checked
    plan = ode_plan(8, -1.0, "euler")                                                           # every mask the rule builds passes
    for k in (2, 3, 7):
        assert U.check_mask(guidance_mask(plan, (0.1, 0.9), [2.0, 0.0, 1.0], k).tolist()) is None


# ------------------------------------------------------------------------------------------------ 4. config, options, front end
def test_model_config_fields(tmp_path):
    from vietvoice_tts_amd.core import ModelConfig
    kw = dict(model_cache_dir=str(tmp_path), synthetic_model=True, model_spec="tiny")
    cfg = ModelConfig(**kw)
    assert cfg.cfg_reuse is None and cfg.cfg_reuse_report is False
    assert ModelConfig(cfg_reuse=1, **kw).cfg_reuse == 1 and ModelConfig(cfg_reuse=3, **kw).cfg_reuse == 3
    for bad in (0, -1, True, 2.5, "2"):
        with pytest.raises(ValueError, match="cfg_reuse must be an integer >= 1 or None"):
            ModelConfig(cfg_reuse=bad, **kw)
    for apg in (dict(apg_eta=0.5), dict(apg_norm=2.0), dict(apg_eta=0.0, apg_norm=1.0)):
        with pytest.raises(ValueError) as ei:
            ModelConfig(cfg_reuse=2, **apg, **kw)
        assert "cfg_reuse" in str(ei.value) and "apg_eta" in str(ei.value) and "apg_norm" in str(ei.value)
        assert ModelConfig(cfg_reuse=1, **apg, **kw).cfg_reuse == 1                             # 1 is off: nothing to refuse
    assert ModelConfig(cfg_reuse=2, apg_eta=1.0, **kw).cfg_reuse == 2                           # eta 1 without a cap is "off" (check_apg)
    for k in (None, 1):
        with pytest.raises(ValueError, match="cfg_reuse_report needs cfg_reuse > 1"):
            ModelConfig(cfg_reuse=k, cfg_reuse_report=True, **kw)
    cfg = ModelConfig(cfg_reuse=2, cfg_reuse_report=True, cfg_interval=(0.2, 0.8), **kw)
    d = cfg.to_dict()
    assert d["cfg_reuse"] == 2 and d["cfg_reuse_report"] is True
    assert ModelConfig.from_dict(json.loads(json.dumps(d))).to_dict() == d
    names = list(d)
    assert names.index("cfg_reuse") > names.index("apg_norm") and names.index("cfg_reuse_report") == names.index("cfg_reuse") + 1


def test_request_options(tmp_path):
    from vietvoice_tts_amd.core import ModelConfig
    from vietvoice_tts_amd.request_options import RequestOptions, column
    ten = RequestOptions(1.5, (0.2, 0.8), 0.5, 2.0, -16.0, "true", 2.0, 1.1, "keep", 1.0)      # the ten fields before this one, by position
    assert ten.cfg_reuse is None and ten.denoise == 1.0 and ten.cfg_strength == 1.5
    assert list(vars(RequestOptions()))[-1] == "cfg_reuse" and len(vars(RequestOptions())) == 11
    assert RequestOptions.checked().cfg_reuse is None
    assert RequestOptions.checked(cfg_reuse=2).cfg_reuse == 2 and RequestOptions.checked(cfg_reuse=1).cfg_reuse == 1
    for bad in (0, True, 1.5, "3"):
        with pytest.raises(ValueError, match="cfg_reuse must be an integer >= 1 or None"):
            RequestOptions.checked(cfg_reuse=bad)
    with pytest.raises(ValueError, match="cfg_interval"):                                       # the existing fields' errors come first
        RequestOptions.checked(cfg_interval=(0.9, 0.1), cfg_reuse=0)
    with pytest.raises(ValueError, match="cfg_strength"):
        RequestOptions.checked(cfg_strength=float("nan"), cfg_reuse=0)
    kw = dict(model_cache_dir=str(tmp_path), synthetic_model=True, model_spec="tiny")
    cfg = ModelConfig(cfg_reuse=3, **kw)
    assert RequestOptions().resolved(cfg).cfg_reuse == 3
    assert RequestOptions.checked(cfg_reuse=2).resolved(cfg).cfg_reuse == 2
    assert RequestOptions.checked(cfg_reuse=1).resolved(cfg).cfg_reuse == 1                     # an explicit "off" beats the engine's k
    assert RequestOptions().resolved(ModelConfig(**kw)).cfg_reuse is None
    assert column([RequestOptions(), RequestOptions.checked(cfg_reuse=2)], "cfg_reuse") == [None, 2]


def test_batching_frontend_refuses_bad_reuse():
    from vietvoice_tts_amd.batching import BatchingFrontend
    fe = BatchingFrontend(engine=None, overlap=False)
    try:
        for bad in (0, -1, True, 2.5):
            with pytest.raises(ValueError, match="cfg_reuse must be an integer >= 1 or None"):
                fe.submit("x", cfg_reuse=bad).result(timeout=5)
        for apg in (dict(apg_eta=0.5), dict(apg_norm=1.5)):
            with pytest.raises(ValueError) as ei:
                fe.submit("x", cfg_reuse=2, **apg).result(timeout=5)
            assert "cfg_reuse" in str(ei.value) and "apg_eta" in str(ei.value)
    finally:
        fe.close()


def test_header_and_binding_declare_the_reuse_entries():
    import ctypes as C
    from vietvoice_tts_amd import runtime
    hdr = open(os.path.join(os.path.dirname(HERE), "include", "vvtts.h")).read()
    declared = set(re.findall(r"\b(vv_[a-z0-9_]+)\s*\(", hdr))
    lib = runtime.load_library()
    for name in ("vv_transformer_steps_reuse", "vv_transformer_reuse_ws_bytes", "vv_ode_stage_reuse", "vv_cfg_drift_reduce"):
        assert name in declared and name in runtime.EXPORTS and hasattr(lib, name)
    assert C.sizeof(runtime.vv_reuse_args) == 16 and C.sizeof(runtime.vv_reuse_stage_args) == 24
    assert C.sizeof(runtime.vv_cfg_drift_args) == 8 + 16 + 8 + 8 + 8 + 8 + 8 + 8 + 8 + 8
    assert (runtime.REUSE_LOAD, runtime.REUSE_STORE) == (1, 2)
    assert re.search(r"#define VV_REUSE_LOAD 1\b", hdr) and re.search(r"#define VV_REUSE_STORE 2\b", hdr)


# ------------------------------------------------------------------------------------------------ 5. the drift report's mirror
def test_drift_mirror_against_a_plain_float64_loop():
    """Three ragged items (31, 32 and 45 frames: below, at and above a tile), n_mel 100.  The mirror adds in the kernel's order, the plain
    loop row by row: the two agree to the rounding of a float64 sum of that many non-negative terms (n * 2^-53 relative), not bit for bit."""
    rng = np.random.default_rng(21)
    M = 100
    for frames in (31, 32, 45):
        pc = rng.standard_normal((frames, M)).astype(np.float32)
        pu = rng.standard_normal((frames, M)).astype(np.float32)
        old = (pc - pu + 0.1 * rng.standard_normal((frames, M))).astype(np.float32)
        for d_old in (None, old):
            e2, n2 = U.drift_mirror(pc, pu, d_old)
            pe2, pn2 = U.drift_plain(pc, pu, d_old)
            tol = frames * M * 2.0 ** -53
            assert abs(n2 - pn2) <= tol * pn2 and abs(e2 - pe2) <= tol * pe2
            assert (e2 == 0.0) == (d_old is None) and n2 > 0.0
    # an item is a function of its own rows: the same rows give the same bits whatever stands around them
    pc = rng.standard_normal((45, M)).astype(np.float32)
    pu = rng.standard_normal((45, M)).astype(np.float32)
    assert U.drift_mirror(pc, pu, None) == U.drift_mirror(pc.copy(), pu.copy(), None)
    assert U.drift_mirror(pc, pc, None) == (0.0, 0.0)
