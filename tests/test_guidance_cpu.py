"""N8 host side (no GPU): the guidance mask on hand-worked plans, the config field and the front end's validation."""
import os
import re

import pytest
import torch

from vietvoice_tts_amd.model_spec import OdePlan, check_cfg_interval, guidance_mask, ode_plan

HERE = os.path.dirname(os.path.abspath(__file__))


def _plan(t, s=1):
    t = torch.tensor(t, dtype=torch.float32)
    return OdePlan(t, torch.full((t.numel() // s,), 0.25), ((0.0,),) * s, (1.0,) + (0.0,) * (s - 1), s)


def test_mask_edges_are_inclusive():
    """Times that fp32 holds exactly, so the edges are hit, not approached: 0, 1/4, 1/2, 3/4."""
    plan = _plan([0.0, 0.25, 0.5, 0.75])
    m = guidance_mask(plan, (0.25, 0.5), [2.0, 2.0])
    assert m.dtype == torch.uint8 and m.shape == (4, 2)
    assert m.tolist() == [[0, 0], [1, 1], [1, 1], [0, 0]]
    assert guidance_mask(plan, (0.5, 0.5), [2.0]).tolist() == [[0], [0], [1], [0]]          # lo == hi: one point
    assert guidance_mask(plan, (0.26, 0.49), [2.0]).tolist() == [[0], [0], [0], [0]]        # nothing inside: all zero, not None
    # the fp32 time is compared as a double: 0.1f = 0.100000001490116... lies above an edge of 0.1
    assert guidance_mask(_plan([0.1]), (0.0, 0.1), [1.0]).tolist() == [[0]]
    assert guidance_mask(_plan([0.1]), (0.1, 1.0), [1.0]) is None


def test_mask_zero_strength_and_none():
    plan = _plan([0.0, 0.25, 0.5, 0.75])
    assert guidance_mask(plan, None, [2.0, 1.0, -0.5]) is None                                # all ones
    assert guidance_mask(plan, (0.0, 1.0), [2.0, 1.0]) is None
    m = guidance_mask(plan, None, [2.0, 0.0, 3.0])                                            # a zero strength is never guided
    assert m.tolist() == [[1, 0, 1]] * 4
    assert guidance_mask(plan, None, [-0.0]).tolist() == [[0]] * 4
    m = guidance_mask(plan, (0.25, 0.75), [0.0, 2.0])
    assert m.tolist() == [[0, 0], [0, 1], [0, 1], [0, 1]]
    # one interval per item
    m = guidance_mask(plan, [(0.0, 0.25), None, (0.5, 1.0)], [1.0, 1.0, 1.0])
    assert m.tolist() == [[1, 1, 0], [1, 1, 0], [0, 1, 1], [0, 1, 1]]
    assert guidance_mask(plan, [None, None], [1.0, 1.0]) is None
    with pytest.raises(ValueError):
        guidance_mask(plan, [None, None, None], [1.0, 1.0])
    with pytest.raises(ValueError):
        guidance_mask(plan, (0.5, 0.25), [1.0])


def test_mask_follows_the_stage_times_of_a_runge_kutta_plan():
    """Row e = step * s + stage.  Midpoint on the uniform 3-point grid: stages at t_n and t_n + h / 2 = 0, 0.25, 0.5, 0.75."""
    plan = ode_plan(3, 0.0, "midpoint")
    assert plan.s == 2 and [float(v) for v in plan.t] == [0.0, 0.25, 0.5, 0.75]
    assert guidance_mask(plan, (0.2, 0.6), [2.0]).tolist() == [[0], [1], [1], [0]]            # an edge inside each step
    # the project's rk4 (the 3/8 rule) on two points: stages at 0, 1/3, 2/3, 1
    plan = ode_plan(2, 0.0, "rk4")
    assert [round(float(v), 6) for v in plan.t] == [0.0, 0.333333, 0.666667, 1.0]
    assert guidance_mask(plan, (0.5, 1.0), [2.0]).tolist() == [[0], [0], [1], [1]]
    assert guidance_mask(plan, (0.3, 0.7), [2.0, 0.0]).tolist() == [[0, 0], [1, 0], [1, 0], [0, 0]]
    assert guidance_mask(plan, (0.0, 1.0), [2.0]) is None


def test_check_cfg_interval():
    assert check_cfg_interval(None) is None
    assert check_cfg_interval([0, 1]) == (0.0, 1.0) and check_cfg_interval((0.3, 0.3)) == (0.3, 0.3)
    for bad in ((0.5, 0.2), (-0.1, 0.5), (0.2, 1.1), (float("nan"), 0.5), (0.0, float("inf")), (0.1,), (0.1, 0.2, 0.3), 0.5, "ab"):
        with pytest.raises(ValueError):
            check_cfg_interval(bad)


def test_model_config_interval(tmp_path):
    from vietvoice_tts_amd.core import ModelConfig
    kw = dict(model_cache_dir=str(tmp_path), synthetic_model=True, model_spec="tiny")
    assert ModelConfig(**kw).cfg_interval is None
    for bad in ((0.8, 0.2), (-0.5, 0.5), (0.0, 1.5), (float("nan"), 1.0), (0.5,)):
        with pytest.raises(ValueError):
            ModelConfig(cfg_interval=bad, **kw)
    cfg = ModelConfig(cfg_interval=(0.2, 0.8), cfg_strength=1.5, **kw)
    d = cfg.to_dict()
    assert d["cfg_interval"] == (0.2, 0.8)
    back = ModelConfig.from_dict(d)
    assert back.to_dict() == d
    import json
    again = ModelConfig.from_dict(json.loads(json.dumps(d)))                                  # JSON turns the pair into a list
    assert again.cfg_interval == (0.2, 0.8) and again.to_dict() == d
    names = list(d)
    assert names[:4] == ["model_url", "model_cache_dir", "model_filename", "nfe_step"] and names.index("cfg_interval") > names.index("cfg_strength")


def test_header_and_binding_declare_the_guided_entries():
    import ctypes as C
    from vietvoice_tts_amd import runtime
    hdr = open(os.path.join(os.path.dirname(HERE), "include", "vvtts.h")).read()
    declared = set(re.findall(r"\b(vv_[a-z0-9_]+)\s*\(", hdr))
    lib = runtime.load_library()
    for name in ("vv_transformer_steps_guided", "vv_transformer_guided_ws_bytes", "vv_ode_stage_guided"):
        assert name in declared and name in runtime.EXPORTS and hasattr(lib, name)
    # no field was added to the two argument structs
    assert C.sizeof(runtime.vv_steps_args) == 8 + 9 * 8 + 8 + 8 + 8 + 8
    assert C.sizeof(runtime.vv_ode_stage_args) == 8 + 8 + 16 + 24 + 16 + 8 + 8 + 8 + 8 + 8 + 8


def test_batching_frontend_refuses_a_bad_interval():
    from vietvoice_tts_amd.batching import BatchingFrontend
    fe = BatchingFrontend(engine=None, overlap=False)
    try:
        for bad in ((0.9, 0.1), (0.0, 2.0), (float("nan"), 0.5), 3):
            with pytest.raises(ValueError):
                fe.submit("x", cfg_interval=bad).result(timeout=5)
    finally:
        fe.close()
