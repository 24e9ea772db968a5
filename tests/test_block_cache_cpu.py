"""N23 block caching, the host side: the option's checks, the schedule on hand-worked plans, the report's mirror against plain loops, the
config round trip, and the two new kernels compiled for the host under sanitizers (tools/elementwise_host_check.py).  Needs no GPU."""
import json

import numpy as np
import pytest

from tests import block_cache_util as U
from tests.host_check_util import tool


def _spec():
    from vietvoice_tts_amd import model_spec
    return model_spec


# ------------------------------------------------------------------------------------------------ the option
def test_check_block_cache():
    ms = _spec()
    assert ms.check_block_cache(None, 22) is None
    assert ms.check_block_cache((4, 20, 2), 22) == (4, 20, 2)
    assert ms.check_block_cache([0, 22, 1], 22) == (0, 22, 1)                   # a list (from JSON) becomes the tuple
    assert ms.check_block_cache((np.int64(1), np.int32(2), 3), 2) == (1, 2, 3)
    for bad in ((4, 4, 2), (5, 4, 2), (-1, 4, 2), (0, 23, 2), (0, 4, 0), (0, 4), (0, 4, 2, 1), (0.0, 4, 2), (True, 4, 2), "042", 7):
        with pytest.raises(ValueError, match="block_cache"):
            ms.check_block_cache(bad, 22)
    assert (ms.BLOCK_FULL, ms.BLOCK_STORE, ms.BLOCK_LIGHT) == (U.FULL, U.STORE, U.LIGHT) == (0, 1, 2)


def _cfg(tmp, **kw):
    from vietvoice_tts_amd.core import ModelConfig
    return ModelConfig(model_cache_dir=str(tmp), synthetic_model=True, model_spec="tiny", **kw)


def test_config_refusals_and_round_trip(tmp_path):
    from vietvoice_tts_amd.core import ModelConfig
    c = _cfg(tmp_path)
    assert c.block_cache is None and c.block_cache_interval is None and c.block_cache_report is False
    c = _cfg(tmp_path, block_cache=[1, 2, 2], block_cache_interval=[0.1, 0.9], block_cache_report=1)
    assert c.block_cache == (1, 2, 2) and c.block_cache_interval == (0.1, 0.9) and c.block_cache_report is True
    d = json.loads(json.dumps(c.to_dict()))                                      # tuples come back as lists
    c2 = ModelConfig.from_dict(d)
    assert c2.block_cache == (1, 2, 2) and c2.block_cache_interval == (0.1, 0.9) and c2.to_dict() == c.to_dict()
    for kw in (dict(cfg_interval=(0.1, 0.9)), dict(cfg_reuse=2), dict(apg_eta=0.5), dict(apg_norm=2.0)):
        with pytest.raises(ValueError, match="block_cache cannot be combined"):
            _cfg(tmp_path, block_cache=(1, 2, 2), **kw)
    _cfg(tmp_path, block_cache=(1, 2, 2), cfg_reuse=1, apg_eta=1.0, cfg_strength=0.0)      # the "off" values are no conflict
    with pytest.raises(ValueError, match="need block_cache"):
        _cfg(tmp_path, block_cache_report=True)
    with pytest.raises(ValueError, match="need block_cache"):
        _cfg(tmp_path, block_cache_interval=(0.0, 1.0))
    with pytest.raises(ValueError, match="block_cache"):
        _cfg(tmp_path, block_cache=(2, 1, 2))
    with pytest.raises(ValueError, match="cfg_interval"):                        # the interval's own check, under its usual wording
        _cfg(tmp_path, block_cache=(1, 2, 2), block_cache_interval=(0.9, 0.1))


def test_request_options_are_untouched():
    """Block caching is an engine option: a request's record has no field for it."""
    from vietvoice_tts_amd.request_options import RequestOptions
    assert not [f for f in RequestOptions.__dataclass_fields__ if "block" in f]


# ------------------------------------------------------------------------------------------------ the schedule
def _plan(method, nfe=9):
    ms = _spec()
    return ms.ode_plan(nfe, ms.ModelSpec.tiny().sway_coef, method)


def test_schedule_on_hand_worked_plans():
    sched = _spec().block_cache_schedule
    e = _plan("euler")                                                           # 8 evaluations
    assert sched(e, 1).tolist() == [0] * 8
    assert sched(e, 1, None, True).tolist() == [1] * 8
    assert sched(e, 2).tolist() == [1, 2, 1, 2, 1, 2, 1, 2]
    assert sched(e, 3).tolist() == [1, 2, 2, 1, 2, 2, 1, 2]
    assert sched(e, 8).tolist() == [1, 2, 2, 2, 2, 2, 2, 2]
    assert sched(e, 9).tolist() == [1] + [2] * 7
    assert sched(_plan("euler", 10), 3).tolist() == [1, 2, 2, 1, 2, 2, 1, 2, 2]
    assert sched(_plan("euler", 8), 2).tolist() == [1, 2, 1, 2, 1, 2, 0]         # the last full evaluation has no light one behind it: no store
    assert sched(_plan("euler", 8), 2, None, True).tolist() == [1, 2, 1, 2, 1, 2, 1]     # ... under a report every full one stores
    assert sched(_plan("ab2"), 2).tolist() == sched(e, 2).tolist()               # a multistep plan has Euler's evaluations
    r = _plan("rk4", 3)                                                          # 2 steps x 4 stages; the count runs over evaluations
    assert sched(r, 2).tolist() == [1, 2] * 4 and sched(r, 3).tolist() == [1, 2, 2, 1, 2, 2, 1, 2]
    # an interval: the candidates are the evaluations inside it, both edges inclusive; the count starts at the first candidate
    t = [float(v) for v in e.t]
    assert all(t[i] <= t[i + 1] for i in range(7)) and t[0] == 0.0
    iv = (t[2], t[5])
    assert sched(e, 2, iv).tolist() == [0, 0, 1, 2, 1, 2, 0, 0]
    assert sched(e, 3, iv).tolist() == [0, 0, 1, 2, 2, 0, 0, 0]                  # candidate 3 is full with nothing light behind it
    assert sched(e, 3, iv, True).tolist() == [1, 1, 1, 2, 2, 1, 1, 1]
    assert sched(e, 2, (t[7] + 1e-4, 1.0)).tolist() == [0] * 8                   # an interval without an evaluation: nothing is skipped
    assert sched(e, 2, (0.0, 0.0)).tolist() == [0] * 8                           # one candidate: always full
    for bad in (0, -1, 1.5, True, None):
        with pytest.raises(ValueError, match="every"):
            sched(e, bad)


@pytest.mark.parametrize("method,nfe", [("euler", 8), ("euler", 32), ("midpoint", 5), ("heun2", 5), ("heun3", 4), ("rk4", 3), ("rk4", 6), ("ab2", 8), ("ab3", 9)])
def test_schedule_equals_the_independent_rule(method, nfe):
    sched = _spec().block_cache_schedule
    p = _plan(method, nfe)
    t = [float(v) for v in p.t]
    assert all(t[i] <= t[i + 1] for i in range(len(t) - 1))                      # what makes the candidates contiguous
    for every in (1, 2, 3, 5):
        for iv in (None, (0.0, 1.0), (0.05, 0.7), (0.3, 0.31), (t[1], t[-2])):
            for report in (False, True):
                got = sched(p, every, iv, report).tolist()
                assert got == U.schedule(t, every, iv, report), (method, nfe, every, iv, report)
                assert U.check_modes(got, (0, 1), 1, len(t)) is None             # a light evaluation always has a store in front of it
                if every == 1:
                    assert 2 not in got
                for e_, m in enumerate(got):
                    if m == 2:
                        assert got[e_ - 1] in (1, 2) and e_ > 0


def test_blocks_run_and_the_restated_refusals():
    assert U.blocks_run([1, 2, 1, 2], (4, 20), 22) == [22, 6, 22, 6] and sum(U.blocks_run([1, 2] * 16, (4, 20), 22)) / 32 == 14
    ok = [1, 2, 1, 2]
    assert U.check_modes(ok, (1, 3), 4, 4) is None
    assert U.check_modes(ok, (3, 3), 4, 4) == "span" and U.check_modes(ok, (0, 5), 4, 4) == "span"
    assert U.check_modes(ok, (1, 3), 4, 5) == "n_modes"
    assert U.check_modes([1, 3, 1, 2], (1, 3), 4, 4) == "value"
    assert U.check_modes([2, 1, 2, 0], (1, 3), 4, 4) == "2 before 1" and U.check_modes([0, 2, 1, 2], (1, 3), 4, 4) == "2 before 1"
    assert U.check_modes(ok, (1, 3), 4, 4, e0=2) == "step0" and U.check_modes([1, 2, 1, 1], (1, 3), 4, 4, e0=2) is None


# ------------------------------------------------------------------------------------------------ the report's mirror
@pytest.mark.parametrize("D", [4, 128, 1024])
def test_mirror_equals_plain_loops(D):
    rng = np.random.default_rng(5 + D)
    for frames in (0, 1, U.TILE - 1, U.TILE, U.TILE + 1, 2 * U.TILE + 13):
        if D == 1024 and frames > U.TILE + 1:
            continue
        a = rng.standard_normal((frames, D)).astype(np.float32)
        b = (a + 0.25 * rng.standard_normal((frames, D))).astype(np.float32)
        got, plain = U.report_mirror(a, b), U.report_plain(a, b)
        assert np.allclose(got, plain, rtol=1e-12, atol=0.0), (D, frames, got, plain)
        first = U.report_mirror(a, None)
        assert first[0] == 0.0 and first[1] == got[1]                            # N2 does not depend on what was stored before
        assert U.report_mirror(a, a) == (0.0, got[1])
        if frames == 0:
            assert got == (0.0, 0.0)


def test_span_expected_and_bf16_round():
    import torch
    x, d1, d2, buf = (a[U.GUARD: -U.GUARD] for a in U.span_operands(3, 128))
    X = (torch.from_numpy(x) + torch.from_numpy(d1)) + torch.from_numpy(d2)
    assert np.array_equal(U.span_expected(U.MARK, x, d1, d2, buf)[1], X.numpy())
    assert np.array_equal(U.span_expected(U.DIFF, x, d1, d2, buf)[1], (X - torch.from_numpy(buf)).numpy())
    assert np.array_equal(U.span_expected(U.APPLY, x, None, None, buf)[0], (torch.from_numpy(x) + torch.from_numpy(buf)).numpy())
    assert np.array_equal(U.bf16_round(d1), torch.from_numpy(d1).to(torch.bfloat16).float().numpy())


# ------------------------------------------------------------------------------------------------ the kernels on the host, under sanitizers
@pytest.mark.parametrize("san", ["asan", "tsan"])
def test_new_kernels_on_the_shim_equal_the_mirror_with_no_report(san, tmp_path):
    """block_span_kernel (every mode and dtype; two workgroups, 43 trips of the grid-stride loop) and the report's two kernels (sequences
    of 0, 31, 32, 33 and 45 rows, an overstated length, a row_start past the rows) on exact-size heap blocks: a stand-alone program, one OS
    thread per GPU thread; nothing is loaded into this process under a sanitizer."""
    t = tool("elementwise")
    cxx = t.find_cxx()
    if cxx is None:
        pytest.skip("no host C++ compiler found")
    exe = t.build(cxx, str(tmp_path), san)
    res = list(t.block_cache_cases(exe, str(tmp_path), reduced=True))           # a sanitizer report, a non-zero exit or a run past its time limit raises
    assert len(res) >= 15 and not [label for label, ok in res if not ok]
