"""N11, adaptive projected guidance, the parts that need no GPU: the value checks, the config fields, the front end's
per-request validation, the four exports, and the rule itself on a hand-worked item in exact fractions."""
import os
import re
from fractions import Fraction as F

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
NEW_EXPORTS = ["vv_transformer_steps_apg", "vv_transformer_apg_ws_bytes", "vv_apg_coef", "vv_ode_stage_apg"]


# ------------------------------------------------------------------------------------------------ check_apg
@pytest.mark.parametrize("eta,norm,want", [
    (None, None, None), (1.0, None, None), (1, None, None),                     # off: the plain rule
    (0.0, None, (0.0, None)), (0, None, (0.0, None)), (0.5, 2, (0.5, 2.0)), (None, 0.3, (1.0, 0.3)), (1.0, 0.3, (1.0, 0.3)),
    (-0.5, None, (-0.5, None)), (3.0, 1e-6, (3.0, 1e-6)),
])
def test_check_apg_accepts(eta, norm, want):
    from vietvoice_tts_amd.model_spec import check_apg
    assert check_apg(eta, norm) == want


@pytest.mark.parametrize("eta,norm", [
    (float("nan"), None), (float("inf"), None), (-float("inf"), 1.0), ("0.5", None), (True, None), ([0.0], None),
    (None, 0.0), (None, -1.0), (0.0, float("nan")), (0.0, float("inf")), (None, "1"), (None, False), (0.5, (1.0,)),
])
def test_check_apg_refuses(eta, norm):
    from vietvoice_tts_amd.model_spec import check_apg
    with pytest.raises(ValueError):
        check_apg(eta, norm)


# ------------------------------------------------------------------------------------------------ ModelConfig
def _config(tmp, **kw):
    from vietvoice_tts_amd.core import ModelConfig
    return ModelConfig(model_cache_dir=str(tmp), synthetic_model=True, model_spec="tiny", **kw)


def test_model_config_fields(tmp_path):
    from vietvoice_tts_amd.core import ModelConfig
    c = _config(tmp_path)
    assert c.apg_eta is None and c.apg_norm is None                              # defaults: nothing changes
    c = _config(tmp_path, apg_eta=0, apg_norm=2)
    assert (c.apg_eta, c.apg_norm) == (0.0, 2.0) and isinstance(c.apg_eta, float) and isinstance(c.apg_norm, float)
    d = c.to_dict()
    assert d["apg_eta"] == 0.0 and d["apg_norm"] == 2.0
    back = ModelConfig.from_dict(d)
    assert back.to_dict() == d
    import json
    assert ModelConfig.from_dict(json.loads(json.dumps(d))).to_dict() == d       # through JSON as well
    for bad in (dict(apg_eta=float("nan")), dict(apg_eta=float("inf")), dict(apg_norm=0.0), dict(apg_norm=-0.1), dict(apg_norm=float("inf")),
                dict(apg_eta="0")):
        with pytest.raises(ValueError):
            _config(tmp_path, **bad)


def test_sessions_and_manager_carry_the_fields():
    """HipSession takes the two values the way it takes cfg_interval (no engine is needed to see that)."""
    from vietvoice_tts_amd.core.model import HipSession
    s = HipSession(None, "transformer", None, 1, None, None, apg_eta=0.0, apg_norm=0.5)
    assert (s.apg_eta, s.apg_norm) == (0.0, 0.5)
    s = HipSession(None, "transformer", None)
    assert (s.apg_eta, s.apg_norm) == (None, None)


# ------------------------------------------------------------------------------------------------ BatchingFrontend.submit
class _NoEngine:
    """submit() validates before anything reaches the engine: none is needed."""
    class model_session_manager:
        engine = None


def test_submit_validates_the_requests_own_values():
    from vietvoice_tts_amd.batching import BatchingFrontend
    fe = BatchingFrontend(_NoEngine(), max_wait_ms=1.0)
    try:
        for bad in (dict(apg_eta=float("nan")), dict(apg_eta=float("inf")), dict(apg_norm=0.0), dict(apg_norm=-2.0), dict(apg_eta="x"),
                    dict(apg_eta=0.0, apg_norm=float("nan"))):
            fut = fe.submit("xin chào", **bad)
            assert fut.done() and isinstance(fut.exception(timeout=1), ValueError), bad
    finally:
        fe.close()


# ------------------------------------------------------------------------------------------------ the C ABI
def test_header_version_script_and_exports_agree():
    from vietvoice_tts_amd import runtime
    root = os.path.dirname(HERE)
    hdr = open(os.path.join(root, "include", "vvtts.h")).read()
    declared = set(re.findall(r"\b(vv_[a-z0-9_]+)\s*\(", hdr))
    vmap = open(os.path.join(root, "vietvoice-tts_amd", "csrc", "vvtts.map")).read()
    patterns = re.findall(r"global:\s*([^;]+);", vmap)
    assert patterns, "the version script names its exports"
    import fnmatch
    for name in NEW_EXPORTS:
        assert name in declared, name
        assert name in runtime.EXPORTS, name
        assert any(fnmatch.fnmatchcase(name, p.strip()) for pat in patterns for p in pat.split()), name
    lib = runtime.load_library()                                                 # dlopen on a CPU-only host: the symbols are there
    for name in NEW_EXPORTS:
        assert hasattr(lib, name)
    assert re.search(r"#define\s+VV_PROF_NCLASS\s+18\b", hdr)
    assert int(re.search(r"#define\s+VV_APG_TILE\s+(\d+)", hdr).group(1)) == runtime.APG_TILE
    # the struct layouts the Python side mirrors
    for struct, cls in (("vv_apg_args", runtime.vv_apg_args), ("vv_apg_coef_args", runtime.vv_apg_coef_args),
                        ("vv_apg_stage_args", runtime.vv_apg_stage_args)):
        body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (struct, struct), hdr, re.S).group(1)
        body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
        names = []
        for decl in body.split(";"):
            decl = decl.strip()
            if decl:
                names += [re.sub(r"[\s*]", "", v).split("[")[0] for v in re.sub(r"^(const\s+)?\w+\s*\*?", "", decl, count=1).split(",")]
        assert names == [f[0] for f in cls._fields_], (struct, names)


# ------------------------------------------------------------------------------------------------ the rule, in exact fractions
def apg_exact(pc, pu, xe, t, g, eta, r):
    """DESIGN N11 on one item in exact rational arithmetic (r None = no cap; the cap compares squares, so no root is taken unless the
    item is capped -- the worked example below is chosen so that the root is rational)."""
    D = [a - b for a, b in zip(pc, pu)]
    d = [x + (1 - t) * a for x, a in zip(xe, pc)]
    S1, S2, S3 = sum(a * b for a, b in zip(D, d)), sum(a * a for a in d), sum(a * a for a in D)
    n = len(pc)
    ms = (1 - t) ** 2 * S3 / n                                                   # the mean square of the data-space difference
    s = F(1)
    if r is not None and ms > r * r:
        root = F(int(round(float(ms) ** 0.5 * 1000)), 1000)
        assert root * root == ms, "the example keeps the RMS rational"
        s = r / root
    A = g * s
    Cc = F(0) if S2 == 0 else g * s * (eta - 1) * S1 / S2
    k = [a + A * dd + Cc * e for a, dd, e in zip(pc, D, d)]
    return k, A, Cc, d, D


# a 2-frame item with two columns: pc, pu, the state; t = 1/2
PC = [F(1), F(2), F(-1), F(0)]
PU = [F(0), F(1), F(1), F(-2)]                 # D = (1, 1, -2, 2): S3 = 10
XE = [F(1, 2), F(0), F(1, 2), F(1)]            # d = x + pc / 2 = (1, 1, 0, 1): S2 = 3, S1 = 1 + 1 + 0 + 2 = 4
T, G = F(1, 2), F(2)


def test_rule_by_hand():
    k, A, Cc, d, D = apg_exact(PC, PU, XE, T, G, F(1, 2), None)
    assert d == [1, 1, 0, 1] and D == [1, 1, -2, 2]
    assert A == 2 and Cc == F(2) * (F(1, 2) - 1) * F(4, 3) == F(-4, 3)
    assert k == [1 + 2 - F(4, 3), 2 + 2 - F(4, 3), -1 - 4, 0 + 4 - F(4, 3)]
    # the same through the decomposition: k = pc + g (orth + eta par), par = (S1 / S2) d
    par = [F(4, 3) * v for v in d]
    orth = [a - b for a, b in zip(D, par)]
    assert sum(a * b for a, b in zip(orth, d)) == 0
    assert k == [a + G * (o + F(1, 2) * p) for a, o, p in zip(PC, orth, par)]


def test_eta_one_without_a_cap_is_plain_cfg():
    k, A, Cc, _, D = apg_exact(PC, PU, XE, T, G, F(1), None)
    assert A == G and Cc == 0 and k == [a + G * dd for a, dd in zip(PC, D)]


def test_eta_zero_removes_the_parallel_part_exactly():
    k, _, _, d, _ = apg_exact(PC, PU, XE, T, G, F(0), None)
    assert sum((a - b) * e for a, b, e in zip(k, PC, d)) == 0                    # (k - pc) . d = 0
    pc, pu, xe = [F(3), F(1), F(0), F(0)], [F(-1), F(1), F(0), F(0)], [F(0), F(1), F(0), F(0)]    # RMS = 1 (rational): capped at 1/4
    k, A, _, d, _ = apg_exact(pc, pu, xe, T, G, F(0), F(1, 4))
    assert A == G * F(1, 4) and sum((a - b) * e for a, b, e in zip(k, pc, d)) == 0


def test_cap_scales_the_difference_to_the_limit():
    pc = [F(3), F(0), F(0), F(0)]
    pu = [F(-1), F(0), F(0), F(0)]                                               # D = (4, 0, 0, 0): ms = (1/4) 16 / 4 = 1, RMS = 1
    xe = [F(0), F(1), F(0), F(0)]
    _, A, Cc, d, D = apg_exact(pc, pu, xe, T, G, F(0), F(1, 2))
    assert A == G * F(1, 2)                                                      # s = r / RMS = 1/2
    assert d == [F(3, 2), 1, 0, 0] and Cc == G * F(1, 2) * (0 - 1) * F(6) / F(13, 4)
    _, A1, _, _, _ = apg_exact(pc, pu, xe, T, G, F(0), F(1))                     # exactly at the edge: not capped
    assert A1 == G
    _, A2, _, _, _ = apg_exact(pc, pu, xe, F(1), G, F(0), F(1, 1000))            # t = 1: the data-space difference vanishes, never capped
    assert A2 == G


def test_s2_zero_gives_no_parallel_term():
    pc, pu = [F(2), F(-2)], [F(1), F(1)]
    xe = [F(-1), F(1)]                                                           # d = x + pc / 2 = 0
    k, A, Cc, d, D = apg_exact(pc, pu, xe, T, G, F(0), None)
    assert d == [0, 0] and Cc == 0 and k == [a + G * dd for a, dd in zip(pc, D)]


def test_reference_of_the_gpu_tests_follows_the_same_rule():
    """tests/test_apg_gpu.py's float64 coef_ref against the exact fractions above (it is the yardstick of the device kernels)."""
    import numpy as np
    from tests.test_apg_gpu import coef_ref
    for eta, r in ((F(1, 2), None), (F(0), F(1, 4)), (F(1), None), (F(-3, 4), F(1, 2))):
        pc = [F(3), F(0), F(0), F(1, 2)] if r is not None else PC
        pu = [F(-1), F(0), F(0), F(1, 2)] if r is not None else PU
        _, A, Cc, _, _ = apg_exact(pc, pu, XE, T, G, eta, r)
        a, c, _, _ = coef_ref(np.array([float(v) for v in pc]).reshape(2, 2), np.array([float(v) for v in pu]).reshape(2, 2),
                              np.array([float(v) for v in XE]).reshape(2, 2), 0.5, 2.0, float(eta), None if r is None else float(r))
        assert abs(a - float(A)) <= 1e-15 * abs(float(A)) and abs(c - float(Cc)) <= 1e-15 * max(abs(float(Cc)), 1e-300)
