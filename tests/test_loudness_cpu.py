"""N12, loudness normalisation: the host mirror (the specification), its gates, config and front-end plumbing -- nothing here needs a GPU.

The mirror (core/audio_processor.py) runs the device's run decomposition in numpy; tests/loudness_util.py is the independent reference
(scipy.signal.lfilter over the whole signal).  Bounds: q_j within relative 1e-9 (float64 recurrences with pole radius 0.995 amplify
rounding by ~1/(1 - r); 7e-11 at most was seen on the 265,472-sample signal below, in the sub-block of digital silence, where q has
fallen by ten orders; a lost state or a wrong coefficient moves a sub-block by 1e-2).  The signal generator keeps stretches of
digital silence under one sub-block or so: in longer ones q decays by twenty orders per sub-block and its RELATIVE error is no longer
a statement about the filter.  PCM: output_util.lsb_condition (no difference above 1 LSB, at most 1 sample in 10^4)."""
import ctypes
import os
import re
from fractions import Fraction

import numpy as np
import pytest

from tests.loudness_util import TABLE_48K, ref_measure, ref_normalize, ref_subblock_sums, sine, speechlike
from tests.output_util import lsb_condition

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SR = 24000
SUB = SR // 10
ABS = 10.0 ** ((-70 + 0.691) / 10)


def _ap():
    from vietvoice_tts_amd.core import audio_processor
    return audio_processor


# ------------------------------------------------------------------ coefficients and the sine of the Recommendation
def test_coefficients_at_48k_equal_the_table():
    b1, a1, b2, a2 = _ap().k_weighting(48000)
    assert np.abs(b1 - TABLE_48K["shelf_b"]).max() < 1e-13 and np.abs(a1 - TABLE_48K["shelf_a"]).max() < 1e-13
    assert np.array_equal(b2, TABLE_48K["hp_b"]) and np.abs(a2 - TABLE_48K["hp_a"]).max() < 1e-13


@pytest.mark.parametrize("sr,want", [(48000, -3.01), (24000, -2.98)])
def test_full_scale_997_hz_sine(sr, want):
    L, zbar, kept, peak = _ap().measure_loudness(sine(3 * sr, sr), sr)
    print(sr, L, zbar, kept, peak)
    assert abs(L - want) <= 0.01 and kept == 27 and peak == 32767
    assert abs(ref_measure(sine(3 * sr, sr), sr)["lufs"] - want) <= 0.01


def test_tables_hold_the_zero_input_response_of_a_run():
    ap = _ap()
    t = ap.loudness_tables(SR)
    assert t.size == ap.LOUD_TABLE_DOUBLES == 43 and t[42] == ABS and ap._loud_run_lengths(SUB) == (19, 96)
    b1, a1, b2, a2 = ap.k_weighting(SR)
    assert np.array_equal(t[:10], np.concatenate([b1, a1, b2, a2]))
    for M, length in ((t[10:26].reshape(4, 4), 128), (t[26:42].reshape(4, 4), 96)):
        for j in range(4):
            s = [np.float64(i == j) for i in range(4)]
            for _ in range(length):
                _y, s = ap._loud_step(np.float64(0), s, b1, a1, b2, a2)
            assert np.array_equal(M[:, j], np.array(s))
    with pytest.raises(ValueError):
        ap.loudness_tables(22050 + 5)                       # not a multiple of 10 Hz
    with pytest.raises(ValueError):
        ap.loudness_tables(1270)                            # a sub-block shorter than one run


# ------------------------------------------------------------------ the gates, on hand-made sub-block sums with exact answers
def _q(*z):
    """Sub-block sums that make 4 equal neighbours a block of mean square z: q = z * SUB (exact for the dyadic z used here)."""
    return [v * SUB for v in z]


def test_gate_fewer_than_four_sub_blocks():
    gate = _ap().loudness_gate
    assert gate([], SUB) == (0.0, 0) and gate(_q(0.25, 0.25, 0.25), SUB) == (0.0, 0)
    assert gate(_q(0.25, 0.25, 0.25, 0.25), SUB) == (0.25, 1)


def test_gate_everything_below_the_absolute_gate():
    assert _ap().loudness_gate(_q(*[2.0 ** -24] * 12), SUB) == (0.0, 0)            # 6e-8 < ABS = 1.17e-7


def test_gate_relative_gate_drops_exactly_the_quiet_blocks():
    loud, quiet = 0.25, 2.0 ** -10
    q = _q(*([loud] * 8 + [quiet] * 8))
    z = [sum(Fraction(v) for v in q[j: j + 4]) / (4 * SUB) for j in range(13)]      # exact: 5 loud, 3 mixed, 5 quiet blocks
    assert all(v > ABS for v in z)
    gamma = sum(z) / 13 / 10
    keep = [v for v in z if v > gamma]
    assert len(keep) == 8 and all(float(v) == quiet for v in z if v <= gamma)       # exactly the five all-quiet blocks go
    zbar, kept = _ap().loudness_gate(q, SUB)
    assert kept == 8 and zbar == float(sum(keep) / 8)


def test_gate_block_exactly_at_the_absolute_gate_is_not_kept():
    gate = _ap().loudness_gate
    q0 = ABS * (4 * SUB)
    for _ in range(64):                                     # the float whose quotient is exactly ABS
        if q0 / (4 * SUB) == ABS:
            break
        q0 = np.nextafter(q0, np.inf if q0 / (4 * SUB) < ABS else -np.inf)
    assert q0 / (4 * SUB) == ABS
    assert gate([q0, 0, 0, 0], SUB) == (0.0, 0)             # z == ABS: the comparison is strict
    up = np.nextafter(q0, np.inf)
    while up / (4 * SUB) == ABS:
        up = np.nextafter(up, np.inf)
    assert gate([up, 0, 0, 0], SUB) == (up / (4 * SUB), 1)


def test_gate_block_exactly_at_the_relative_gate_is_not_kept():
    gate = _ap().loudness_gate
    a, b = 4 * 2.0 ** -8, 49 * 2.0 ** -8                    # blocks: a once, b four times, zeros between: mean = (a + 4 b) / 5 = 40 * 2^-8
    q = [a * 4 * SUB, 0, 0, 0, 0, 0, 0, b * 4 * SUB, 0, 0, 0]
    assert 0.1 * ((a + 4 * b) / 5) == a                     # Gamma == a exactly, in float64
    assert gate(q, SUB) == (b, 4)                           # a == Gamma is dropped: strict
    q[0] = np.nextafter(q[0], np.inf) * (1 + 1e-12)
    zbar, kept = gate(q, SUB)
    assert kept == 5 and zbar < b


# ------------------------------------------------------------------ the mirror against the sequential scipy reference
@pytest.fixture(scope="module")
def long_signal():
    return speechlike(265472, SR, seed=7)


def test_mirror_sub_block_sums_against_scipy(long_signal):
    ap = _ap()
    for x in (long_signal, speechlike(50003, SR, 3), sine(2 * SR + 17, SR), np.zeros(5000, np.int16)):
        q, want = ap._loud_subblock_sums(x, SR), ref_subblock_sums(x, SR)
        assert q.shape == want.shape == (x.size // SUB,)
        err = np.abs(q - want) / np.where(want == 0, 1.0, np.abs(want))
        print(x.size, "largest relative difference of a sub-block sum", err.max(initial=0))
        assert np.all(np.abs(q - want) <= 1e-9 * np.abs(want))


def test_mirror_is_independent_of_what_follows_and_of_the_tail(long_signal):
    """Causal and cut at sub-block starts: a prefix measures the same sub-blocks bit for bit, the incomplete tail is never measured."""
    ap = _ap()
    q = ap._loud_subblock_sums(long_signal, SR)
    for n in (SUB * 7, SUB * 7 + 1, SUB * 8 - 1):
        assert np.array_equal(ap._loud_subblock_sums(long_signal[:n], SR), q[:7])


@pytest.mark.parametrize("target,peak", [(-23.0, -1.0), (-16.0, -1.0), (-30.0, -6.0), (-5.0, 0.0)])
def test_mirror_pcm_against_scipy(long_signal, target, peak):
    ap = _ap()
    for x in (long_signal, speechlike(12000, SR, 5)):
        want, m, g, limited = ref_normalize(x, SR, target, peak)
        got = ap.normalize_loudness(x, SR, target, peak)
        L, zbar, kept, pk = ap.measure_loudness(x, SR)
        print(x.size, target, peak, "gain", g, "limited", limited, "differing", lsb_condition(got, want))
        assert kept == m["kept"] > 0 and pk == m["peak"] and abs(L - m["lufs"]) < 1e-9
        if not limited:
            assert abs(ap.measure_loudness(got, SR)[0] - target) < 0.01
        else:
            assert np.abs(got.astype(np.int32)).max() <= 32767 * 10 ** (peak / 20)


def test_gain_is_one_and_the_samples_are_copied():
    ap = _ap()
    x = speechlike(12000, SR, 5)
    for pcm, target in ((x[:2000], -23.0), (np.zeros(12000, np.int16), -23.0), (x, None),
                        (np.random.default_rng(0).integers(-3, 4, 12000).astype(np.int16), -23.0)):
        assert np.array_equal(ap.normalize_loudness(pcm, SR, target), pcm)
    lone = np.zeros(100, np.int16)
    lone[50] = -32768
    assert ap.measure_loudness(lone, SR)[3] == 32768                               # |-32768| = 32768, an exact integer
    assert ap.loudness_gain(0.5, 3, 0, 1.0, 100.0) == 1.0 and ap.loudness_gain(0.5, 0, 9, 1.0, 100.0) == 1.0
    assert ap.loudness_gain(0.25, 3, 100, 1.0, 1e9) == 2.0 and ap.loudness_gain(0.25, 3, 100, 1.0, 150.0) == 1.5
    with pytest.raises(ValueError):
        ap.normalize_loudness(x.astype(np.float32), SR, -23.0)


# ------------------------------------------------------------------ config, front end, stream
def test_config_validation_and_round_trip(tmp_path):
    from vietvoice_tts_amd.core import ModelConfig
    base = dict(model_cache_dir=str(tmp_path), synthetic_model=True, model_spec="tiny")
    c = ModelConfig(**base)
    assert c.output_loudness is None and c.output_peak_dbfs == -1.0
    c = ModelConfig(output_loudness=-23, output_peak_dbfs=-2, **base)
    d = c.to_dict()
    assert d["output_loudness"] == -23.0 and d["output_peak_dbfs"] == -2.0 and isinstance(d["output_loudness"], float)
    assert ModelConfig.from_dict(d).to_dict() == d
    for ok in (dict(output_loudness=-60), dict(output_loudness=-5), dict(output_peak_dbfs=0), dict(output_peak_dbfs=-20)):
        ModelConfig(**base, **ok)
    for bad in (dict(output_loudness=-60.5), dict(output_loudness=-4.9), dict(output_loudness=float("nan")), dict(output_loudness="loud"),
                dict(output_loudness=True), dict(output_peak_dbfs=0.1), dict(output_peak_dbfs=-21), dict(output_peak_dbfs=None),
                dict(output_peak_dbfs=float("nan"))):
        with pytest.raises(ValueError):
            ModelConfig(**base, **bad)


def test_front_end_refuses_a_bad_loudness():
    from vietvoice_tts_amd.batching import BatchingFrontend
    fe = BatchingFrontend(engine=None, overlap=False)
    try:
        for bad in (-61, -4, float("nan"), "x", True):
            with pytest.raises(ValueError):
                fe.submit("x", loudness=bad).result(timeout=5)
    finally:
        fe.close()


@pytest.fixture(scope="module")
def cpu_engine(tmp_path_factory):
    from vietvoice_tts_amd.core import ModelConfig, TTSEngine
    from oracle.vv_oracle import Oracle, OracleSession
    d = tmp_path_factory.mktemp("models")
    cfg = ModelConfig(model_cache_dir=str(d), synthetic_model=True, model_spec="tiny", nfe_step=3, max_chunk_duration=8.0)

    def factory(spec, weights, config):
        orc = Oracle(spec, weights, nfe_step=config.nfe_step)
        return {k: OracleSession(orc, k, seed=config.random_seed) for k in ("preprocess", "transformer", "decode")}
    eng = TTSEngine(cfg, session_factory=factory)
    yield eng
    eng.cleanup()


def _reseed(eng):
    import torch
    for sess in eng.model_session_manager.sessions.values():
        sess.gen = torch.Generator().manual_seed(123)


TEXT = "Hôm nay trời đẹp quá, chúng ta cùng nhau đi dạo quanh hồ nhé. " * 3


def test_engine_and_front_end_apply_the_mirror_on_oracle_sessions(cpu_engine):
    from vietvoice_tts_amd.batching import BatchingFrontend
    from vietvoice_tts_amd.core.audio_processor import lin2ulaw, normalize_loudness, resample_output
    eng = cpu_engine
    _reseed(eng)
    base, _ = eng.synthesize(TEXT)
    assert len(eng._last_plan) > 1
    try:
        eng.config.output_loudness, eng.config.output_peak_dbfs = -23.0, -3.0
        assert not eng._device_output()                      # injected sessions: the host mirror
        _reseed(eng)
        got, _ = eng.synthesize(TEXT)
        want = normalize_loudness(base, SR, -23.0, -3.0)
        assert np.array_equal(got, want)
        eng.config.output_sample_rate, eng.config.output_encoding = 8000, "ulaw"      # after the join, before rate and encoding
        _reseed(eng)
        assert np.array_equal(eng.synthesize(TEXT)[0], lin2ulaw(resample_output(want, SR, 8000)))
        eng.config.output_sample_rate, eng.config.output_encoding = None, "pcm16"
        with pytest.raises(ValueError, match="output_loudness"):                      # before any work: nothing is drawn or synthesised
            eng.synthesize_stream(TEXT)
        eng.config.output_loudness = None
        fe = BatchingFrontend(eng, overlap=False)
        try:
            _reseed(eng)
            own = fe.submit(TEXT, loudness=-30.0).result(timeout=300)[0]
            _reseed(eng)
            plain = fe.submit(TEXT).result(timeout=300)[0]
        finally:
            fe.close()
        assert np.array_equal(plain, base) and np.array_equal(own, normalize_loudness(base, SR, -30.0, -3.0))
    finally:
        eng.config.output_loudness, eng.config.output_peak_dbfs = None, -1.0
        eng.config.output_sample_rate, eng.config.output_encoding = None, "pcm16"


# ------------------------------------------------------------------ ABI
def test_header_version_script_and_exports_agree():
    from vietvoice_tts_amd import build_ext, runtime
    hdr = open(os.path.join(ROOT, "include", "vvtts.h")).read()
    declared = set(re.findall(r"VV_API\s+[\w\s\*]+?\b(vv_\w+)\s*\(", hdr))
    assert declared == set(runtime.EXPORTS), declared ^ set(runtime.EXPORTS)
    ver = open(os.path.join(ROOT, "vietvoice-tts_amd", "csrc", "vvtts.map")).read()
    globs = [g.strip() for g in re.findall(r"global:\s*([^;]+);", ver)]
    lib = runtime.load_library()
    for name, n_args in (("vv_pcm_loudness", 15), ("vv_pcm_loudness_ws_bytes", 2)):
        assert name in declared and len(runtime.EXPORTS[name][1]) == n_args
        assert any(re.fullmatch(g.replace("*", ".*"), name) for g in globs) and hasattr(lib, name)
    args = [None if t is ctypes.c_void_p else 0 for t in runtime.EXPORTS["vv_pcm_loudness"][1]]
    assert lib.vv_pcm_loudness(*args) == -22                                          # no context: refused before anything else
    assert lib.vv_pcm_loudness_ws_bytes(1000, 3) >= 1000 * (4 * 8 + 8 + 8 + 4) and lib.vv_pcm_loudness_ws_bytes(0, 1) > 0
    assert "vv_loudness" in build_ext.SOURCES
    assert int(re.search(r"#define VV_LOUD_RUN (\d+)", hdr).group(1)) == runtime.LOUD_RUN == _ap().LOUD_RUN == 128
    assert re.search(r"#define\s+VV_PROF_NCLASS\s+18\b", hdr)
    src = open(os.path.join(ROOT, "vietvoice-tts_amd", "csrc", "vv_loudness.hip")).read()
    assert "#pragma clang fp contract(off)" in src
