"""N13, the look-ahead peak limiter: the host mirror (the specification), its consequences, the stream form, config and front-end
plumbing -- nothing here needs a GPU.

The mirror (core/audio_processor.py, limit_peaks) is checked against tests/limiter_util.py, the same seven steps from scipy's filters.
Bounds: gains within 1e-12 absolute (sums of at most 241 non-negative float64 terms below 1 and of 24 products: a few ulp, 4.5e-16 was
seen; a wrong index or window moves a gain by 1e-3 or more); PCM by output_util.lsb_condition (no difference above 1 LSB, at most 1
sample in 10^4: a gain that differs by 1e-16 can flip a tie).  Everything else is exact: equalities, or the ceiling as an integer."""
import ctypes
import math
import os
import re

import numpy as np
import pytest

from tests.limiter_util import H, SR, noisy, ref_ceiling, ref_gains, ref_limit, ref_taps, ref_window, sine, with_full_scale
from tests.output_util import lsb_condition

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
L0 = 120
W0 = 2 * L0 + H
PEAK = -1.0
MODES = ("sample", "true")


def _ap():
    from vietvoice_tts_amd.core import audio_processor
    return audio_processor


# ------------------------------------------------------------------ tables
def test_tables_and_constants():
    ap = _ap()
    assert ap.LIMIT_H == H == 12 and ap.LIMIT_MAX_L == 1024 and ap.LIMITER_LOOKAHEAD_S == 0.005 and ap.limiter_lookahead(SR) == L0
    h = ap.limiter_taps()
    assert h.dtype == np.float64 and h.size == 8 * H + 1 and h[4 * H] == 1.0 and np.abs(h - ref_taps()).max() < 1e-15
    assert np.abs(h[4 * H + 4:: 4]).max() < 1e-15 and np.array_equal(h, h[::-1])      # phase 0 is the sample itself
    for L in (1, 3, 120, 1024):
        w = ap.limiter_window(L)
        assert w.dtype == np.float64 and w.size == 2 * L + 1 and np.abs(w - ref_window(L)).max() < 1e-15 and abs(w.sum() - 1.0) < 1e-14
        assert w.min() > 0.0
    for bad in (0, 1025, -3, 2.0, True, None):
        with pytest.raises(ValueError):
            ap.limiter_window(bad)
    assert ap.check_limiter(None) is None and ap.check_limiter("sample") == "sample" and ap.check_limiter("true") == "true"
    for bad in ("peak", "TRUE", 1, True, 0.5):
        with pytest.raises(ValueError):
            ap.check_limiter(bad)
    with pytest.raises(ValueError):
        ap.limiter_lookahead(400000)                       # 2000 samples: over VV_LIMIT_MAX_L
    with pytest.raises(ValueError):
        ap.limit_peaks(np.zeros(8, np.float32), SR, PEAK, "true")
    for bad in (0.0, -1.0, float("nan"), float("inf"), "2", True):
        with pytest.raises(ValueError):
            ap.limit_peaks(np.zeros(8, np.int16), SR, PEAK, "true", gain=bad)


# ------------------------------------------------------------------ the mirror against the independent reference
@pytest.mark.parametrize("n", [1, 2, 120, 121, 241, 252, 253, 2047, 2049, 50003])
@pytest.mark.parametrize("mode", MODES)
def test_mirror_equals_the_scipy_reference(n, mode):
    ap = _ap()
    x = with_full_scale(noisy(n, n))
    g = 1.7
    v, e, s = ap.limiter_gains(x, ap.loudness_ceiling(PEAK), mode, g, L0)
    _v, e_ref, s_ref = ref_gains(x, ref_ceiling(PEAK), mode, g, L0)
    y, st = ap.limit_peaks(x, SR, PEAK, mode, gain=g)
    print(n, mode, "gain diff", np.abs(s - s_ref).max(), "e diff", np.abs(e - e_ref).max(), "limited", st["n_limited"])
    assert np.abs(s - s_ref).max() <= 1e-12
    assert np.abs(e - e_ref).max() <= 1e-12 * 65536
    lsb_condition(y, ref_limit(x, PEAK, mode, g, L0))
    assert st == {"g": g, "e_max": float(e.max()), "s_min": float(s.min()), "n_limited": int((s < 1).sum())} and st["n_limited"] > 0
    assert np.array_equal(y, np.clip(np.rint(v * s), -32768, 32767).astype(np.int16))


def test_empty_signal():
    y, st = _ap().limit_peaks(np.zeros(0, np.int16), SR, PEAK, "true", gain=2.0)
    assert y.size == 0 and y.dtype == np.int16 and st == {"g": 2.0, "e_max": 0.0, "s_min": 1.0, "n_limited": 0}


# ------------------------------------------------------------------ the true-peak estimate
@pytest.mark.parametrize("f", [997, 5000, 9000, 11000])
def test_true_peak_estimate_of_a_sine(f):
    ap = _ap()
    x = sine(4800, f, 30000.0, phase=0.3)
    _v, e, _s = ap.limiter_gains(x, 1e9, "true", 1.0, L0)
    db = 20 * math.log10(e[2 * H: -2 * H].max() / 30000.0)
    print(f, "Hz reads", db, "dB")
    assert abs(db) <= 0.05


def test_quarter_rate_sine_at_45_degrees():
    ap = _ap()
    x = sine(4800, SR / 4, 30000.0, phase=math.pi / 4)
    c = ap.loudness_ceiling(PEAK)
    assert int(np.abs(x.astype(np.int32)).max()) == 21213                              # the samples never see the peak of 30000
    _v, e, _s = ap.limiter_gains(x, 1e9, "true", 1.0, L0)
    print("fs/4 reads", e[2 * H: -2 * H].max())
    assert abs(20 * math.log10(e[2 * H: -2 * H].max() / 30000.0)) <= 0.05
    y, st = ap.limit_peaks(x, SR, PEAK, "sample")
    assert np.array_equal(y, x) and st["n_limited"] == 0 and st["s_min"] == 1.0       # 21213 < c: untouched
    y, st = ap.limit_peaks(x, SR, PEAK, "true")
    inner = np.abs(y[W0: -W0].astype(np.int32)).max()
    print("true mode: sample peak", inner, "c / sqrt 2", c / math.sqrt(2))
    assert abs(inner - c / math.sqrt(2)) <= 1.0 and st["n_limited"] == x.size


# ------------------------------------------------------------------ consequences of the specification
def _theorem_inputs():
    rng = np.random.default_rng(7)
    lone = np.zeros(700, np.int16)
    lone[333] = -32768
    alt = np.full(901, 32767, np.int16)
    alt[1::2] = -32767
    return {"random": rng.integers(-32768, 32768, 5003).astype(np.int16), "dc": np.full(600, -32768, np.int16), "lone": lone, "alternating": alt,
            "dc+": np.full(5, 32767, np.int16)}


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("name", ["random", "dc", "lone", "alternating", "dc+"])
def test_ceiling_is_a_theorem(name, mode):
    ap = _ap()
    x = _theorem_inputs()[name]
    for peak, g, L in ((PEAK, 1.0, L0), (PEAK, 1.7, L0), (0.0, 4.0, 3), (-20.0, 1.0, 1), (-6.0, 250.0, 1024)):
        y, st = ap.limit_peaks(x, SR, peak, mode, gain=g, L=L)
        c = ap.loudness_ceiling(peak)
        print(name, mode, peak, g, L, "max |y|", np.abs(y.astype(np.int32)).max(), "ceil c", math.ceil(c))
        assert np.abs(y.astype(np.int32)).max() <= math.ceil(c)
        assert st["e_max"] >= np.abs(x.astype(np.float64) * g).max() and 0.0 < st["s_min"] <= 1.0


@pytest.mark.parametrize("mode", MODES)
def test_untouched_region_and_reach_of_a_peak(mode):
    ap = _ap()
    g = 1.5
    x = noisy(6000, 3, scale=800.0)                         # far under the ceiling, also between the samples
    x[3000] = 32767                                         # one isolated peak
    c = ap.loudness_ceiling(PEAK)
    v, e, s = ap.limiter_gains(x, c, mode, g, L0)
    over = np.flatnonzero(e > c)
    assert over.size and over.min() >= 3000 - H and over.max() <= 3000 + H
    dist = np.abs(np.arange(x.size)[:, None] - over[None, :]).min(axis=1)
    far = dist > 2 * L0 + H
    assert far.sum() > 5000 and np.all(s[dist > 2 * L0] == 1.0)                      # exactly 1: the attenuation is a sum of zeros
    y, st = ap.limit_peaks(x, SR, PEAK, mode, gain=g)
    plain = np.clip(np.rint(x.astype(np.float64) * g), -32768, 32767).astype(np.int16)
    assert np.array_equal(y[far], plain[far])
    touched = np.flatnonzero(y != plain)
    print(mode, "samples over", over.size, "touched", touched.size, "s < 1", st["n_limited"])
    assert st["n_limited"] <= 4 * L0 + 1 + 2 * H and touched.size and touched.max() - touched.min() + 1 <= 4 * L0 + 1 + 2 * H
    assert abs(int(y[3000])) <= math.ceil(c)


@pytest.mark.parametrize("mode", MODES)
def test_a_quiet_signal_is_the_plain_product_bit_for_bit(mode):
    ap = _ap()
    x = noisy(30000, 5, scale=2500.0)
    for g in (1.0, 1.3):
        v, e, s = ap.limiter_gains(x, ap.loudness_ceiling(PEAK), mode, g, L0)
        assert e.max() < ap.loudness_ceiling(PEAK) and np.all(s == 1.0)
        y, st = ap.limit_peaks(x, SR, PEAK, mode, gain=g)
        assert np.array_equal(y, np.clip(np.rint(x.astype(np.float64) * g), -32768, 32767).astype(np.int16)) and st["n_limited"] == 0
    assert np.array_equal(ap.limit_peaks(x, SR, PEAK, mode)[0], x)


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("L", [3, 120])
def test_a_block_with_context_equals_the_whole(mode, L):
    ap = _ap()
    x = with_full_scale(noisy(9000, 11))
    W = 2 * L + H
    whole = ap.limit_peaks(x, SR, PEAK, mode, gain=1.7, L=L)[0]
    for a, b in ((W, 2 * W + 1), (1000, 1001), (2047, 4100), (x.size - W - 50, x.size - W)):
        part = ap.limit_peaks(x[a - W: b + W], SR, PEAK, mode, gain=1.7, L=L)[0]
        assert np.array_equal(part[W: W + b - a], whole[a: b]), (a, b)
    # one sample of context less and the seam shows: the window W is not generous
    part = ap.limit_peaks(x[0: 3000], SR, PEAK, mode, gain=1.7, L=L)[0]
    assert np.array_equal(part[: 3000 - W], whole[: 3000 - W])


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("block", [1, 7, W0 - 1, W0, W0 + 1, 5000])
def test_stream_equals_the_whole(block, mode):
    ap = _ap()
    n = 1500 if block == 1 else 12000
    x = np.clip(with_full_scale(noisy(n, 21)).astype(np.float64) * 1.7, -32768, 32767).astype(np.int16)
    want = ap.limit_peaks(x, SR, PEAK, mode)[0]
    ls = ap.LimiterStream(SR, PEAK, mode)
    out, most = [], 0
    for i in range(0, n, block):
        out.append(ls.push(x[i: i + block]))
        most = max(most, ls.hist.size)
        assert sum(o.size for o in out) == max(0, min(n, i + block) - W0)            # exactly W held back
    out.append(ls.flush())
    assert np.array_equal(np.concatenate(out), want) and ls.flush().size == 0
    assert most <= 2 * W0 + block                                                     # 2W of history once a push has been answered
    empty = ap.LimiterStream(SR, PEAK, mode)
    assert empty.push(np.zeros(0, np.int16)).size == 0 and empty.flush().size == 0


# ------------------------------------------------------------------ with the loudness stage
def _peaky(seed=2):
    """Three seconds of a speech-like signal and one lone plosive of 2.5 times its largest sample inside a loud stretch (40 samples
    after the largest sample, so that no gated block changes sides): it sets the sample peak and carries under 1 % of the energy.
    What the limiter takes away is at most the 4L + 1 + 2H = 505 samples around it, 0.7 % of the signal, if among its loudest.
    -> (signal, position of the plosive)."""
    from tests.loudness_util import speechlike
    x = speechlike(3 * SR, SR, seed)
    a = np.abs(x.astype(np.int32))
    at = [int(a.argmax()) + 40]
    x[at] = int(2.5 * a.max())
    return x, at


def test_normalize_loudness_with_a_limiter():
    ap = _ap()
    x, PLOSIVES = _peaky()
    L_in = ap.measure_loudness(x, SR)[0]
    quiet_target = L_in - 6.0                               # the gain is under 1: the ceiling is never reached
    for mode in MODES:
        assert np.array_equal(ap.normalize_loudness(x, SR, quiet_target, PEAK, limiter=mode), ap.normalize_loudness(x, SR, quiet_target, PEAK))
    assert np.array_equal(ap.normalize_loudness(x, SR, None, PEAK, limiter="true"), ap.limit_peaks(x, SR, PEAK, "true")[0])
    body = x.copy()
    body[list(PLOSIVES)] = 0
    g_body = 0.8 * ap.loudness_ceiling(PEAK) / np.abs(body.astype(np.int32)).max()     # the body stays under the ceiling, the plosives do not
    assert g_body > 2.0
    target = L_in + 20 * math.log10(g_body)
    capped = ap.normalize_loudness(x, SR, target, PEAK)
    L_capped = ap.measure_loudness(capped, SR)[0]
    for mode in MODES:
        got = ap.normalize_loudness(x, SR, target, PEAK, limiter=mode)
        L_got = ap.measure_loudness(got, SR)[0]
        print(mode, "input", L_in, "target", target, "capped gain reaches", L_capped, "limiter reaches", L_got)
        assert L_capped < target - 3.0                      # one plosive held the whole utterance down
        assert L_got > L_capped and abs(L_got - target) <= 0.1
        assert np.abs(got.astype(np.int32)).max() <= math.ceil(ap.loudness_ceiling(PEAK))
        _Lm, zbar, kept, peak = ap.measure_loudness(x, SR)
        g = ap.limiter_pregain(zbar, kept, peak, ap.loudness_target(target))
        assert g == float(np.sqrt(np.float64(ap.loudness_target(target)) / np.float64(zbar)))
        assert np.array_equal(got, ap.limit_peaks(x, SR, PEAK, mode, gain=g)[0])
    assert ap.limiter_pregain(0.5, 0, 9, 1.0) == 1.0 and ap.limiter_pregain(0.5, 3, 0, 1.0) == 1.0 and ap.limiter_pregain(0.5, 3, 9, 0.0) == 1.0
    assert ap.limiter_pregain(0.25, 3, 100, 1.0) == 2.0    # not capped by the peak


# ------------------------------------------------------------------ config, front end
def test_config_validation_and_round_trip(tmp_path):
    from vietvoice_tts_amd.core import ModelConfig
    base = dict(model_cache_dir=str(tmp_path), synthetic_model=True, model_spec="tiny")
    assert ModelConfig(**base).output_limiter is None
    for mode in MODES:
        c = ModelConfig(output_limiter=mode, output_peak_dbfs=-2, **base)
        d = c.to_dict()
        assert d["output_limiter"] == mode and ModelConfig.from_dict(d).to_dict() == d
    ModelConfig(output_limiter="true", output_loudness=-16, **base)
    for bad in ("on", "True", 1, True, 0.0, ["true"]):
        with pytest.raises(ValueError):
            ModelConfig(output_limiter=bad, **base)


def test_front_end_refuses_a_bad_limiter():
    from vietvoice_tts_amd.batching import BatchingFrontend
    fe = BatchingFrontend(engine=None, overlap=False)
    try:
        for bad in ("on", 1, True, 0.5):
            with pytest.raises(ValueError):
                fe.submit("x", limiter=bad).result(timeout=5)
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
    from vietvoice_tts_amd.core.audio_processor import limit_peaks, lin2ulaw, normalize_loudness, resample_output
    eng = cpu_engine
    _reseed(eng)
    base, _ = eng.synthesize(TEXT)
    assert len(eng._last_plan) > 1 and eng.config.output_limiter is None
    peak = float(np.clip(20 * math.log10(np.abs(base.astype(np.int32)).max() / 32767.0) - 6.0, -20.0, -1.0))   # 6 dB under the largest sample
    try:
        eng.config.output_peak_dbfs = peak
        _reseed(eng)
        assert np.array_equal(eng.synthesize(TEXT)[0], base)                          # the option unset: today's output
        for mode in MODES:
            eng.config.output_limiter = mode
            assert not eng._device_output()                  # injected sessions: the host mirror
            want, st = limit_peaks(base, SR, peak, mode)
            assert st["n_limited"] > 0 and not np.array_equal(want, base)
            _reseed(eng)
            assert np.array_equal(eng.synthesize(TEXT)[0], want)
            _reseed(eng)
            blocks = list(eng.synthesize_stream(TEXT))
            assert len(blocks) > 1 and np.array_equal(np.concatenate(blocks), want)   # stream == buffered
        eng.config.output_sample_rate, eng.config.output_encoding = 8000, "ulaw"      # after the join, before rate and encoding
        _reseed(eng)
        final = lin2ulaw(resample_output(want, SR, 8000))
        assert np.array_equal(eng.synthesize(TEXT)[0], final)
        _reseed(eng)
        assert np.array_equal(np.concatenate(list(eng.synthesize_stream(TEXT))), final)
        eng.config.output_sample_rate, eng.config.output_encoding = None, "pcm16"
        eng.config.output_loudness = -23.0                                            # join -> loudness gain, uncapped -> limiter
        _reseed(eng)
        assert np.array_equal(eng.synthesize(TEXT)[0], normalize_loudness(base, SR, -23.0, peak, limiter="true"))
        with pytest.raises(ValueError, match="output_loudness"):                      # still refused, limiter or not
            eng.synthesize_stream(TEXT)
        eng.config.output_loudness, eng.config.output_limiter = None, None
        fe = BatchingFrontend(eng, overlap=False)
        try:
            _reseed(eng)
            own = fe.submit(TEXT, limiter="sample").result(timeout=300)[0]
            _reseed(eng)
            both = fe.submit(TEXT, limiter="true", loudness=-30.0).result(timeout=300)[0]
            _reseed(eng)
            plain = fe.submit(TEXT).result(timeout=300)[0]
        finally:
            fe.close()
        assert np.array_equal(plain, base) and np.array_equal(own, limit_peaks(base, SR, peak, "sample")[0])
        assert np.array_equal(both, normalize_loudness(base, SR, -30.0, peak, limiter="true"))
    finally:
        eng.config.output_loudness, eng.config.output_peak_dbfs, eng.config.output_limiter = None, -1.0, None
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
    for name, n_args in (("vv_pcm_limit", 18), ("vv_pcm_limit_ws_bytes", 3), ("vv_pcm_limit_tile", 1)):
        assert name in declared and len(runtime.EXPORTS[name][1]) == n_args
        assert any(re.fullmatch(g.replace("*", ".*"), name) for g in globs) and hasattr(lib, name)
    args = [None if t is ctypes.c_void_p else 0 for t in runtime.EXPORTS["vv_pcm_limit"][1]]
    assert lib.vv_pcm_limit(*args) == -22                                             # no context: refused before anything else
    assert lib.vv_pcm_limit_ws_bytes(1000, 3, 2) >= 1000 * 8 + 3 * 24 and lib.vv_pcm_limit_ws_bytes(0, 0, 1) > 0
    assert "vv_limiter" in build_ext.SOURCES
    assert int(re.search(r"#define VV_LIMIT_H (\d+)", hdr).group(1)) == _ap().LIMIT_H == 12
    assert int(re.search(r"#define VV_LIMIT_MAX_L (\d+)", hdr).group(1)) == _ap().LIMIT_MAX_L == 1024
    assert re.search(r"#define\s+VV_PROF_NCLASS\s+18\b", hdr)
    src = open(os.path.join(ROOT, "vietvoice-tts_amd", "csrc", "vv_limiter.hip")).read()
    assert "#pragma clang fp contract(off)" in src and not re.search(r"atomic\w*\s*\(", src)
    # the tile of the gain pass: r over tile + 4L and d over tile + 2L float64 share 7424 slots of LDS
    for L, tile in ((1, 2048), (3, 2048), (120, 2048), (554, 2048), (555, 1024), (896, 1024), (897, 512), (1024, 512)):
        assert lib.vv_pcm_limit_tile(L) == tile and 2 * tile + 6 * L <= 7424
    assert lib.vv_pcm_limit_tile(0) == -22 and lib.vv_pcm_limit_tile(1025) == -22
