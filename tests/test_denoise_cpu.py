"""N19 on the host (no GPU): the mirror of the vocoder-bias denoiser (core/audio_processor.py: denoise_fft, denoise_bias, denoise_pcm) and
its plumbing.  What the subtraction means is measured on a synthetic hum under a tone with numpy's own transform (tests/denoise_util.py);
the device is held to this mirror bit for bit in tests/test_denoise_gpu.py."""
import ctypes
import os
import re

import numpy as np
import pytest

from tests import denoise_util as du

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _ap():
    from vietvoice_tts_amd.core import audio_processor
    return audio_processor


# ------------------------------------------------------------------ the transform and the identity
def test_the_mirrors_transform_equals_numpys_fft():
    ap = _ap()
    rng = np.random.default_rng(11)
    re_, im_ = rng.standard_normal((7, du.N)) * 1e4, rng.standard_normal((7, du.N)) * 1e4
    z = re_ + 1j * im_
    for inverse, want in ((False, np.fft.fft(z, axis=1)), (True, np.fft.ifft(z, axis=1) * du.N)):
        r, i = ap.denoise_fft(re_, im_, inverse=inverse)
        err = np.abs((r + 1j * i) - want).max() / np.abs(want).max()
        print("relative error of the transform, inverse =", inverse, ":", err)
        assert err <= 1e-12
    w, tw = ap.denoise_tables()
    k = np.arange(du.N)
    assert np.array_equal(w, 0.5 - 0.5 * np.cos(2.0 * np.pi * k / du.N)) and tw.shape == (2, du.N // 2) and tw.dtype == np.float64
    assert np.array_equal(tw[0], np.cos(2.0 * np.pi * k[:512] / du.N)) and np.array_equal(tw[1], -np.sin(2.0 * np.pi * k[:512] / du.N))
    w4 = (w * w).reshape(4, du.H).sum(axis=0)                                         # every sample lies under four frames: sum of w^2 = 1.5
    assert np.abs(w4 - 1.5).max() < 1e-12


@pytest.mark.parametrize("n", (1, 255, 256, 257, 1023, 1024, 1025, 5000))
def test_strength_zero_gives_the_input_back(n):
    ap = _ap()
    x = du.noise(n, 100 + n)
    z, mag = ap.denoise_pcm(x, du.random_bias(3), 0.0, mags=True)
    assert z.dtype == np.int16 and np.array_equal(z, x)                               # computed through both transforms, not short-circuited
    assert mag.shape == (du.frames_of(n), du.N) and mag.any()
    assert np.array_equal(ap.denoise_pcm(x, np.zeros(du.BINS), 16.0), x)              # an all-zero bias at any strength


def test_strength_zero_on_the_full_scale_alternation():
    ap = _ap()
    x = du.alternation(5000)
    assert np.array_equal(ap.denoise_pcm(x, du.random_bias(4), 0.0), x)
    assert ap.denoise_pcm(np.zeros(0, np.int16), du.random_bias(4), 1.0).size == 0


# ------------------------------------------------------------------ the feature means something
def test_hum_under_a_tone_is_removed_and_the_tone_stays():
    ap = _ap()
    sig, hum = du.hum_and_tone()
    bias = ap.denoise_bias(hum)                                                       # 20 full frames of the rounded hum alone
    assert bias.shape == (du.BINS,) and bias.dtype == np.float64 and int(np.argmax(bias)) == 40
    a0 = du.segment_amplitudes(sig)
    for s in (0.5, 1.0, 1.5):
        a = du.segment_amplitudes(ap.denoise_pcm(sig, bias, s))
        print(f"strength {s}: hum bin {a[40]:.1f} of {a0[40]:.1f} ({a[40] / a0[40]:.3e}), tone bin changed by {abs(a[150] - a0[150]) / a0[150]:.2e}")
        if s == 0.5:
            assert abs(a[40] - 0.5 * a0[40]) <= 0.01 * 0.5 * a0[40]                   # within 1 % of half its input
        else:
            assert a[40] < 1e-3 * a0[40]
        assert abs(a[150] - a0[150]) <= 1e-4 * a0[150]


def test_a_bias_above_every_magnitude_gives_zeros():
    ap = _ap()
    x = du.speechlike(3000, 5)
    z, mag = ap.denoise_pcm(x, np.full(du.BINS, 1e12), 1.0, mags=True)
    assert mag.max() < 1e12 and not z.any() and z.size == x.size


def test_denoise_bias_wants_a_full_frame_and_is_the_mean_magnitude():
    ap = _ap()
    for n in (0, 1, 1023):
        with pytest.raises(ValueError, match="denoise_bias"):
            ap.denoise_bias(np.zeros(n, np.int16))
    x = du.speechlike(1024 + 3 * 256 + 100, 6)                                        # four full frames; the ragged tail is not measured
    w = ap.denoise_tables()[0]
    want = np.mean([np.abs(np.fft.rfft(w * x[f * 256: f * 256 + 1024].astype(np.float64))) for f in range(4)], axis=0)
    got = ap.denoise_bias(x)
    assert np.abs(got - want).max() <= 1e-12 * want.max()
    assert np.array_equal(ap.denoise_bias(x[: 1024 + 3 * 256]), got)
    for bad in (np.zeros(512), np.full(du.BINS, -1.0), np.full(du.BINS, np.nan), None):
        with pytest.raises(ValueError):
            ap.denoise_pcm(x, bad, 1.0)
    for bad in (-0.5, 16.5, float("nan")):
        with pytest.raises(ValueError):
            ap.denoise_pcm(x, np.zeros(du.BINS), bad)


# ------------------------------------------------------------------ plans and options
def test_plan_denoise_on_hand_worked_rows_and_every_refusal():
    from vietvoice_tts_amd import pcm_stage as P
    rows = [[3, 1000, 64, 0], [1010, 257, 1070, 1], [1300, 0, 1400, 0]]
    full, s, frame_offs, n_y = P.plan_denoise(rows, [0.25, 1, 0.0], 2000, 2)
    assert full == rows and s == [0.25, 1.0, 0.0] and all(isinstance(v, float) for v in s)
    assert frame_offs == [0, 4 + 3, 7 + 2 + 3, 12 + 3] and n_y == 1327                # M = 4, 2, 0
    assert P.plan_denoise(rows, 0.5, 2000, 2)[1] == [0.5] * 3 and P.plan_denoise(rows, 0.5, 2000, 2, out_n=1327)[3] == 1327
    bad_rows = ([], [[0, 10, 0]], [[0, 10, 0, 0, 0]], [[-1, 10, 0, 0]], [[0, -1, 0, 0]], [[0, 10, -1, 0]], [[0, 10, 0, -1]], [[0, 10, 0, 2]],
                [[1995, 10, 0, 0]], [[0, (1 << 30) + 1, 0, 0]], [[0, 300, 0, 0], [300, 300, 299, 0]], [[0, 1, 0, 0]] * 65536)
    for r in bad_rows:
        with pytest.raises(ValueError, match="pcm_denoise"):
            P.plan_denoise(r, 1.0, 1 << 31 if r and r[0][1] > 1 << 30 else 2000, 2)
    for bad in (-0.1, 16.1, float("nan"), float("inf"), None, "1", True, [1.0], [1.0, 1.0, 1.0, 1.0]):
        with pytest.raises(ValueError, match="pcm_denoise"):
            P.plan_denoise(rows, bad, 2000, 2)
    with pytest.raises(ValueError, match="pcm_denoise"):
        P.plan_denoise(rows, 1.0, 2000, 2, out_n=1326)
    with pytest.raises(ValueError, match="pcm_denoise"):
        P.plan_denoise(rows, 1.0, 2000, 2, overlaps=True)
    assert P.plan_denoise_bias([[5, 1024], [0, 1280, 0, 0], [0, 1279]], 2000) == ([[5, 1024, 0, 0], [0, 1280, 0, 0], [0, 1279, 0, 0]], 1 + 2 + 1)
    for r in ([[0, 1023]], [[0, (1 << 20) + 1]], [[1000, 1024]], [[-1, 1024]], [], [[0, 1024, 0]]):
        with pytest.raises(ValueError, match="pcm_denoise_bias"):
            P.plan_denoise_bias(r, 1 << 21 if r and r[0][1] > 1 << 20 else 2000)


def test_finish_outputs_option_plans_nothing_when_no_request_has_a_strength():
    from vietvoice_tts_amd import pcm_stage as P
    assert P.plan_finish_denoise(3, None) is None and P.plan_finish_denoise(3, [None, None, None]) is None
    assert P.plan_finish_denoise(3, 1.5) == [1.5] * 3 and P.plan_finish_denoise(3, [None, 2, None]) == [None, 2.0, None]
    for bad in (0, 0.0, -1.0, 16.5, "1", True, [1.0, 1.0], float("nan")):
        with pytest.raises(ValueError):
            P.plan_finish_denoise(3, bad)
    assert P.plan_finish(3) == (None, None, [])                                      # the pinned plans are as before


def test_check_denoise_model_config_and_submit(tmp_path):
    from vietvoice_tts_amd.batching import BatchingFrontend
    from vietvoice_tts_amd.core import ModelConfig
    ap = _ap()
    make = lambda **kw: ModelConfig(model_cache_dir=str(tmp_path), synthetic_model=True, model_spec="tiny", **kw)      # noqa: E731
    assert ap.check_denoise(None) is None and ap.check_denoise(1) == 1.0 and ap.check_denoise(16) == 16.0
    for bad in (0, -1, 16.01, "1", True, float("nan"), float("inf")):
        with pytest.raises(ValueError, match="output_denoise"):
            ap.check_denoise(bad)
        with pytest.raises(ValueError, match="output_denoise"):
            make(output_denoise=bad)
    cfg = make()
    assert cfg.output_denoise is None and cfg.output_denoise_bias is None
    bias = du.random_bias(1)
    cfg = make(output_denoise=1.5, output_denoise_bias=bias)
    assert cfg.output_denoise == 1.5 and cfg.output_denoise_bias == [float(v) for v in bias]
    assert ModelConfig.from_dict(cfg.to_dict()).output_denoise_bias == cfg.output_denoise_bias
    for bad in ([1.0] * 512, [1.0] * 514, [-1.0] + [1.0] * 512, [float("nan")] * 513, "bias", [[1.0] * 513]):
        with pytest.raises(ValueError, match="output_denoise_bias"):
            make(output_denoise_bias=bad)

    class _Eng:
        config = cfg
    fe = BatchingFrontend.__new__(BatchingFrontend)
    fe.engine = _Eng()
    for bad in (0, -1.0, 17, "2"):
        with pytest.raises(ValueError, match="output_denoise"):
            BatchingFrontend.submit(fe, "x", denoise=bad).result(timeout=5)


def test_header_version_script_and_exports_agree_for_the_new_entries():
    from vietvoice_tts_amd import build_ext, runtime
    hdr = open(os.path.join(ROOT, "include", "vvtts.h")).read()
    declared = set(re.findall(r"VV_API\s+[\w\s\*]+?\b(vv_\w+)\s*\(", hdr))
    assert declared == set(runtime.EXPORTS), declared ^ set(runtime.EXPORTS)
    ver = open(os.path.join(ROOT, "vietvoice-tts_amd", "csrc", "vvtts.map")).read()
    globs = [g.strip() for g in re.findall(r"global:\s*([^;]+);", ver)]
    lib = runtime.load_library()
    for name, n_args in (("vv_pcm_denoise", 19), ("vv_pcm_denoise_ws_bytes", 1), ("vv_pcm_denoise_bias", 13), ("vv_pcm_denoise_bias_ws_bytes", 2)):
        assert name in declared and len(runtime.EXPORTS[name][1]) == n_args
        assert any(re.fullmatch(g.replace("*", ".*"), name) for g in globs) and hasattr(lib, name)
    assert "vv_denoise" in build_ext.SOURCES
    for name in ("vv_pcm_denoise", "vv_pcm_denoise_bias"):
        args = [None if t is ctypes.c_void_p else 0 for t in runtime.EXPORTS[name][1]]
        assert getattr(lib, name)(*args) == -22                                       # no context: refused before anything else
    assert len(runtime.EXPORTS["vv_pcm_formant"][1]) == 18                            # the old entry keeps its arguments
    assert lib.vv_pcm_denoise_ws_bytes(4) >= 4 * 16
    assert lib.vv_pcm_denoise_bias_ws_bytes(50, 4) >= 50 * du.BINS * 8 + 4 * 16 > lib.vv_pcm_denoise_bias_ws_bytes(5, 1) >= 5 * du.BINS * 8
    m = re.match(rb"vvtts-hip (\d+)\.(\d+) ", lib.vv_version())
    assert m and (int(m.group(1)), int(m.group(2))) >= (0, 12)                        # bumped with the additive entries
    ap = _ap()
    for macro, value in (("VV_DENOISE_N", ap.DENOISE_N), ("VV_DENOISE_H", ap.DENOISE_H), ("VV_DENOISE_BIAS_MAX_N", ap.DENOISE_BIAS_MAX_N)):
        assert re.search(rf"#define {macro} {value}\b", hdr)


# ------------------------------------------------------------------ engine and front end on injected sessions: the host mirror
def test_engine_and_front_end_apply_the_mirror_on_oracle_sessions(tmp_path):
    import torch
    from oracle.vv_oracle import Oracle, OracleSession
    from vietvoice_tts_amd.batching import BatchingFrontend
    from vietvoice_tts_amd.core import ModelConfig, TTSEngine
    ap = _ap()
    text = "Hôm nay trời đẹp quá, chúng ta cùng nhau đi dạo quanh hồ nhé."
    cfg = ModelConfig(model_cache_dir=str(tmp_path), synthetic_model=True, model_spec="tiny", nfe_step=3, max_chunk_duration=8.0)

    def factory(spec, weights, config):
        orc = Oracle(spec, weights, nfe_step=config.nfe_step)
        return {k: OracleSession(orc, k, seed=config.random_seed) for k in ("preprocess", "transformer", "decode")}

    eng = TTSEngine(cfg, session_factory=factory)

    def reseed():
        for sess in eng.model_session_manager.sessions.values():
            sess.gen = torch.Generator().manual_seed(123)

    try:
        reseed()
        base, _ = eng.synthesize(text)
        bias = ap.denoise_bias(base) * 0.5                                            # the caller's own profile
        cfg.output_denoise = 1.0
        with pytest.raises(RuntimeError, match="output_denoise_bias"):                # the model's bias needs the HIP engine
            eng.synthesize(text)
        with pytest.raises(ValueError, match="output_denoise"):
            eng.synthesize_stream(text)
        cfg.output_denoise_bias = [float(v) for v in bias]
        reseed()
        got, _ = eng.synthesize(text)
        want = ap.denoise_pcm(base, bias, 1.0)
        assert np.array_equal(got, want) and not np.array_equal(want, base)
        cfg.output_loudness = -20.0                                                   # the later links see the cleaned signal
        reseed()
        assert np.array_equal(eng.synthesize(text)[0], ap.normalize_loudness(want, cfg.sample_rate, -20.0, cfg.output_peak_dbfs))
        cfg.output_loudness, cfg.output_denoise = None, None
        fe = BatchingFrontend(eng, overlap=False)
        try:
            reseed()
            own = fe.submit(text, denoise=1.0).result(timeout=300)[0]
            reseed()
            plain = fe.submit(text).result(timeout=300)[0]
        finally:
            fe.close()
        assert np.array_equal(own, want) and np.array_equal(plain, base)
    finally:
        eng.cleanup()
