"""N22 on the host (no GPU): the mirror of the keyed audio watermark (core/audio_processor.py: watermark_chips, watermark_embed,
watermark_cells, watermark_stats, watermark_decide) and its plumbing.  The detection figures are those of the stand-in signals of
tests/watermark_util.py; the device is held to this mirror bit for bit in tests/test_watermark_gpu.py."""
import ctypes
import functools
import os
import re

import numpy as np
import pytest

from tests import watermark_util as wu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _ap():
    from vietvoice_tts_amd.core import audio_processor
    return audio_processor


@functools.lru_cache(maxsize=None)
def _marked(secs, seed, payload):
    x = wu.speechlike(secs * wu.SR, seed)
    y = _ap().watermark_embed(x, wu.KEY, payload, 0.2)
    y.setflags(write=False)
    return x, y


CASES = [(secs, seed, payload) for secs in (4, 11) for seed in wu.SEEDS for payload in wu.PAYLOADS]


def _expect(r, payload, offsets=(0,)):
    print(f"score {r.score:.3f} offset {r.offset} payload {r.payload} crc_ok {r.crc_ok}")
    assert r.present and r.crc_ok and r.payload == payload and r.offset in offsets
    assert r.score >= 2.0 * wu.NULL_MAX and len(r.z) == wu.NB


# ------------------------------------------------------------------ the known answers and the table
def test_known_answers_of_the_generator_and_the_crc():
    ap = _ap()
    assert ap.watermark_words(0, 1) == [0xE220A8397B1DCDAF]
    assert ap.watermark_words(0, 3)[:1] == ap.watermark_words(0, 1) and len(set(ap.watermark_words(7, 100))) == 100
    assert ap.watermark_message(0x1234) == 0x1234F1 and ap.flac_crc8(bytes([0x12, 0x34])) == 0xF1
    assert ap.watermark_message(0) == 0 and ap.watermark_message(0xFFFF) >> 8 == 0xFFFF
    assert (ap.WATERMARK_LO, ap.WATERMARK_K, ap.WATERMARK_G, ap.WATERMARK_P, ap.WATERMARK_NB, ap.WATERMARK_Q) == (wu.LO, wu.K, wu.G, wu.P, wu.NB, wu.Q)
    assert ap.WATERMARK_THRESHOLD == pytest.approx(1.3 * wu.NULL_MAX, abs=1e-3)         # the constant is the measured pool maximum times 1.3
    notes = open(os.path.join(ROOT, "profiles", "watermark", "notes.md")).read()
    assert f"{wu.NULL_MAX}" in notes and f"{ap.WATERMARK_THRESHOLD}" in notes


def test_the_chip_table_is_plus_minus_one_and_differs_between_keys():
    ap = _ap()
    a, b = ap.watermark_chips(wu.KEY), ap.watermark_chips(wu.WRONG_KEY)
    assert a.shape == (wu.P, wu.K) and a.dtype == np.int8 and set(np.unique(a)) == {-1, 1}
    assert 0.45 < (a != b).mean() < 0.55 and abs(int(a.sum())) < 4 * np.sqrt(a.size)
    word0 = ap.watermark_words(wu.KEY, 1)[0]
    assert [int(v) for v in a.reshape(-1)[:64]] == [1 if word0 >> i & 1 else -1 for i in range(64)]      # LSB first
    e = 37 * wu.K + 111                                                                # cell e takes bit e % 64 of word e // 64
    assert a[37, 111] == (1 if ap.watermark_words(wu.KEY, e // 64 + 1)[e // 64] >> (e % 64) & 1 else -1)
    assert ap.watermark_chips(wu.KEY) is a and not a.flags.writeable
    for bad in (-1, 1 << 64, 1.0, "1", True, None):
        with pytest.raises(ValueError):
            ap.watermark_chips(bad)


@pytest.mark.parametrize("n", wu.LENGTHS)
def test_strength_zero_gives_the_input_back(n):
    ap = _ap()
    x = wu.noise(n, 200 + n)
    z = ap.watermark_embed(x, wu.KEY, 0xBEEF, 0.0)
    assert z.dtype == np.int16 and np.array_equal(z, x)                               # computed through both transforms, not short-circuited
    assert ap.watermark_embed(np.zeros(0, np.int16), wu.KEY, 1, 0.2).size == 0
    if n >= 1023:
        assert not np.array_equal(ap.watermark_embed(x, wu.KEY, 0xBEEF, 0.2), x)


def test_the_statistic_equals_its_definition_cell_by_cell():
    ap = _ap()
    y = ap.watermark_embed(wu.speechlike(1500, 4), wu.KEY, 0x1234, 0.5)
    cells = ap.watermark_cells(y)
    assert cells.shape == (wu.frames_of(1500), wu.K) and cells.dtype == np.int32 and np.abs(cells).max() <= 32768
    assert np.array_equal(ap.watermark_stats(y, wu.KEY), wu.naive_stats(cells, ap.watermark_chips(wu.KEY)))
    w = ap.denoise_tables()[0]                                                        # the cell value against numpy's own transform
    F = cells.shape[0]
    xp = np.concatenate([np.zeros(3 * wu.H), y.astype(np.float64), np.zeros(wu.N + wu.H)])
    m = np.stack([np.abs(np.fft.rfft(w * xp[f * wu.H: f * wu.H + wu.N]))[wu.LO: wu.LO + wu.K] for f in range(F)])
    f = np.arange(F)
    r = 0.5 * (m[np.maximum(f - wu.G, 0)] + m[np.minimum(f + wu.G, F - 1)])
    assert np.abs(np.rint(32768.0 * (m - r) / (m + r + 1.0)) - cells).max() <= 1


# ------------------------------------------------------------------ detection on the stand-in signals
@pytest.mark.parametrize("secs,seed,payload", CASES)
def test_a_marked_signal_is_found_with_its_payload(secs, seed, payload):
    ap = _ap()
    x, y = _marked(secs, seed, payload)
    d = y.astype(np.float64) - x
    print("marked versus original:", 10 * np.log10((x.astype(np.float64) ** 2).sum() / (d * d).sum()), "dB")
    _expect(ap.watermark_detect(y, wu.KEY), payload)


@pytest.mark.parametrize("secs,seed,payload", CASES)
def test_it_survives_a_mu_law_round_trip(secs, seed, payload):
    _x, y = _marked(secs, seed, payload)
    _expect(_ap().watermark_detect(wu.ulaw_round_trip(y), wu.KEY), payload)


@pytest.mark.parametrize("secs,seed,payload", CASES)
def test_it_survives_a_gain_of_one_half(secs, seed, payload):
    _x, y = _marked(secs, seed, payload)
    half = np.rint(0.5 * y.astype(np.float64)).astype(np.int16)
    _expect(_ap().watermark_detect(half, wu.KEY), payload)


@pytest.mark.parametrize("secs,seed,payload", CASES)
def test_it_is_found_again_after_a_cut_at_the_front(secs, seed, payload):
    _x, y = _marked(secs, seed, payload)
    _expect(_ap().watermark_detect(np.ascontiguousarray(y[wu.CUT:]), wu.KEY), payload, offsets=(20, 21))


def test_unmarked_wrong_key_silence_and_a_tone_are_not_present():
    ap = _ap()
    x, y = _marked(4, 1, wu.PAYLOADS[0])
    tone = np.rint(12000.0 * np.sin(2 * np.pi * 1000.0 * np.arange(2 * wu.SR) / wu.SR)).astype(np.int16)
    for name, sig, key in (("unmarked", x, wu.KEY), ("wrong key", y, wu.WRONG_KEY), ("noise", wu.noise(wu.SR, 9), wu.KEY),
                           ("zeros", np.zeros(5000, np.int16), wu.KEY), ("empty", np.zeros(0, np.int16), wu.KEY), ("one sample", x[:1], wu.KEY),
                           ("tone", tone, wu.KEY)):
        stats = ap.watermark_stats(sig, key)
        r = ap.watermark_decide(stats)
        print(f"{name}: score {r.score:.3f}")
        assert stats.shape == (wu.Q, wu.NB, 2) and stats.dtype == np.int64 and (stats[..., 1] >= 0).all()
        assert not r.present and np.isfinite(r.score) and np.all(np.isfinite(r.z)) and r.score < ap.WATERMARK_THRESHOLD
    zeros = ap.watermark_stats(np.zeros(5000, np.int16), wu.KEY)
    assert not zeros.any() and ap.watermark_decide(zeros).score == 0.0                # den = 0 everywhere: z = 0, no division
    r = ap.watermark_decide(ap.watermark_stats(y, wu.KEY))
    flipped = ap.watermark_stats(y, wu.KEY).copy()
    flipped[r.offset, 5, 0] *= -1                                                     # one wrong bit: the CRC says so and no payload is given
    bad = ap.watermark_decide(flipped)
    assert bad.present and not bad.crc_ok and bad.payload is None


# ------------------------------------------------------------------ plans and options
def test_the_plans_on_hand_worked_rows_and_every_refusal():
    from vietvoice_tts_amd import pcm_stage as P
    ap = _ap()
    rows = [[3, 1000, 64], [1010, 257, 1070], [1300, 0, 1400]]
    full, gp, gm, n_y = P.plan_watermark(rows, [0x1234, 0, 65535], 0.2, 2000)
    assert full == [[3, 1000, 64, 0x1234F1], [1010, 257, 1070, 0], [1300, 0, 1400, ap.watermark_message(65535)]]
    assert (gp, gm, n_y) == (1.0 + 0.2, 1.0 - 0.2, 1327)
    assert P.plan_watermark(rows, 7, 0, 2000)[1:3] == (1.0, 1.0) and P.plan_watermark(rows, 7, 0.5, 2000, out_n=1327)[1:] == (1.5, 0.5, 1327)
    bad_rows = ([], [[0, 10]], [[0, 10, 0, 0]], [[-1, 10, 0]], [[0, -1, 0]], [[0, 10, -1]], [[1995, 10, 0]], [[0, (1 << 30) + 1, 0]],
                [[0, 300, 0], [300, 300, 299]], [[0, 1, 0]] * 65536)
    for r in bad_rows:
        with pytest.raises(ValueError, match="pcm_watermark"):
            P.plan_watermark(r, 1, 0.2, 1 << 31 if r and r[0][1] > 1 << 30 else 2000)
    for bad in (-1, 65536, 1.0, "1", True, None, [1], [1, 2, 3, 4]):
        with pytest.raises(ValueError, match="watermark"):
            P.plan_watermark(rows, bad, 0.2, 2000)
    for bad in (-0.1, 0.51, float("nan"), float("inf"), None, "0.2", True):
        with pytest.raises(ValueError, match="output_watermark_strength"):
            P.plan_watermark(rows, 1, bad, 2000)
    with pytest.raises(ValueError, match="pcm_watermark"):
        P.plan_watermark(rows, 1, 0.2, 2000, out_n=1326)
    with pytest.raises(ValueError, match="pcm_watermark"):
        P.plan_watermark(rows, 1, 0.2, 2000, overlaps=True)
    assert P.plan_watermark_detect([[5, 1024], [0, 1, 0, 0], [0, 0]], 2000) == ([[5, 1024, 0, 0], [0, 1, 0, 0], [0, 0, 0, 0]], [0, 7, 11, 14])
    for r in ([[0, (1 << 24) + 1]], [[1000, 1024]], [[-1, 1024]], [[0, -1]], [], [[0, 1024, 0]], [[0, 1]] * 65536):
        with pytest.raises(ValueError, match="pcm_watermark_detect"):
            P.plan_watermark_detect(r, 1 << 25 if r and r[0][1] > 1 << 24 else 2000)
    assert P.plan_finish_watermark(3, None, 5) is None and P.plan_finish_watermark(3, [None] * 3, None) is None
    assert P.plan_finish_watermark(3, 9, 5) == (5, [9, 9, 9], 0.2) and P.plan_finish_watermark(3, [None, 2, None], 5, 0.5) == (5, [None, 2, None], 0.5)
    for args in ((3, 9, None), (3, [1, 2], 5), (3, 65536, 5), (3, 1.5, 5), (3, 9, -1), (3, 9, 1 << 64), (3, 9, 5, 0.0), (3, 9, 5, 0.6)):
        with pytest.raises(ValueError):
            P.plan_finish_watermark(*args)
    assert P.plan_finish(3) == (None, None, [])                                      # the pinned plans are as before


def test_checks_model_config_request_options_and_submit(tmp_path):
    from vietvoice_tts_amd.batching import BatchingFrontend
    from vietvoice_tts_amd.core import ModelConfig
    from vietvoice_tts_amd.request_options import RequestOptions, column
    ap = _ap()
    make = lambda **kw: ModelConfig(model_cache_dir=str(tmp_path), synthetic_model=True, model_spec="tiny", **kw)      # noqa: E731
    assert ap.check_watermark_key(None) is None and ap.check_watermark_key(0) == 0 and ap.check_watermark_key((1 << 64) - 1) == (1 << 64) - 1
    assert ap.check_watermark_payload(None) is None and ap.check_watermark_payload(65535) == 65535
    assert ap.check_watermark_strength(0.5) == 0.5 and ap.check_watermark_strength(0, zero=True) == 0.0
    for bad in (-1, 1 << 64, 0.5, "1", True):
        with pytest.raises(ValueError, match="output_watermark_key"):
            ap.check_watermark_key(bad)
        with pytest.raises(ValueError, match="output_watermark_key"):
            make(output_watermark_key=bad)
    for bad in (-1, 65536, 0.5, "1", True):
        with pytest.raises(ValueError, match="watermark payload"):
            ap.check_watermark_payload(bad)
        with pytest.raises(ValueError, match="watermark payload"):
            make(output_watermark_payload=bad)
        with pytest.raises(ValueError, match="watermark payload"):
            RequestOptions.checked(watermark_payload=bad)
    with pytest.raises(ValueError, match="watermark payload"):
        make(output_watermark_payload=None)
    for bad in (0, 0.0, -0.1, 0.51, "0.2", True, None, float("nan")):
        with pytest.raises(ValueError, match="output_watermark_strength"):
            ap.check_watermark_strength(bad)
        with pytest.raises(ValueError, match="output_watermark_strength"):
            make(output_watermark_strength=bad)
    plain, keyed = make(), make(output_watermark_key=wu.KEY, output_watermark_payload=77, output_watermark_strength=0.3)
    assert (plain.output_watermark_key, plain.output_watermark_payload, plain.output_watermark_strength) == (None, 0, 0.2)
    assert ModelConfig.from_dict(keyed.to_dict()).output_watermark_key == wu.KEY
    # the record: None = the engine's payload, which exists only with a key
    assert RequestOptions().resolved(plain).watermark_payload is None and not RequestOptions().resolved(plain).wants_output_stage()
    assert RequestOptions().resolved(keyed).watermark_payload == 77 and RequestOptions().resolved(keyed).wants_output_stage()
    own = RequestOptions.checked(watermark_payload=5)
    assert own.watermark_payload == 5 and own.resolved(keyed).watermark_payload == 5 and own.wants_output_stage()
    assert RequestOptions.checked(watermark_payload=0).resolved(keyed).watermark_payload == 0       # 0 is a payload, not "unset"
    with pytest.raises(ValueError, match="output_watermark_key"):
        own.resolved(plain)
    assert column([RequestOptions().resolved(keyed), own.resolved(keyed)], "watermark_payload") == [77, 5]

    class _Eng:
        config = plain
    fe = BatchingFrontend.__new__(BatchingFrontend)
    fe.engine = _Eng()
    with pytest.raises(ValueError, match="output_watermark_key"):                     # a payload on an engine without a key
        BatchingFrontend.submit(fe, "x", watermark_payload=5).result(timeout=5)
    _Eng.config = keyed
    for bad in (-1, 65536, "2", 1.5):
        with pytest.raises(ValueError, match="watermark payload"):
            BatchingFrontend.submit(fe, "x", watermark_payload=bad).result(timeout=5)


def test_finish_output_receives_the_column_only_with_a_key_and_the_stream_refuses(tmp_path):
    from vietvoice_tts_amd.core import ModelConfig, TTSEngine
    from vietvoice_tts_amd.request_options import RequestOptions
    seen = {}

    class _Hip:
        def finish_output(self, *args, **kw):
            seen.clear()
            seen.update(kw)
            return ["done"]

    class _Manager:
        engine = _Hip()

    def run(options=None, **kw):
        eng = TTSEngine.__new__(TTSEngine)
        eng.config = ModelConfig(model_cache_dir=str(tmp_path), synthetic_model=True, model_spec="tiny", **kw)
        eng.model_session_manager = _Manager()
        assert eng._finish_device((None, [(0, 10), (10, 10)]), [1, 1], options) == ["done"]
        return eng

    run()
    assert not any(k.startswith("watermark") for k in seen)                           # without a key the call is the one of ever
    eng = run(output_watermark_key=wu.KEY, output_watermark_payload=3, output_watermark_strength=0.25)
    assert (seen["watermark"], seen["watermark_key"], seen["watermark_strength"]) == ([3, 3], wu.KEY, 0.25) and eng._device_output()
    run([None, RequestOptions.checked(watermark_payload=9)], output_watermark_key=wu.KEY)
    assert seen["watermark"] == [0, 9]
    with pytest.raises(ValueError, match="output_watermark_key"):
        eng.synthesize_stream("xin chào")
    with pytest.raises(ValueError, match="needs a key"):
        run().detect_watermark(np.zeros(10, np.int16))


def test_header_version_script_and_exports_agree_for_the_new_entries():
    from vietvoice_tts_amd import build_ext, runtime
    hdr = open(os.path.join(ROOT, "include", "vvtts.h")).read()
    declared = set(re.findall(r"VV_API\s+[\w\s\*]+?\b(vv_\w+)\s*\(", hdr))
    assert declared == set(runtime.EXPORTS), declared ^ set(runtime.EXPORTS)
    ver = open(os.path.join(ROOT, "vietvoice-tts_amd", "csrc", "vvtts.map")).read()
    globs = [g.strip() for g in re.findall(r"global:\s*([^;]+);", ver)]
    lib = runtime.load_library()
    for name, n_args in (("vv_pcm_watermark", 17), ("vv_pcm_watermark_ws_bytes", 1), ("vv_pcm_watermark_detect", 17),
                         ("vv_pcm_watermark_detect_ws_bytes", 2)):
        assert name in declared and len(runtime.EXPORTS[name][1]) == n_args
        assert any(re.fullmatch(g.replace("*", ".*"), name) for g in globs) and hasattr(lib, name)
    assert "vv_watermark" in build_ext.SOURCES and "vv_denoise" in build_ext.SOURCES
    for name in ("vv_pcm_watermark", "vv_pcm_watermark_detect"):
        args = [None if t is ctypes.c_void_p else 0 for t in runtime.EXPORTS[name][1]]
        assert getattr(lib, name)(*args) == -22                                       # no context: refused before anything else
    assert len(runtime.EXPORTS["vv_pcm_denoise"][1]) == 19                            # the old entry keeps its arguments
    assert lib.vv_pcm_watermark_ws_bytes(4) >= 4 * 16
    assert lib.vv_pcm_watermark_detect_ws_bytes(50, 4) >= 50 * wu.K * 12 + 4 * 16 > lib.vv_pcm_watermark_detect_ws_bytes(5, 1) >= 5 * wu.K * 12
    m = re.match(rb"vvtts-hip (\d+)\.(\d+) ", lib.vv_version())
    assert m and (int(m.group(1)), int(m.group(2))) >= (0, 14)                        # bumped with the additive entries
    ap = _ap()
    for macro, value in (("VV_WATERMARK_LO", ap.WATERMARK_LO), ("VV_WATERMARK_K", ap.WATERMARK_K), ("VV_WATERMARK_G", ap.WATERMARK_G),
                         ("VV_WATERMARK_P", ap.WATERMARK_P), ("VV_WATERMARK_NB", ap.WATERMARK_NB),
                         ("VV_WATERMARK_DETECT_MAX_N", ap.WATERMARK_DETECT_MAX_N)):
        assert re.search(rf"#define {macro} {value}\b", hdr)
    for name in ("vv_denoise.hip", "vv_watermark.hip"):                              # the transform lives in one place
        src = open(os.path.join(ROOT, "vietvoice-tts_amd", "csrc", name)).read()
        assert '#include "vv_denoise_fft.h"' in src and "void two_stages(" not in src and "void transform(" not in src


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
        cfg.output_watermark_key, cfg.output_watermark_payload = wu.KEY, 0x1234
        with pytest.raises(ValueError, match="output_watermark_key"):
            eng.synthesize_stream(text)
        reseed()
        got, _ = eng.synthesize(text)
        want = ap.watermark_embed(base, wu.KEY, 0x1234, 0.2)
        assert np.array_equal(got, want) and not np.array_equal(want, base)
        assert eng.detect_watermark(got) == ap.watermark_detect(want, wu.KEY)         # the engine's key; on injected sessions the mirror answers
        both = eng.detect_watermark([got, base], key=wu.KEY)
        assert both[0] == ap.watermark_detect(want, wu.KEY) and not both[1].present
        cfg.output_loudness = -20.0                                                   # the later links see the marked signal
        reseed()
        assert np.array_equal(eng.synthesize(text)[0], ap.normalize_loudness(want, cfg.sample_rate, -20.0, cfg.output_peak_dbfs))
        cfg.output_loudness = None
        fe = BatchingFrontend(eng, overlap=False)
        try:
            reseed()
            own = fe.submit(text, watermark_payload=0xBEEF).result(timeout=300)[0]
            reseed()
            engines = fe.submit(text).result(timeout=300)[0]
        finally:
            fe.close()
        assert np.array_equal(own, ap.watermark_embed(base, wu.KEY, 0xBEEF, 0.2)) and np.array_equal(engines, want)
    finally:
        eng.cleanup()
