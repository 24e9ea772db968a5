"""RequestOptions: one record from BatchingFrontend.submit to the stage that consumes each value.

1. ``checked`` raises what the options' own check_* functions raise, in submit's order, and the same text arrives on the Future.
2. ``resolved`` against the rule written out as a table: a request's value, else the engine's.
3. What ``_finish_device`` hands to the output stage, and how a full stream chain (limiter -> rate -> FLAC) cuts its blocks, against
   tests/golden/request_options_golden.json, recorded before the options were one record (tests/golden/make_request_options_golden.py).
"""
import importlib.util
import json
import math
import os

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
_spec = importlib.util.spec_from_file_location("make_request_options_golden", os.path.join(HERE, "golden", "make_request_options_golden.py"))
gold_script = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(gold_script)
with open(gold_script.OUT, encoding="utf-8") as _f:
    GOLD = json.load(_f)

FIELDS = ("cfg_strength", "cfg_interval", "apg_eta", "apg_norm", "loudness", "limiter", "pitch", "tempo", "formants", "denoise")


@pytest.fixture(scope="module")
def model_dir(tmp_path_factory):
    return tmp_path_factory.mktemp("models")          # the synthetic tiny pack is written once


@pytest.fixture(scope="module")
def cpu_engine(model_dir):
    eng = gold_script.make_engine(model_dir)
    yield eng
    eng.cleanup()


# ------------------------------------------------------------------ 1. checked
def _original(field, bad):
    """The text of the check that ``submit`` has always run for this option."""
    from vietvoice_tts_amd.core import audio_processor as ap
    from vietvoice_tts_amd import model_spec
    if field == "cfg_strength":                  # the one rule without a function of its own (ModelConfig states it in the same words)
        return "cfg_strength must be a finite number or None"
    call = {"loudness": lambda: ap.check_loudness(bad), "limiter": lambda: ap.check_limiter(bad), "pitch": lambda: ap.check_prosody(bad, None),
            "tempo": lambda: ap.check_prosody(None, bad), "formants": lambda: ap.check_formants(bad), "denoise": lambda: ap.check_denoise(bad),
            "cfg_interval": lambda: model_spec.check_cfg_interval(bad), "apg_eta": lambda: model_spec.check_apg(bad, None),
            "apg_norm": lambda: model_spec.check_apg(None, bad)}[field]
    with pytest.raises(ValueError) as e:
        call()
    return str(e.value)


BAD = [("cfg_strength", math.nan), ("cfg_strength", math.inf), ("cfg_interval", (0.8, 0.2)), ("cfg_interval", 0.5), ("apg_eta", math.inf),
       ("apg_eta", "1"), ("apg_norm", 0.0), ("apg_norm", True), ("loudness", -4.0), ("loudness", "loud"), ("loudness", math.nan),
       ("limiter", "peak"), ("limiter", 1), ("pitch", 12.5), ("pitch", math.nan), ("tempo", 0.25), ("tempo", "fast"), ("formants", "move"),
       ("formants", 0), ("denoise", 0.0), ("denoise", 17.0), ("denoise", math.nan)]


def test_every_option_has_a_bad_value():
    assert {f for f, _b in BAD} == set(FIELDS)


@pytest.mark.parametrize("field,bad", BAD, ids=[f"{f}-{b!r}" for f, b in BAD])
def test_checked_raises_the_original_text(cpu_engine, field, bad):
    from vietvoice_tts_amd.batching import BatchingFrontend
    from vietvoice_tts_amd.request_options import RequestOptions
    want = _original(field, bad)
    with pytest.raises(ValueError) as e:
        RequestOptions.checked(**{field: bad})
    assert str(e.value) == want
    fe = BatchingFrontend(cpu_engine, overlap=False)
    try:
        err = fe.submit("x", **{field: bad}).exception(timeout=5)
    finally:
        fe.close()
    assert type(err) is ValueError and str(err) == want


def test_checked_reports_the_first_error_in_submits_order(cpu_engine):
    """submit's order: loudness, limiter, pitch and tempo, formants, denoise, cfg_interval, apg, cfg_strength."""
    from vietvoice_tts_amd.batching import BatchingFrontend
    from vietvoice_tts_amd.request_options import RequestOptions
    order = [("loudness", 0.0), ("limiter", "peak"), ("pitch", 99.0), ("tempo", 9.0), ("formants", "move"), ("denoise", -1.0),
             ("cfg_interval", (2.0, 3.0)), ("apg_eta", math.nan), ("apg_norm", -1.0), ("cfg_strength", math.nan)]
    fe = BatchingFrontend(cpu_engine, overlap=False)
    try:
        for i, (first, bad1) in enumerate(order):
            for second, bad2 in order[i + 1:]:
                want = _original(first, bad1)
                with pytest.raises(ValueError) as e:
                    RequestOptions.checked(**{first: bad1, second: bad2})
                assert str(e.value) == want, (first, second)
                assert str(fe.submit("x", **{first: bad1, second: bad2}).exception(timeout=5)) == want
    finally:
        fe.close()


def test_checked_normalises_as_submit_did():
    from vietvoice_tts_amd.request_options import RequestOptions
    o = RequestOptions.checked(cfg_strength=2, cfg_interval=[0, 1], apg_eta=0, apg_norm=3, loudness=-20, limiter="true", pitch=2, tempo=1,
                               formants="keep", denoise=1)
    assert o == RequestOptions(2.0, (0.0, 1.0), 0.0, 3.0, -20.0, "true", 2.0, 1.0, "keep", 1.0)
    for f in FIELDS:
        v = getattr(o, f)
        assert type(v) is (str if f in ("limiter", "formants") else tuple if f == "cfg_interval" else float), f
    assert type(o.cfg_interval[0]) is float and RequestOptions.checked() == RequestOptions()
    assert all(getattr(RequestOptions(), f) is None for f in FIELDS)
    with pytest.raises(Exception):
        o.pitch = 1.0                            # frozen


def test_the_module_imports_no_torch():
    src = open(os.path.join(os.path.dirname(HERE), "vietvoice-tts_amd", "request_options.py"), encoding="utf-8").read()
    assert "import torch" not in src and "from torch" not in src


# ------------------------------------------------------------------ 2. resolved
ENGINE_SET = dict(cfg_strength=1.5, cfg_interval=(0.2, 0.8), apg_eta=0.5, apg_norm=4.0, output_loudness=-23.0, output_limiter="true",
                  output_pitch=-2.0, output_tempo=1.25, output_formants="keep", output_denoise=2.0)
ENGINE_UNSET = dict(cfg_strength=None, cfg_interval=None, apg_eta=None, apg_norm=None, output_loudness=None, output_limiter=None,
                    output_pitch=None, output_tempo=None, output_formants="shift", output_denoise=None)      # formants has no "unset": "shift"
OWN_ALL = dict(cfg_strength=3.0, cfg_interval=(0.0, 0.5), apg_eta=0.0, apg_norm=1.0, loudness=-16.0, limiter="sample", pitch=5.0, tempo=0.75,
               formants="shift", denoise=8.0)
OWN_MIXED = dict(cfg_interval=(0.1, 0.9), apg_norm=2.0, loudness=-30.0, tempo=1.5, denoise=0.5)

# (engine, request) -> every field of the result, written out: the request's value where it has one, else the engine's
RESOLVED = {
    ("set", "none"): (1.5, (0.2, 0.8), 0.5, 4.0, -23.0, "true", -2.0, 1.25, "keep", 2.0),
    ("set", "all"): (3.0, (0.0, 0.5), 0.0, 1.0, -16.0, "sample", 5.0, 0.75, "shift", 8.0),
    ("set", "mixed"): (1.5, (0.1, 0.9), 0.5, 2.0, -30.0, "true", -2.0, 1.5, "keep", 0.5),
    ("unset", "none"): (None, None, None, None, None, None, None, None, "shift", None),
    ("unset", "all"): (3.0, (0.0, 0.5), 0.0, 1.0, -16.0, "sample", 5.0, 0.75, "shift", 8.0),
    ("unset", "mixed"): (None, (0.1, 0.9), None, 2.0, -30.0, None, None, 1.5, "shift", 0.5),
}


@pytest.mark.parametrize("engine,request_", sorted(RESOLVED))
def test_resolved_is_own_value_else_the_engines(model_dir, engine, request_):
    from vietvoice_tts_amd.core import ModelConfig
    from vietvoice_tts_amd.request_options import RequestOptions
    config = ModelConfig(model_cache_dir=str(model_dir), synthetic_model=True, model_spec="tiny", **{"set": ENGINE_SET, "unset": ENGINE_UNSET}[engine])
    own = RequestOptions.checked(**{"none": {}, "all": OWN_ALL, "mixed": OWN_MIXED}[request_])
    got = own.resolved(config)
    assert isinstance(got, RequestOptions)
    assert tuple(getattr(got, f) for f in FIELDS) == RESOLVED[engine, request_]
    assert got.resolved(config) == got           # nothing is left open
    assert own == RequestOptions.checked(**{"none": {}, "all": OWN_ALL, "mixed": OWN_MIXED}[request_])      # and the request's record is untouched


def test_wants_output_stage_and_column():
    from vietvoice_tts_amd.request_options import RequestOptions, column
    assert not RequestOptions().wants_output_stage()
    assert not RequestOptions(cfg_strength=2.0, cfg_interval=(0.0, 1.0), apg_eta=0.0, apg_norm=1.0, formants="keep").wants_output_stage()
    for f, v in (("loudness", -20.0), ("limiter", "true"), ("pitch", 0.0), ("tempo", 1.0), ("denoise", 1.0)):
        assert RequestOptions(**{f: v}).wants_output_stage(), f
    opts = [RequestOptions(pitch=2.0), RequestOptions(), RequestOptions(pitch=0.0, limiter="true")]
    assert column(opts, "pitch") == [2.0, None, 0.0] and column(opts, "limiter") == [None, None, "true"]
    assert column(opts, "tempo") is None and column([], "tempo") is None


# ------------------------------------------------------------------ 3. the hand-over to the output stage, and the stream chain
def test_finish_device_hands_over_what_it_did_before(cpu_engine):
    got = gold_script.record_handover(cpu_engine)
    want = GOLD["handover"]
    assert set(want) == set(gold_script.CONFIGS) and all(set(want[c]) == set(gold_script.BATCHES) for c in want)
    for cname in want:
        for bname in want[cname]:
            assert got[cname][bname] == want[cname][bname], (cname, bname)
    assert cpu_engine.model_session_manager.engine is None and cpu_engine.config.output_loudness is None      # the recorder is gone again
    # the golden file itself: the all-None batch of the unset engine calls nothing beyond the join, every option reaches its column
    plain = want["unset"]["three_plain"]
    assert plain["groups"] == [] and plain["pitch"] is None and plain["tempo"] is None and plain["denoise"] is None and plain["formants"] is None
    mixed = want["unset"]["everything_mixed"]
    assert mixed["pitch"] == [-5.0, None, None, 4.0] and mixed["tempo"] == [None, 1.5, None, 0.75] and mixed["denoise"] == [0.5, None, None, 8.0]
    assert mixed["formants"] == ["shift", "keep", "shift", "shift"]
    assert mixed["groups"] == [[None, [0], [-14.0]], ["sample", [3], [-27.0]], ["true", [1], [None]]]
    assert want["loud_lim_flac_lpc"]["engine_call"]["flac_lpc_order"] == 8 and want["all_set"]["one_plain"]["denoise_bias"] == gold_script.bias_digest(gold_script.BIAS)


def test_full_stream_chain_equals_buffered_and_cuts_the_same_blocks(model_dir):
    """Limiter -> output rate -> FLAC, all three stages at once: the blocks add up to synthesize()'s bytes, and there are as many, as
    large, as before the stages became a list.  "synthesize()'s bytes" for FLAC: every frame, byte for byte, and the samples they decode
    to.  The 42 bytes in front (marker + STREAMINFO) hold the total and the frame sizes, which a stream cannot know when it writes them
    and leaves at 0 (tests/test_flac_cpu.py compares from byte 42 in the same way)."""
    from tests.flac_util import decode_stream
    eng = gold_script.make_engine(model_dir, **gold_script.STREAM_CONFIG)
    try:
        assert (eng.config.output_limiter, eng.config.output_sample_rate, eng.config.output_encoding) == ("true", 8000, "flac")
        blocks, whole = gold_script.stream_run(eng)
        assert len(eng._last_plan) == GOLD["stream"]["chunks"] >= 3
    finally:
        eng.cleanup()
    assert all(b.dtype == np.uint8 and b.size for b in blocks) and whole.dtype == np.uint8
    streamed = np.concatenate(blocks)
    assert streamed.size == whole.size and np.array_equal(streamed[42:], whole[42:]) and np.array_equal(streamed[:4], whole[:4])
    got, _frames, sinfo = decode_stream(streamed)
    want, _frames, info = decode_stream(whole)
    assert np.array_equal(got, want) and want.size > 3 * 4096 and (sinfo["rate"], info["rate"], sinfo["total"], info["total"]) == (8000, 8000, 0, want.size)
    assert [int(b.size) for b in blocks] == GOLD["stream"]["block_sizes"]
