"""N10, the output stage: host mirrors, join planning, config and WAV plumbing -- everything that needs no GPU.

The join itself is pinned to the reference's own function by tests/golden/output_golden.npz (tests/golden/make_output_golden.py runs it);
G.711 to stdlib audioop over all 65,536 inputs; the rate conversion to scipy.signal.resample_poly within 1 LSB."""
import ctypes
import os
import re
import struct

import numpy as np
import pytest

from tests.output_util import emulate_join, golden, join_cases, lsb_condition, pack_requests, scipy_resample

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RATES = [8000, 16000, 22050, 44100, 48000]
LONG = "Hôm nay trời đẹp quá, chúng ta cùng nhau đi dạo quanh hồ nhé. " * 3


# ------------------------------------------------------------------ G.711
def test_g711_mirrors_equal_the_tables():
    from vietvoice_tts_amd.core.audio_processor import lin2alaw, lin2ulaw
    _meta, arr = golden()
    every = np.arange(-32768, 32768, dtype=np.int16)
    u, a = lin2ulaw(every), lin2alaw(every)
    assert u.dtype == np.uint8 and a.dtype == np.uint8
    assert np.array_equal(u, arr["g711_ulaw"]) and np.array_equal(a, arr["g711_alaw"])
    try:
        import audioop
    except ImportError:          # removed from the standard library in 3.13: the tables above are its output
        return
    assert u.tobytes() == audioop.lin2ulaw(every.tobytes(), 2) and a.tobytes() == audioop.lin2alaw(every.tobytes(), 2)


# ------------------------------------------------------------------ output rate
@pytest.mark.parametrize("dst", RATES)
def test_resample_output_against_scipy(dst):
    """Float64 accumulation error is ~1e-10 LSB, so only a value sitting on a tie can flip: at most 1 LSB, at most 1 sample in 10^4."""
    from vietvoice_tts_amd.core.audio_processor import output_design, resample_len, resample_output
    x = golden()[1]["poly_x"]
    taps, up, down, _skip = output_design(24000, dst)
    for n in (1, 2, down - 1, down, down + 1, x.size):
        if n < 1:
            continue
        y = resample_output(x[:n], 24000, dst)
        assert y.dtype == np.int16 and y.size == resample_len(n, up, down) == -(-n * up // down)
        n_diff = lsb_condition(y, scipy_resample(x[:n], up, down))
        print(f"24000 -> {dst}: {n} samples in, {y.size} out, {n_diff} differ from scipy")
    assert np.shares_memory(resample_output(x, 24000, 24000), x)          # equal rates: the samples themselves


@pytest.mark.parametrize("dst", [8000, 44100])
def test_output_stream_blocks_equal_the_whole_clip(dst):
    from vietvoice_tts_amd.core.audio_processor import OutputStream, encode_output, resample_output
    x = golden()[1]["poly_x"]
    for enc in ("pcm16", "ulaw"):
        whole = encode_output(resample_output(x, 24000, dst), enc)
        for block in (1, 7, 997, 6007):
            xs = x[:300] if block == 1 else x
            want = whole if block != 1 else encode_output(resample_output(xs, 24000, dst), enc)
            s = OutputStream(24000, dst, enc)
            got = np.concatenate([s.push(xs[i: i + block]) for i in range(0, xs.size, block)] + [s.flush()])
            assert got.dtype == want.dtype and np.array_equal(got, want), (dst, enc, block)
            assert s.hist.size <= 2 * (s.taps.size // s.up + 2)          # only the filter's reach is kept


# ------------------------------------------------------------------ join planning
def test_host_mirror_equals_the_fixture():
    from vietvoice_tts_amd.core import AudioProcessor
    names = set()
    for name, sr, d, chunks, want in join_cases():
        got = np.asarray(AudioProcessor.concatenate_with_crossfade_improved([c.copy() for c in chunks], d, sr))
        assert got.dtype == want.dtype and np.array_equal(got, want), name
        names.add(name)
    for n in (1, 7, 8, 9, 127, 128, 129, 2400, 8192, 8193, 21600):
        assert f"n{n}_set0" in names
    assert {"clip_32767", "neg_32768_only", "rms_below_100", "gain_0.7", "gain_1.5", "gain_between", "wrap", "no_crossfade",
            "single_chunk_32767"} <= names
    wrap = next(m for m in golden()[0]["join"] if m["name"] == "wrap")
    assert wrap["sign_flips_last_2400"] > 100          # the gain of 1.5 wraps: the fixture holds the case


def test_join_plan_writes_every_sample_once():
    """vv_join_chunks's algorithm in numpy, driven by runtime.plan_join's rows (positions, junction sizes, final owners): it gives the
    fixture's samples, writes every output sample exactly once and nothing else -- alone and with all cases in one call."""
    from vietvoice_tts_amd.runtime import plan_join
    cases = join_cases()
    for name, sr, d, chunks, want in cases:
        plane, reqs = pack_requests([chunks])
        out, cnt, offs, lens = emulate_join(plane, reqs, d, sr, plan_join)
        assert lens == [want.size] and np.array_equal(out[offs[0]: offs[0] + lens[0]], want), name
        assert (cnt[offs[0]: offs[0] + lens[0]] == 1).all() and cnt.sum() == lens[0], name
    same = [c for c in cases if c[1] == 16000 and abs(c[2] - 0.008) < 1e-9]
    assert len(same) >= 5
    plane, reqs = pack_requests([c[3] for c in same])
    out, cnt, offs, lens = emulate_join(plane, reqs, 0.008, 16000, plan_join)
    for (name, _sr, _d, _c, want), o, n in zip(same, offs, lens):
        assert o % 8 == 0 and n == want.size and np.array_equal(out[o: o + n], want), name
    assert cnt.sum() == sum(lens) and cnt.max() == 1


def test_join_plan_refusals():
    from vietvoice_tts_amd.runtime import JOIN_MAX_N, plan_join
    with pytest.raises(ValueError, match="empty chunk"):
        plan_join([[(0, 10), (10, 0)]], 0.1, 24000)
    with pytest.raises(ValueError, match="without chunks"):
        plan_join([[]], 0.1, 24000)
    with pytest.raises(ValueError, match="more than"):
        plan_join([[(0, 60000), (60000, 60000)]], (JOIN_MAX_N + 1) / 24000 + 1e-9, 24000)
    rows, reqs, lens, ns, total = plan_join([[(0, 0)], [(0, 100), (100, 1), (101, 100)]], 50 / 24000 + 1e-12, 24000)
    assert lens == [0, 100 - 1 + 1 - 50 + 100] and ns == [1, 50] and reqs[1][2] % 8 == 0
    assert [r[2] for r in rows[1:]] == [0, 99, 50] and [r[4] for r in rows[1:]] == [50, 50, (1 << 63) - 1]


# ------------------------------------------------------------------ config
def test_config_validation_and_round_trip(tmp_path):
    from vietvoice_tts_amd.core import ModelConfig
    base = dict(model_cache_dir=str(tmp_path), synthetic_model=True, model_spec="tiny")
    c = ModelConfig(**base)
    assert (c.output_stage, c.output_sample_rate, c.output_encoding) == ("host", None, "pcm16")
    c = ModelConfig(output_stage="device", output_sample_rate=8000, output_encoding="ulaw", **base)
    d = c.to_dict()
    assert (d["output_stage"], d["output_sample_rate"], d["output_encoding"]) == ("device", 8000, "ulaw")
    assert ModelConfig.from_dict(d).to_dict() == d
    assert ModelConfig(output_sample_rate=16000.0, **base).output_sample_rate == 16000
    for bad in (dict(output_stage="gpu"), dict(output_encoding="mp3"), dict(output_sample_rate=0), dict(output_sample_rate=8000.5),
                dict(output_sample_rate=True), dict(output_sample_rate=10 ** 7)):
        with pytest.raises(ValueError):
            ModelConfig(**base, **bad)


# ------------------------------------------------------------------ engine plumbing on oracle sessions
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


def test_engine_rate_and_encoding_on_oracle_sessions(cpu_engine, tmp_path):
    from vietvoice_tts_amd.core.audio_processor import lin2ulaw, output_design, resample_output
    eng = cpu_engine
    assert not eng._device_output()                     # injected sessions: the host mirrors
    _reseed(eng)
    base, _ = eng.synthesize(LONG)
    assert base.dtype == np.int16 and len(eng._last_plan) > 1
    try:
        for rate, enc in ((8000, "ulaw"), (44100, "pcm16"), (None, "alaw"), (24000, "pcm16")):
            eng.config.output_sample_rate, eng.config.output_encoding = rate, enc
            _reseed(eng)
            path = tmp_path / f"o_{rate}_{enc}.wav"
            whole, secs = eng.synthesize(LONG, output_path=str(path))
            dst = rate or 24000
            _taps, up, down, _skip = output_design(24000, dst) if dst != 24000 else (None, 1, 1, 0)
            assert whole.size == -(-base.size * up // down) and secs > 0
            assert whole.dtype == (np.int16 if enc == "pcm16" else np.uint8)
            if (rate, enc) == (8000, "ulaw"):
                assert np.array_equal(whole, lin2ulaw(resample_output(base, 24000, 8000)))
            if (rate, enc) == (24000, "pcm16"):
                assert np.array_equal(whole, base)
            tag, _ch, wav_rate, bits, data = _parse_wav(path.read_bytes())
            assert wav_rate == dst and data == whole.tobytes() and tag == {"pcm16": 1, "alaw": 6, "ulaw": 7}[enc]
            for step in (1, 2):
                _reseed(eng)
                blocks = list(eng.synthesize_stream(LONG, chunks_per_step=step))
                got = np.concatenate(blocks)
                assert got.dtype == whole.dtype and np.array_equal(got, whole), (rate, enc, step)
    finally:
        eng.config.output_sample_rate, eng.config.output_encoding = None, "pcm16"


def test_front_end_on_oracle_sessions_applies_the_options(cpu_engine):
    from vietvoice_tts_amd.batching import BatchingFrontend
    eng = cpu_engine
    _reseed(eng)
    base, _ = eng.synthesize("Xin chào.")
    eng.config.output_sample_rate, eng.config.output_encoding = 16000, "alaw"
    fe = BatchingFrontend(eng, overlap=False)
    try:
        _reseed(eng)
        out = fe.submit("Xin chào.").result(timeout=300)[0]
    finally:
        fe.close()
        eng.config.output_sample_rate, eng.config.output_encoding = None, "pcm16"
    assert out.dtype == np.uint8 and out.size == -(-base.size * 2 // 3)


# ------------------------------------------------------------------ WAV headers, parsed by hand
def _parse_wav(data):
    assert data[:4] == b"RIFF" and data[8:12] == b"WAVE" and struct.unpack("<I", data[4:8])[0] == len(data) - 8
    pos, chunks = 12, {}
    while pos + 8 <= len(data):
        cid, size = data[pos: pos + 4], struct.unpack("<I", data[pos + 4: pos + 8])[0]
        chunks[cid] = data[pos + 8: pos + 8 + size]
        pos += 8 + size + (size & 1)
    assert pos == len(data)
    fmt = chunks[b"fmt "]
    tag, ch, rate, byte_rate, align, bits = struct.unpack("<HHIIHH", fmt[:16])
    if tag == 0xFFFE:
        tag = struct.unpack("<H", fmt[24:26])[0]
    assert ch == 1 and align == bits // 8 and byte_rate == rate * align
    if tag in (6, 7):
        assert bits == 8 and len(fmt) == 18 and struct.unpack("<I", chunks[b"fact"])[0] == len(chunks[b"data"])
    return tag, ch, rate, bits, chunks[b"data"]


def test_wav_headers_for_tags_1_6_7(tmp_path):
    from vietvoice_tts_amd.core import AudioProcessor
    from vietvoice_tts_amd.core.audio_processor import lin2alaw, lin2ulaw
    pcm = (np.arange(-500, 501) * 60).astype(np.int16)          # an odd number of samples: the G.711 data chunk is padded
    assert AudioProcessor.to_wav_bytes(pcm, 24000) == AudioProcessor.to_wav_bytes(pcm, 24000, "pcm16")
    assert _parse_wav(AudioProcessor.to_wav_bytes(pcm, 16000)) == (1, 1, 16000, 16, pcm.tobytes())
    for enc, tag, fn in (("ulaw", 7, lin2ulaw), ("alaw", 6, lin2alaw)):
        codes = fn(pcm)
        assert _parse_wav(AudioProcessor.to_wav_bytes(codes, 8000, enc)) == (tag, 1, 8000, 8, codes.tobytes())
        p = tmp_path / f"{enc}.wav"
        AudioProcessor.save_audio(codes, str(p), 8000, enc)
        assert p.read_bytes() == AudioProcessor.to_wav_bytes(codes, 8000, enc)
        with pytest.raises(ValueError):
            AudioProcessor.save_audio(pcm, str(p), 8000, enc)          # int16 handed over as G.711
    p = tmp_path / "pcm.wav"
    AudioProcessor.save_audio(pcm, str(p), 44100)
    assert _parse_wav(p.read_bytes()) == (1, 1, 44100, 16, pcm.tobytes())
    with pytest.raises(ValueError):
        AudioProcessor.save_audio(pcm, str(p), 8000, "mp3")


# ------------------------------------------------------------------ ABI
def test_header_version_script_and_exports_agree():
    from vietvoice_tts_amd import build_ext, runtime
    hdr = open(os.path.join(ROOT, "include", "vvtts.h")).read()
    declared = set(re.findall(r"VV_API\s+[\w\s\*]+?\b(vv_\w+)\s*\(", hdr))
    ver = open(os.path.join(ROOT, "vietvoice-tts_amd", "csrc", "vvtts.map")).read()
    globs = [g.strip() for g in re.findall(r"global:\s*([^;]+);", ver)]
    lib = runtime.load_library()
    for name, n_args in (("vv_join_chunks", 17), ("vv_pcm_resample", 14), ("vv_pcm_encode", 10)):
        assert name in declared and name in runtime.EXPORTS and len(runtime.EXPORTS[name][1]) == n_args
        assert any(re.fullmatch(g.replace("*", ".*"), name) for g in globs)
        assert hasattr(lib, name)
        args = [None if t is ctypes.c_void_p else 0 for t in runtime.EXPORTS[name][1]]
        assert getattr(lib, name)(*args) == -22                        # no context: refused before anything else
    assert "vv_output" in build_ext.SOURCES
    assert int(re.search(r"#define VV_JOIN_MAX_N (\d+)", hdr).group(1)) == runtime.JOIN_MAX_N
    m = re.match(rb"vvtts-hip (\d+)\.(\d+) ", lib.vv_version())
    assert m and (int(m.group(1)), int(m.group(2))) >= (0, 4)          # bumped with the additive entries
