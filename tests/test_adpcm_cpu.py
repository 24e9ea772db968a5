"""N25 without a GPU: the host mirror of the IMA ADPCM encoder and of the ADPCM / G.711 decoders (core/audio_processor.py) against stdlib
audioop -- recorded in tests/golden/adpcm_golden.npz, and live where the interpreter still has it -- and against the plain-Python
reference of tests/adpcm_util.py; the container, the stream, the refusals, and the engine on oracle sessions.  The device is held against
the mirror in tests/test_adpcm_gpu.py.  On the commit before N25 every test here fails with ``output_encoding must be one of ...``,
``unsupported WAVE format tag ...`` or a missing name of the mirror."""
import hashlib
import os
import struct

import numpy as np
import pytest

from tests import adpcm_util as U

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = np.load(U.GOLDEN)


def _ap():
    from vietvoice_tts_amd.core import audio_processor
    return audio_processor


def _sha1(b):
    return np.frombuffer(hashlib.sha1(bytes(b)).digest(), np.uint8)


# ------------------------------------------------------------------ encoder
@pytest.fixture(scope="module")
def encoded():
    """{(spb, name): (x, the mirror's blocks)}: every input once."""
    ap = _ap()
    return {(spb, name): (x, ap.adpcm_encode_blocks(x, spb)) for spb in U.SPBS for name, x in U.encoder_inputs(spb)}


def _check_against_record(x, spb, got, best, err, carried, sha1_or_bytes):
    ba = (spb - 1) // 2 + 4
    blocks = U.pad_blocks(x, spb)
    assert got.dtype == np.uint8 and got.size == blocks.shape[0] * ba
    g = got.reshape(-1, ba)
    assert np.array_equal(g[:, :2].copy().view("<i2")[:, 0], blocks[:, 0]) and not g[:, 3].any()      # header: (x[first], idx, 0)
    assert np.array_equal(g[:, 2], best)                                                       # the smallest argmin over all 89 indices
    assert (err <= carried).all()                                                              # no block worse than the carried-state encoder
    if isinstance(sha1_or_bytes, bytes):
        assert got.tobytes() == sha1_or_bytes
    else:
        assert np.array_equal(_sha1(got), sha1_or_bytes)


def test_encoder_equals_the_recorded_audioop_search_byte_for_byte(encoded):
    assert len(encoded) == 3 * 10
    assert GOLD["check"].tobytes().hex() == "7f7a"
    for (spb, name), (x, got) in encoded.items():
        k = f"enc_{spb}_{name}_"
        _check_against_record(x, spb, got, GOLD[k + "best"], GOLD[k + "err"], GOLD[k + "carried"], GOLD[k + "sha1"])


def test_encoder_equals_live_audioop(encoded):
    audioop = pytest.importorskip("audioop")
    assert audioop.lin2adpcm(np.array([1000, -1000, 3000, 0], np.int16).tobytes(), 2, (0, 20))[0].hex() == "7f7a"
    for (spb, name), (x, got) in encoded.items():
        best, err, carried, data = U.audioop_encoder_record(audioop, x, spb)
        _check_against_record(x, spb, got, best, err, carried, data)


def test_encoder_equals_the_plain_python_reference_and_reports_its_error(encoded):
    ap = _ap()
    for (spb, name), (x, got) in encoded.items():
        if spb != 505:
            continue                                          # pure-Python loops: the smallest block size only
        ba = (spb - 1) // 2 + 4
        blocks, best, err = ap.adpcm_choose(x, spb)
        for b, blk in enumerate(blocks):
            real = min(max(x.size - b * spb - 1, 0), spb - 1)
            codes, recon = U.ref_encode(blk[1:], blk[0], int(best[b]))
            assert int(((blk[1:] - np.array(recon, np.int64))[:real] ** 2).sum()) == err[b], (name, b)
            packed = bytes(codes[i] | (codes[i + 1] << 4) for i in range(0, len(codes), 2))              # low nibble first
            assert got[b * ba + 4: (b + 1) * ba].tobytes() == packed, (name, b)


def test_silence_ties_at_every_index_and_index_zero_wins(encoded):
    for spb in U.SPBS:
        x, got = encoded[(spb, "silence")]
        assert not got.any()                                  # header (0, 0, 0) and codes 0: the predictor never leaves 0


def test_square_wave_reaches_the_predictor_clamp(encoded):
    ap = _ap()
    for spb in U.SPBS:
        x, got = encoded[(spb, "square")]
        assert x.min() == -32768 and x.max() == 32767
        y = ap.adpcm_decode_blocks(got, spb, x.size)
        assert y.min() == -32768 and y.max() == 32767         # the reconstruction sits on both ends of the range


def test_empty_input_follows_the_other_encodings():
    ap = _ap()
    empty = np.zeros(0, np.int16)
    assert ap.encode_output(empty, "ulaw").size == 0 and ap.adpcm_encode_blocks(empty, 505).size == 0
    f = ap.encode_output(empty, "adpcm", 8000)                # like "flac": a file is a header alone
    assert f.dtype == np.uint8 and f.size == ap.ADPCM_HEADER_BYTES == 60
    frames, width, rate = ap._decode_wav(f.tobytes())
    assert frames.shape == (0, 1) and width == 2 and rate == 8000


def test_round_trip_has_the_length_and_equals_the_reference_decode(encoded):
    ap = _ap()
    for (spb, name), (x, got) in encoded.items():
        y = ap.adpcm_decode_blocks(got, spb, x.size)
        assert y.dtype == np.int16 and y.size == x.size
        ba = (spb - 1) // 2 + 4
        if spb == 505:
            assert np.array_equal(y, U.ref_adpcm_frames(got.tobytes(), 1, ba)[: x.size, 0]), name
        assert y[0] == x[0] and np.array_equal(ap.adpcm_decode_blocks(got, spb)[: x.size], y)


def test_round_trip_equals_live_audioop(encoded):
    audioop = pytest.importorskip("audioop")
    ap = _ap()
    for (spb, name), (x, got) in encoded.items():
        want = U.audioop_adpcm_frames(audioop, got.tobytes(), 1, (spb - 1) // 2 + 4)[: x.size, 0]
        assert np.array_equal(ap.adpcm_decode_blocks(got, spb, x.size), want), (spb, name)


def test_stream_equals_the_whole_signal_for_every_split(encoded):
    ap = _ap()
    rng = np.random.default_rng(3)
    for spb, rate in U.RATE_OF_SPB.items():
        x, whole = encoded[(spb, f"speech_{3 * spb + 7}")]
        cuts = np.sort(rng.integers(0, x.size, 9))
        splits = [np.split(x, range(k, x.size, k)) for k in (1, 100, 505, 1017, 4096)] + [np.split(x, cuts)]
        for parts in (splits if spb == 505 else splits[1:]):  # the split of size 1 at the smallest block size only: it is the slow one
            s = ap.AdpcmStream(rate)
            out = [s.push(p) for p in parts] + [s.flush()]
            assert all(o.dtype == np.uint8 and o.size % ((spb - 1) // 2 + 4) == 0 for o in out)
            assert np.array_equal(np.concatenate(out), whole)
        assert ap.AdpcmStream(rate).flush().size == 0


def test_container_fields_and_save_audio(encoded, tmp_path):
    ap = _ap()
    for spb, rate in ((505, 8000), (505, 16000), (1017, 22050), (1017, 24000), (2041, 44100), (2041, 48000)):
        assert ap.adpcm_block_align(rate) == 256 * max(1, rate // 11025) and ap.adpcm_samples_per_block(ap.adpcm_block_align(rate)) == spb
        x, blocks = encoded[(spb, f"speech_{3 * spb + 7}")]
        f = ap.encode_output(x, "adpcm", rate)
        raw = f.tobytes()
        ba = 256 * max(1, rate // 11025)
        assert raw[:4] == b"RIFF" and struct.unpack("<I", raw[4:8])[0] == len(raw) - 8 and raw[8:16] == b"WAVEfmt "
        assert struct.unpack("<IHHIIHHHH", raw[16:40]) == (20, 0x11, 1, rate, rate * ba // spb, ba, 4, 2, spb)
        assert raw[40:44] == b"fact" and struct.unpack("<II", raw[44:52]) == (4, x.size)
        assert raw[52:56] == b"data" and struct.unpack("<I", raw[56:60])[0] == blocks.size and raw[60:] == blocks.tobytes()
        path = tmp_path / f"a{rate}.wav"
        ap.AudioProcessor.save_audio(f, str(path), rate, "adpcm")
        assert path.read_bytes() == raw == ap.AudioProcessor.to_wav_bytes(f, rate, "adpcm")
        frames, width, got_rate = ap._decode_wav(path.read_bytes())
        assert width == 2 and got_rate == rate and np.array_equal(frames[:, 0], ap.adpcm_decode_blocks(blocks, spb, x.size))
        assert abs(ap.AudioProcessor.probe_duration(str(path)) - x.size / rate) < 1e-12
        assert np.array_equal(ap.adpcm_wav(blocks, rate, x.size), f)                          # a collected stream + its length = the file
    for bad in (np.zeros(100, np.int16), np.zeros(10, np.uint8), blocks):                      # PCM, too short, raw blocks without a header
        with pytest.raises(ValueError):
            ap.AudioProcessor.save_audio(bad, str(tmp_path / "bad.wav"), 8000, "adpcm")
        with pytest.raises(ValueError):
            ap.AudioProcessor.to_wav_bytes(bad, 8000, "adpcm")
    with pytest.raises(ValueError):
        ap.adpcm_block_align(11025 * 17)                      # blocks above VV_ADPCM_MAX_BLOCK_ALIGN
    with pytest.raises(ValueError):
        ap.adpcm_encode_blocks(x, 506)
    with pytest.raises(ValueError):
        ap.OutputStream(24000, None, "adpcm")


# ------------------------------------------------------------------ decoder
def _g711_want(tag, codes, table=None):
    table = GOLD["ulaw2lin" if tag == 7 else "alaw2lin"] if table is None else table
    return table[codes]


def test_g711_tables_equal_audioop_for_all_256_codes():
    ap = _ap()
    codes = np.arange(256, dtype=np.uint8)
    assert np.array_equal(ap.ulaw2lin(codes), GOLD["ulaw2lin"]) and np.array_equal(ap.alaw2lin(codes), GOLD["alaw2lin"])
    assert np.array_equal(ap.lin2ulaw(GOLD["ulaw2lin"]), np.where(codes == 0x7F, 0xFF, codes))    # the coder's inverse (the two zeros share a code)
    audioop = pytest.importorskip("audioop")
    assert np.array_equal(ap.ulaw2lin(codes), np.frombuffer(audioop.ulaw2lin(codes.tobytes(), 2), np.int16))
    assert np.array_equal(ap.alaw2lin(codes), np.frombuffer(audioop.alaw2lin(codes.tobytes(), 2), np.int16))


def test_decoder_files_equal_the_references():
    ap = _ap()
    files = U.decoder_files()
    assert len(files) >= 24
    for name, data, want, rate in files:
        frames, width, got_rate = ap._decode_wav(data)
        assert width == 2 and got_rate == rate and frames.dtype == np.int16, name
        if isinstance(want, tuple):
            assert np.array_equal(frames, _g711_want(*want)), name
        else:
            assert np.array_equal(frames, want), name
            assert np.array_equal(_sha1(frames.astype("<i2").tobytes()), GOLD[f"dec_{name}_sha1"]), name
        assert abs(ap.AudioProcessor.probe_duration(data) - frames.shape[0] / rate) < 1e-12
    by = {f[0]: f for f in files}
    assert ap._decode_wav(by["adpcm_fact"][1])[0].shape[0] == 40 and ap._decode_wav(by["alaw_fact"][1])[0].shape[0] == 100     # the fact cap
    assert [ap._decode_wav(by[f"adpcm_part_{c}"][1])[0].shape[0] for c in (1, 7, 8, 9, 12, 13, 19, 31)] == [50, 50, 51, 51, 51, 53, 59, 73]
    assert [ap._decode_wav(by[f"adpcm_mono_part_{c}"][1])[0].shape[0] for c in (3, 4, 5, 15)] == [50, 51, 53, 73]


def test_decoder_files_equal_live_audioop():
    audioop = pytest.importorskip("audioop")
    ap = _ap()
    for name, data, want, _rate in U.decoder_files():
        w = U.parse_wav(data)
        if isinstance(want, tuple):
            fn = audioop.ulaw2lin if want[0] == 7 else audioop.alaw2lin
            ref = np.frombuffer(fn(want[1].tobytes(), 2), np.int16).reshape(want[1].shape)
        else:
            ref = U.audioop_adpcm_frames(audioop, w["payload"], w["channels"], w["block_align"], w["fact"])
        assert np.array_equal(ap._decode_wav(data)[0], ref), name


def test_refusals_carry_a_reason_and_a_byte():
    ap = _ap()
    S = ap.WavStatus
    for ch in (1, 2):
        data, at = U.bad_index_file(ch)
        with pytest.raises(ap.WavError) as e:
            ap._decode_wav(data)
        assert (e.value.code, e.value.position) == (S.STEP_INDEX, at) and f"at byte {at}" in str(e.value)
        ok = bytearray(data)
        ok[at] = 88
        ap._decode_wav(bytes(ok))                             # 88 is the last valid index
    pay = bytes(64)
    cases = [
        (U.wav_file(0x11, 1, 8000, 4, 4, pay), S.BLOCK_ALIGN, 12),       # smaller than header + one group
        (U.wav_file(0x11, 2, 8000, 8, 4, pay), S.BLOCK_ALIGN, 12),
        (U.wav_file(0x11, 2, 8000, 20, 4, pay), S.BLOCK_ALIGN, 12),      # not a multiple of 4 x channels
        (U.wav_file(0x11, 1, 8000, 18, 4, pay), S.BLOCK_ALIGN, 12),
        (U.wav_file(0x11, 1, 8000, 16, 3, pay), S.BITS, 14),
        (U.wav_file(0x11, 1, 8000, 16, 8, pay), S.BITS, 14),
        (U.wav_file(7, 1, 8000, 1, 16, pay), S.BITS, 14),
        (U.wav_file(6, 1, 8000, 1, 4, pay), S.BITS, 14),
        (U.wav_file(0x11, 3, 8000, 48, 4, pay), S.CHANNELS, 2),
        (U.wav_file(0x11, 2, 8000, 16, 3, pay, extensible=True), S.BITS, 14),
    ]
    for data, code, field in cases:
        with pytest.raises(ap.WavError) as e:
            ap._decode_wav(data)
        assert (e.value.code, e.value.position) == (code, 20 + field), (code, field)           # the fmt chunk's body starts at byte 20
        with pytest.raises(ValueError):
            ap.AudioProcessor.probe_duration(data)
    with pytest.raises(ValueError, match="unsupported WAVE format tag 2"):
        ap._decode_wav(U.wav_file(2, 1, 8000, 256, 4, pay))                                    # MS-ADPCM stays out of scope


def test_every_truncation_decodes_or_refuses():
    ap = _ap()
    for name, data, data_at in U.small_files():
        full = ap._decode_wav(data)[0]
        assert full.shape[0] == 75
        for cut in range(len(data)):
            try:
                frames, width, rate = ap._decode_wav(data[:cut])
            except ValueError:
                assert cut < data_at                         # only the container can be too short to say anything
                continue
            assert width == 2 and frames.shape[0] <= 75 and np.array_equal(frames, full[: frames.shape[0]]), (name, cut)
            ch = full.shape[1]
            assert frames.shape[0] == min(75, ap.adpcm_frame_count(cut - data_at, ch, 16 * ch))


# ------------------------------------------------------------------ plans and plumbing
def test_plans_refuse_what_the_kernels_must_not_see():
    from vietvoice_tts_amd.pcm_stage import plan_adpcm, plan_wav_decode
    assert plan_adpcm([[3, 1000, 0], [2000, 505, 512]], 4000, 505) == (505, [[3, 1000, 0], [2000, 505, 512]], 768, 2)
    for rows, spb, n_y in (([[0, 0, 0]], 505, None), ([[0, 10, 2]], 505, None), ([[3990, 11, 0]], 505, None), ([[0, 10, 0]], 504, None),
                           ([[0, 600, 0], [0, 10, 256]], 505, None), ([[0, 10, 0]], 505, 255), ([[0, 10, 0]], 8193, None)):
        with pytest.raises(ValueError):
            plan_adpcm(rows, 4000, spb, n_y)
    good = [[0, 512, 0x11, 1, 256, 1010, 0], [512, 100, 7, 2, 2, 50, 2032]]
    assert plan_wav_decode(good, 1024, 4096) == [r + [0] for r in good]
    for k, v in ((0, 8), (1, 1100), (2, 2), (3, 3), (4, 6), (5, 1011), (6, 8)):
        bad = [list(good[0]), list(good[1])]
        bad[0][k] = v
        with pytest.raises(ValueError):
            plan_wav_decode(bad, 1024, 4096)
    with pytest.raises(ValueError):
        plan_wav_decode([good[1], good[0]], 1024, 4096)       # not ascending on pcm


def test_header_exports_and_enum_agree():
    import ctypes
    import re
    from vietvoice_tts_amd import build_ext, runtime
    ap = _ap()
    hdr = open(os.path.join(ROOT, "include", "vvtts.h")).read()
    declared = set(re.findall(r"VV_API\s+[\w\s\*]+?\b(vv_\w+)\s*\(", hdr))
    assert declared == set(runtime.EXPORTS), declared ^ set(runtime.EXPORTS)
    lib = runtime.load_library()
    for name in ("vv_pcm_adpcm", "vv_wav_decode"):
        assert name in declared and len(runtime.EXPORTS[name][1]) == 10 and hasattr(lib, name)
        args = [None if t is ctypes.c_void_p else 0 for t in runtime.EXPORTS[name][1]]
        assert getattr(lib, name)(*args) == -22               # no context: refused before anything else
    assert "vv_adpcm" in build_ext.SOURCES and "adpcm" in ap.OUTPUT_ENCODINGS
    codes = dict(re.findall(r"VV_WAV_(\w+) = (\d+)", hdr))
    for name in ("OK", "STEP_INDEX", "BLOCK_ALIGN", "BITS", "CHANNELS"):
        assert int(codes[name]) == getattr(ap.WavStatus, name)
    assert int(re.search(r"#define VV_ADPCM_MAX_BLOCK_ALIGN (\d+)", hdr).group(1)) == ap.ADPCM_MAX_BLOCK_ALIGN
    assert int(re.search(r"#define VV_WAVE_TAG_ADPCM (\d+)", hdr).group(1)) == ap.ADPCM_WAVE_TAG
    m = re.match(rb"vvtts-hip (\d+)\.(\d+) ", lib.vv_version())
    assert m and (int(m.group(1)), int(m.group(2))) >= (0, 15)
    src = open(os.path.join(ROOT, "vietvoice-tts_amd", "csrc", "vv_adpcm.hip")).read()
    assert [int(v) for v in re.search(r"kSteps\[NCAND\] = \{([^}]+)\}", src).group(1).split(",")] == ap.ADPCM_STEPS.tolist() == U.STEPS
    assert "atomic" not in src.split("namespace {")[1] and "float" not in src.split("namespace {")[1] and "double" not in src.split("namespace {")[1]


# ------------------------------------------------------------------ engine on injected oracle sessions
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


def test_engine_on_oracle_sessions_writes_streams_and_reads_back_adpcm(cpu_engine, tmp_path):
    ap = _ap()
    eng, cfg = cpu_engine, cpu_engine.config
    SR = cfg.sample_rate
    voice = (cfg.gender, cfg.group, cfg.area, cfg.emotion)
    _reseed(eng)
    base, _ = eng.synthesize(TEXT)
    assert len(eng._last_plan) > 1 and base.dtype == np.int16 and base.size > 3 * 1017
    try:
        cfg.output_encoding = "adpcm"
        assert not eng._device_output()                      # injected sessions: the host mirror
        _reseed(eng)
        path = tmp_path / "x.wav"
        got, _ = eng.synthesize(TEXT, output_path=str(path))
        assert got.dtype == np.uint8 and path.read_bytes() == got.tobytes()
        assert np.array_equal(got, ap.encode_output(base, "adpcm", SR))                       # the mirror of the pcm16 result
        _reseed(eng)
        blocks = list(eng.synthesize_stream(TEXT))
        assert len(blocks) > 1 and all(b.dtype == np.uint8 for b in blocks)
        assert np.array_equal(np.concatenate(blocks), got[60:])                               # the file's data chunk, byte for byte
        # the place in the chain: join -> limiter -> rate -> ADPCM
        cfg.output_limiter, cfg.output_sample_rate = "sample", 8000
        want = ap.encode_output(ap.resample_output(ap.limit_peaks(base, SR, cfg.output_peak_dbfs, "sample")[0], SR, 8000), "adpcm", 8000)
        _reseed(eng)
        chain, _ = eng.synthesize(TEXT)
        assert np.array_equal(chain, want)
        _reseed(eng)
        assert np.array_equal(np.concatenate(list(eng.synthesize_stream(TEXT))), want[60:])
        cfg.output_limiter, cfg.output_sample_rate = None, None
        # the engine's own files as reference clips: they load to the samples their decode says
        for enc in ("adpcm", "ulaw"):
            cfg.output_encoding = enc
            cfg.gender, cfg.group, cfg.area, cfg.emotion = voice
            _reseed(eng)
            p = tmp_path / f"own_{enc}.wav"
            made, _ = eng.synthesize("Xin chào các bạn.", output_path=str(p))                   # short enough to be a reference clip
            samples = ap.ulaw2lin(made) if enc == "ulaw" else ap.adpcm_decode_blocks(made[60:], 1017, struct.unpack("<I", made[48:52].tobytes())[0])
            frames, width, rate = ap.AudioProcessor.decode(str(p))
            assert width == 2 and rate == SR and np.array_equal(frames[:, 0], samples)
            want_clip = ap.AudioProcessor.normalize_to_int16(samples.astype(np.float32))
            assert np.array_equal(ap.AudioProcessor.load_audio(str(p), SR), want_clip)
            cfg.output_encoding = "pcm16"
            cfg.gender = cfg.group = cfg.area = cfg.emotion = None                            # a user clip excludes the config's voice filters
            _reseed(eng)
            out, _ = eng.synthesize("Xin chào.", reference_audio=str(p), reference_text="hôm nay trời đẹp quá")
            assert out.dtype == np.int16 and out.size > 0
    finally:
        cfg.output_encoding, cfg.output_limiter, cfg.output_sample_rate = "pcm16", None, None
        cfg.gender, cfg.group, cfg.area, cfg.emotion = voice
