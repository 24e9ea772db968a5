"""N15 without a GPU: the host mirror of the FLAC encoder (core/audio_processor.py: flac_choose, flac_encode_frames, flac_stream_header,
FlacStream) against a stand-alone decoder and a brute-force reference of the subframe sizes (tests/flac_util.py), and the plumbing
(config, file writers, engine on oracle sessions, ABI).  The device is held against the mirror in tests/test_flac_gpu.py."""
import ctypes
import os
import re
import time

import numpy as np
import pytest

from tests.flac_util import (BLOCK, LENGTHS, VERBATIM_TIES, best_subframe, crc_bits, decode_frames, decode_stream, device_cases, fixed_bits, mirror_layout,
                             signals, speechlike, stream_header)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SR = 24000


def _ap():
    from vietvoice_tts_amd.core import audio_processor
    return audio_processor


# ------------------------------------------------------------------ check values
def test_crc_check_values():
    ap = _ap()
    assert ap.flac_crc8(b"123456789") == 0xF4 and ap.flac_crc16(b"123456789") == 0xFEE8
    assert crc_bits(b"123456789", 0x07, 8) == 0xF4 and crc_bits(b"123456789", 0x8005, 16) == 0xFEE8      # the decoder's own CRC
    assert ap.flac_crc8(b"") == 0 and ap.flac_crc16(b"\0\0\0" + b"123456789") == 0xFEE8                  # leading zero bytes do not count
    assert ap.FLAC_BLOCK == BLOCK == 4096 and "flac" in ap.OUTPUT_ENCODINGS


# ------------------------------------------------------------------ round trip and coverage
@pytest.fixture(scope="module")
def encoded():
    """Every signal at every length: {(name, n): (pcm, file bytes, decoded samples, decoded frames)}, computed once."""
    ap, res = _ap(), {}
    for n in LENGTHS:
        for name, x in signals(n).items():
            data = ap.encode_output(x, "flac", SR)
            samples, frames, info = decode_stream(data)
            assert info["rate"] == SR and info["total"] == n and info["md5"] == bytes(16)
            res[(name, n)] = (x, data, samples, frames)
    return res


def test_round_trip_is_exact_for_every_signal_and_length(encoded):
    assert len(encoded) == 13 * len(LENGTHS)
    for (name, n), (x, data, samples, frames) in encoded.items():
        assert data.dtype == np.uint8 and samples.dtype == np.int16 and np.array_equal(samples, x), (name, n)
        assert len(frames) == -(-n // BLOCK), (name, n)


def test_the_mirror_chooses_what_the_decoder_reads(encoded):
    ap = _ap()
    for (name, n), (x, _data, _samples, frames) in encoded.items():
        for f, frame in enumerate(frames):
            kind, o, po, ks, bits = ap.flac_choose(x[f * BLOCK: (f + 1) * BLOCK])
            assert frame[:4] == (kind, o, po, ks), (name, n, f)
            assert all(isinstance(k, int) and 0 <= k <= 14 for k in frame[3]), "the escape code is never written"
            m = min(BLOCK, n - f * BLOCK)
            assert frame[4] <= ap.flac_frame_bound(m) <= 16 + 1 + 2 * m + 2


def test_every_path_occurs(encoded):
    """The coverage the issue asks for, on the mirror's own choices for the one-frame signals."""
    ap = _ap()
    want = dict(zeros=("constant", 0, 0), floor=("constant", 0, 0), noise8=("fixed", 0, None), walk20=("fixed", 1, None), ramp=("fixed", 2, None),
                sine200=("fixed", 3, None), sine1k=("fixed", 4, None), fullnoise=("verbatim", 0, 0), alternating=("verbatim", 0, 0),
                switch2048=("fixed", None, 1), switch1024=("fixed", None, 2), switch512=("fixed", None, 3), switch256=("fixed", None, 4))
    seen_o, seen_po, seen_k, kinds = set(), set(), set(), set()
    for name, x in signals().items():
        kind, o, po, ks, _bits = ap.flac_choose(x)
        exp = want[name]
        assert kind == exp[0] and (exp[1] is None or o == exp[1]) and (exp[2] is None or po == exp[2]), (name, kind, o, po)
        kinds.add(kind)
        if kind == "fixed":
            seen_o.add(o)
            seen_po.add(po)
            seen_k.update(ks)
    assert kinds == {"constant", "verbatim", "fixed"} and seen_o == {0, 1, 2, 3, 4} and seen_po >= {0, 1, 2, 3, 4}
    assert 0 in seen_k and 14 in seen_k
    assert ap.flac_choose(signals()["ramp"])[3] == [0]
    ks = ap.flac_choose(signals()["switch2048"])[3]
    assert min(ks) <= 1 and max(ks) == 14
    # the short last frames carry every count of trailing zero bits
    pads = {(-ap.flac_choose(x[-(n % BLOCK or BLOCK):])[4]) % 8 for (name, n), (x, *_r) in encoded.items()}
    assert pads == set(range(8))


def test_a_one_second_clip_encodes_quickly():
    ap, x = _ap(), speechlike(SR)
    t0 = time.perf_counter()
    data = ap.encode_output(x, "flac", SR)
    took = time.perf_counter() - t0
    assert took < 0.5, took
    assert np.array_equal(decode_stream(data)[0], x) and data.size < 0.7 * x.nbytes      # speech-like: well under the PCM's size


# ------------------------------------------------------------------ minimality
def test_frame_size_is_the_brute_force_minimum():
    ap = _ap()
    rng = np.random.default_rng(15)
    for case in range(200):
        m = int(rng.integers(16, 65))
        scale = int(rng.choice([1, 3, 40, 700, 9000, 32767]))
        shape = case % 4
        x = rng.integers(-scale, scale + 1, m)
        if shape == 1:
            x = np.cumsum(x)
        elif shape == 2:
            x = np.cumsum(np.cumsum(rng.integers(-2, 3, m))) * max(scale // 64, 1)
        elif shape == 3:
            x = np.where(np.arange(m) < m // 2, x // max(scale // 2, 1), x)
        x = np.clip(x, -32768, 32767).astype(np.int16)
        want = best_subframe(x)
        got = ap.flac_choose(x)
        assert got == want, (case, m, got, want)
        frame = ap.flac_encode_frame(x, SR, case)
        hdr = 4 + (1 if case < 128 else 2) + 2 + 1
        assert len(frame) == hdr + -(-want[4] // 8) + 2, case


def test_tie_rule_lower_order_then_lower_partition_order_then_lower_k():
    ap = _ap()
    # k, by hand: residuals +1 (u = 2: 3 bits under k = 0, 1 and 2) and -1 (u = 1: 2 bits under k = 0 and 1, 3 under k = 2) tie k = 0 with k = 1
    y = np.tile(np.array([1, -1], np.int16), 16)
    per_k = [fixed_bits(list(y), 0, 0, [k])[0] for k in range(15)]
    assert per_k[0] == per_k[1] == min(per_k) < per_k[2]
    assert ap.flac_choose(y) == best_subframe(y) == ("fixed", 0, 0, [0], per_k[0])
    y = np.tile(np.array([1, 1, 1, -1], np.int16), 8)                  # u = 2, 2, 2, 1: 11 bits per four under k = 0 and under k = 1
    per_k = [fixed_bits(list(y), 0, 0, [k])[0] for k in range(15)]
    assert per_k[0] == per_k[1] == min(per_k)
    assert ap.flac_choose(y)[:4] == ("fixed", 0, 0, [0])
    # order and partition order, by hand: frames where several (o, po) give exactly the same size keep the lowest o, then the lowest po
    hand = (([1, 0, 0, 1, 0, -1, -1, 0, 0, -1, -2, -2, -2, -2, -2, -3], [(0, 0), (0, 1), (1, 0)]),
            ([-1, -1, -2, -2, -1, -1, -2, -4, -6, -9, -12, -15, -17, -20, -22, -25], [(1, 0), (2, 0)]),
            ([1, 1, 1, 2, 2, 1, 0, 0, 0, -1, -3, -5, -7, -9, -11, -14], [(1, 0), (1, 1)]))
    for y, tied in hand:
        cands = {(o, po): fixed_bits(y, o, po) for o in range(5) for po in range(5)}
        low = min(v[0] for v in cands.values() if v is not None)
        assert sorted(key for key, v in cands.items() if v is not None and v[0] == low) == tied
        assert ap.flac_choose(np.array(y, np.int16))[:3] == ("fixed",) + tied[0]
    # and over a seeded family of small walks and two-level signals, which holds many ties of both kinds
    ties_o = ties_po = 0
    rng = np.random.default_rng(3)
    for case in range(300):
        m = int(rng.choice([16, 32]))
        y = (np.cumsum(rng.integers(-1, 2, m)) if case % 2 else rng.integers(0, 2, m) * rng.integers(1, 4)).astype(np.int16)
        if (y == y[0]).all():
            continue
        cands = {(o, po): fixed_bits(list(y), o, po) for o in range(5) for po in range(5)}
        cands = {key: v[0] for key, v in cands.items() if v is not None}
        low = min(cands.values())
        winners = sorted(key for key, v in cands.items() if v == low)
        kind, o, po, _ks, bits = ap.flac_choose(y)
        if low <= 8 + 16 * m:
            assert (kind, o, po, bits) == ("fixed",) + winners[0] + (low,), (y, winners)
            ties_o += len({w[0] for w in winners}) > 1
            ties_po += len([w for w in winners if w[0] == winners[0][0]]) > 1
    assert ties_o >= 3 and ties_po >= 3                                # the family does contain both kinds of tie
    # verbatim only when STRICTLY smaller: frames whose best Fixed size equals 8 + 16 m stay Fixed
    for y in VERBATIM_TIES:
        m = len(y)
        best = min(v[0] for v in (fixed_bits(y, o, po) for o in range(5) for po in range(5)) if v is not None)
        assert best == 8 + 16 * m == fixed_bits(y, 0, 0)[0]
        got = ap.flac_choose(np.array(y, np.int16))
        assert got[:3] == ("fixed", 0, 0) and got[4] == best and got == best_subframe(y)
        frame = ap.flac_encode_frame(np.array(y, np.int16), SR, 0)
        samples, what, _n = decode_frames(frame, SR, 0)
        assert samples.tolist() == y and what[0][0] == "fixed"
    longer = VERBATIM_TIES[0][:-1] + [-32768]                          # one more bit for Fixed: now verbatim is strictly smaller
    assert min(v[0] for v in (fixed_bits(longer, o, po) for o in range(5) for po in range(5)) if v is not None) > 8 + 16 * 16
    assert ap.flac_choose(np.array(longer, np.int16))[0] == "verbatim"


# ------------------------------------------------------------------ frame numbers, rates, batches
@pytest.mark.parametrize("frame0", [0, 127, 128, 2047, 2048, 65535, 65536, (1 << 31) - 2])
def test_frame_numbers_decode(frame0):
    ap = _ap()
    x = speechlike(BLOCK + 10, 3)
    frames, lo, hi = ap.flac_encode_frames(x, SR, frame0)
    samples, what, numbers = decode_frames(frames, SR, frame0)
    assert numbers == [frame0, frame0 + 1] and np.array_equal(samples, x) and (lo, hi) == (min(w[4] for w in what), max(w[4] for w in what))
    coded = 1 if frame0 < 128 else 2 if frame0 < 2048 else 3 if frame0 < 65536 else 4 if frame0 < 1 << 21 else 6
    one = ap.flac_encode_frame(x[:BLOCK], SR, frame0)
    assert len(one) - len(ap.flac_encode_frame(x[:BLOCK], SR, 0)) == coded - 1


def test_frame_number_and_block_limits():
    ap = _ap()
    x = np.zeros(BLOCK + 1, np.int16)
    ap.flac_encode_frames(x, SR, (1 << 31) - 2)
    for bad in (dict(frame0=(1 << 31) - 1), dict(frame0=-1), dict(last=False)):
        with pytest.raises(ValueError):
            ap.flac_encode_frames(x, SR, **bad)
    with pytest.raises(ValueError):
        ap.flac_encode_frames(x.astype(np.int32), SR)
    assert ap.flac_encode_frames(np.zeros(0, np.int16), SR) [1:] == (0, 0)
    assert [ap.flac_frame_bound(m) for m in (0, 1, 4096)] == [0, 20, 8210]


@pytest.mark.parametrize("rate,code,extra", [(8000, 4, b""), (24000, 7, b""), (11025, 13, (11025).to_bytes(2, "big")), (65535, 13, b"\xff\xff"),
                                             (65540, 14, (6554).to_bytes(2, "big")), (192000, 3, b""), (65541, 0, b"")])
def test_rate_codes(rate, code, extra):
    ap = _ap()
    x = speechlike(300, 4)
    frame = ap.flac_encode_frame(x, rate, 5)
    assert frame[2] == (7 << 4) | code                                 # a short frame: block-size code 0111, then the rate code
    assert frame[4] == 5 and frame[5:7] == (299).to_bytes(2, "big") and frame[7: 7 + len(extra)] == extra
    data = ap.encode_output(x, "flac", rate)
    samples, _frames, info = decode_stream(data)
    assert info["rate"] == rate and np.array_equal(samples, x)
    for bad in (0, 655351, 24000.5, True):
        with pytest.raises(ValueError):
            ap.flac_encode_frames(x, bad)


def test_a_request_alone_equals_itself_in_a_batch():
    ap = _ap()
    cases = device_cases()
    whole, info, bound = mirror_layout(cases, SR)
    assert info[-1, 0] == whole.size <= bound
    for j, (name, x, frame0, last) in enumerate(cases):
        alone = ap.flac_encode_frames(x, SR, frame0, bool(last))[0]
        assert np.array_equal(whole[info[j, 0]: info[j + 1, 0]], alone), name
        samples, _w, _n = decode_frames(alone, SR, frame0)
        assert np.array_equal(samples, x), name


def test_stream_header_fields():
    ap = _ap()
    h = ap.flac_stream_header(SR, 123456, 17, 8210)
    assert len(h) == 42 and h[:4] == b"fLaC" and h[4] == 0x80 and h[5:8] == b"\0\0\x22"
    info, at = stream_header(h)
    assert at == 42 and info == dict(min_block=4096, max_block=4096, min_frame=17, max_frame=8210, rate=SR, channels=1, bits=16, total=123456, md5=bytes(16))
    assert stream_header(ap.flac_stream_header(655350, 0))[0]["rate"] == 655350
    assert ap.encode_output(np.zeros(0, np.int16), "flac", SR).tobytes() == ap.flac_stream_header(SR, 0)
    for bad in (dict(total_samples=1 << 36), dict(total_samples=-1), dict(total_samples=0, min_frame=1 << 24)):
        with pytest.raises(ValueError):
            ap.flac_stream_header(SR, **bad)


# ------------------------------------------------------------------ FlacStream
@pytest.mark.parametrize("order", [(1, 4095, 4096, 4097, 10000), (10000, 4097, 4096, 4095, 1), (4096, 1, 10000, 4095, 4097), (4097, 4096, 1, 1, 4095),
                                   (4096, 4096), (1,)])
def test_flac_stream_blocks_add_up(order):
    ap = _ap()
    x = speechlike(sum(order), 11)
    fs, out, at = ap.FlacStream(SR), [], 0
    for k, n in enumerate(order):
        out.append(fs.push(x[at: at + n]))
        at += n
        if k == 0:
            assert out[0][:42].tobytes() == ap.flac_stream_header(SR, 0)
    out.append(fs.flush())
    data = np.concatenate(out)
    samples, frames, info = decode_stream(data)
    assert np.array_equal(samples, x) and info["total"] == 0 and info["min_frame"] == 0
    assert np.array_equal(data[42:], ap.flac_encode_frames(x, SR)[0])            # its frames equal those of the one-shot encoding
    assert fs.flush().size == 0 and fs.frame == len(frames)


def test_flac_stream_backend_sees_whole_blocks_only():
    ap, calls = _ap(), []

    def backend(pcm, frame0, last):
        calls.append((pcm.size, frame0, last))
        return ap.flac_encode_frames(pcm, 8000, frame0, last)[0]
    fs = ap.FlacStream(8000, backend)
    x = speechlike(3 * BLOCK + 7, 2, 8000)
    data = np.concatenate([fs.push(x[:5000]), fs.push(x[5000:5001]), fs.push(x[5001:]), fs.flush()])
    assert calls == [(BLOCK, 0, False), (2 * BLOCK, 1, False), (7, 3, True)]
    assert np.array_equal(decode_stream(data)[0], x)
    assert ap.FlacStream(8000).flush().tobytes() == ap.flac_stream_header(8000, 0)          # an empty stream is its header
    with pytest.raises(ValueError):
        ap.OutputStream(SR, 8000, "flac")


# ------------------------------------------------------------------ config, files, engine on oracle sessions
def test_model_config_accepts_flac_and_still_refuses_mp3():
    from vietvoice_tts_amd.core import ModelConfig
    base = dict(model_cache_dir="/tmp/x", synthetic_model=True, model_spec="tiny")
    c = ModelConfig(output_encoding="flac", **base)
    assert c.output_encoding == "flac" and ModelConfig.from_dict(c.to_dict()).output_encoding == "flac"
    with pytest.raises(ValueError, match="flac"):
        ModelConfig(output_encoding="mp3", **base)


def test_save_audio_and_to_wav_bytes_pass_flac_through(tmp_path):
    ap = _ap()
    x = speechlike(5000, 8)
    data = ap.encode_output(x, "flac", 16000)
    assert ap.AudioProcessor.to_wav_bytes(data, 16000, "flac") == data.tobytes()
    p = tmp_path / "sub" / "x.flac"
    ap.AudioProcessor.save_audio(data, str(p), 16000, "flac")
    assert p.read_bytes() == data.tobytes() and np.array_equal(decode_stream(p.read_bytes())[0], x)
    for bad in (x, data[4:], data.astype(np.int16), data[:20]):
        with pytest.raises(ValueError):
            ap.AudioProcessor.save_audio(bad, str(p), 16000, "flac")
        with pytest.raises(ValueError):
            ap.AudioProcessor.to_wav_bytes(bad, 16000, "flac")


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


def test_engine_on_oracle_sessions_writes_and_streams_flac(cpu_engine, tmp_path):
    from vietvoice_tts_amd.core.audio_processor import limit_peaks, resample_output
    eng, cfg = cpu_engine, cpu_engine.config
    _reseed(eng)
    base, _ = eng.synthesize(TEXT)
    assert len(eng._last_plan) > 1 and base.dtype == np.int16 and base.size > 2 * BLOCK
    try:
        cfg.output_encoding = "flac"
        assert not eng._device_output()                      # injected sessions: the host mirror
        _reseed(eng)
        path = tmp_path / "x.flac"
        got, _ = eng.synthesize(TEXT, output_path=str(path))
        samples, frames, info = decode_stream(got)
        assert got.dtype == np.uint8 and path.read_bytes() == got.tobytes()
        assert np.array_equal(samples, base) and info["rate"] == SR and info["total"] == base.size and info["max_frame"] == max(f[4] for f in frames)
        _reseed(eng)
        blocks = list(eng.synthesize_stream(TEXT))
        assert len(blocks) > 1 and all(b.dtype == np.uint8 for b in blocks)
        streamed, _f, sinfo = decode_stream(np.concatenate(blocks))
        assert np.array_equal(streamed, base) and sinfo["total"] == 0
        assert np.array_equal(np.concatenate(blocks)[42:], got[42:])             # the same frames, byte for byte
        # the place in the chain: join -> limiter -> rate -> FLAC
        cfg.output_limiter, cfg.output_sample_rate = "true", 8000
        want = resample_output(limit_peaks(base, SR, cfg.output_peak_dbfs, "true")[0], SR, 8000)
        _reseed(eng)
        chain, _ = eng.synthesize(TEXT)
        samples, _f, info = decode_stream(chain)
        assert info["rate"] == 8000 and np.array_equal(samples, want)
        _reseed(eng)
        streamed = decode_stream(np.concatenate(list(eng.synthesize_stream(TEXT))))[0]
        assert np.array_equal(streamed, want)
    finally:
        cfg.output_encoding, cfg.output_limiter, cfg.output_sample_rate = "pcm16", None, None


# ------------------------------------------------------------------ ABI
def test_header_version_script_and_exports_agree():
    from vietvoice_tts_amd import build_ext, runtime
    ap = _ap()
    hdr = open(os.path.join(ROOT, "include", "vvtts.h")).read()
    declared = set(re.findall(r"VV_API\s+[\w\s\*]+?\b(vv_\w+)\s*\(", hdr))
    assert declared == set(runtime.EXPORTS), declared ^ set(runtime.EXPORTS)
    ver = open(os.path.join(ROOT, "vietvoice-tts_amd", "csrc", "vvtts.map")).read()
    globs = [g.strip() for g in re.findall(r"global:\s*([^;]+);", ver)]
    lib = runtime.load_library()
    for name, n_args in (("vv_pcm_flac", 13), ("vv_pcm_flac_ws_bytes", 2), ("vv_flac_frame_bound", 1)):
        assert name in declared and len(runtime.EXPORTS[name][1]) == n_args
        assert any(re.fullmatch(g.replace("*", ".*"), name) for g in globs) and hasattr(lib, name)
    args = [None if t is ctypes.c_void_p else 0 for t in runtime.EXPORTS["vv_pcm_flac"][1]]
    assert lib.vv_pcm_flac(*args) == -22                                              # no context: refused before anything else
    buf = (ctypes.c_int64 * 64)()
    good = [None, ctypes.addressof(buf), 64, ctypes.addressof(buf), ctypes.addressof(buf), 1, SR, ctypes.addressof(buf), 512, ctypes.addressof(buf),
            ctypes.addressof(buf), 512, None]
    assert lib.vv_pcm_flac(*good) == -22                                              # every refusal is -22 without a context, whatever the rest
    assert [lib.vv_flac_frame_bound(m) for m in (-1, 0, 1, 17, 4096, 4097)] == [0, 0, 20, 52, 8210, 0]
    assert all(lib.vv_flac_frame_bound(m) == ap.flac_frame_bound(m) <= 16 + 1 + 2 * m + 2 for m in (1, 2, 100, 4095, 4096))
    assert lib.vv_pcm_flac_ws_bytes(66, 33) >= 8 * 34 + 66 * 24 and lib.vv_pcm_flac_ws_bytes(0, 0) > 0
    assert "vv_flac" in build_ext.SOURCES
    assert int(re.search(r"#define VV_FLAC_BLOCK (\d+)", hdr).group(1)) == ap.FLAC_BLOCK
    assert re.search(r"#define\s+VV_PROF_NCLASS\s+18\b", hdr)
    m = re.match(rb"vvtts-hip (\d+)\.(\d+) ", lib.vv_version())
    assert m and (int(m.group(1)), int(m.group(2))) >= (0, 8)                         # bumped with the additive entries
    src = open(os.path.join(ROOT, "vietvoice-tts_amd", "csrc", "vv_flac.hip")).read()
    kernels = src[src.index("namespace {"): src.index("}  // namespace")]
    assert not re.search(r"\b(float|double)\b", kernels)                              # integer arithmetic throughout
