"""-m gpu: FLAC input on the device (csrc/vv_flac_decode.hip) against the Python mirror -- byte for byte over the case list
of tests/flac_decode_util.py (a writer that shares nothing with the product), a clip alone against the clip in the batch, the product's
own encoder fed back, voice-bank entries from FLAC against the WAV of the same PCM, the engine and the batching front end with a FLAC
voice, and the refusals with the mirror's reason code and byte."""
import numpy as np
import pytest
import torch

from tests import flac_decode_util as U
from tests.flac_util import signals, speechlike

pytestmark = pytest.mark.gpu

TEXT = "Xin chào các bạn, hôm nay thế nào?"
REF_TEXT = "xin chào"


def _ap():
    from vietvoice_tts_amd.core import audio_processor
    return audio_processor


@pytest.fixture(scope="module")
def eng(hip_tiny):
    return hip_tiny["f32"]


def _clips(eng, files):
    """[(frames (n, channels), width, rate) | FlacError] of one flac_clips call."""
    pcm, res = eng.flac_clips(files)
    host, out = pcm.cpu().numpy(), []
    for r in res:
        if isinstance(r, Exception):
            out.append(r)
            continue
        off, n, width, rate, ch = r
        out.append((host[off: off + n * ch * width].view({1: np.int8, 2: np.int16, 4: np.int32}[width]).reshape(n, ch).copy(), width, rate))
    return out


@pytest.fixture(scope="module")
def batch(eng):
    """Every case of the list in ONE call, shuffled: {name: (frames, width, rate)}."""
    cases = U.cases()
    order = np.random.default_rng(17).permutation(len(cases))
    got = _clips(eng, [cases[i][1] for i in order])
    return {cases[i][0]: g for i, g in zip(order, got)}


def test_device_equals_mirror_over_the_case_list_in_one_batch(batch):
    ap = _ap()
    for name, data, x, bits, rate in U.cases():
        got = batch[name]
        assert not isinstance(got, Exception), (name, got)
        want = ap.flac_decode(data)
        assert got[0].dtype == want[0].dtype and got[0].shape == want[0].shape and got[0].tobytes() == want[0].tobytes(), name
        assert got[1:] == want[1:] == ({8: 1, 16: 2, 24: 4}[bits], rate), name
        assert np.array_equal(got[0], U.layout(x, bits)), name                 # and both equal the writer's input


def test_a_clip_alone_equals_the_clip_in_the_batch(eng, batch):
    for name, data, _x, _bits, _rate in U.cases():
        (alone,) = _clips(eng, [data])
        assert alone[0].dtype == batch[name][0].dtype and alone[0].tobytes() == batch[name][0].tobytes() and alone[1:] == batch[name][1:], name


@pytest.mark.parametrize("lpc_order", [0, 12])
def test_the_device_encoder_fed_into_the_device_decoder_gives_its_input(eng, lpc_order):
    ap = _ap()
    items = [speechlike(3 * 4096 + 1000), *list(signals(4096).values())[:6], np.array([5], np.int16)]
    x = torch.from_numpy(np.concatenate(items)).to(eng.device)
    offs = np.concatenate([[0], np.cumsum([len(i) for i in items])])
    y, info = eng.pcm_flac(x, [[int(offs[j]), len(items[j]), 0, 1] for j in range(len(items))], 24000, lpc_order)
    info, y = info.cpu().numpy(), y.cpu().numpy()
    files = []
    for j, it in enumerate(items):
        end = int(info[j + 1, 0]) if j + 1 < len(items) else int(info[len(items), 0])
        files.append(ap.flac_stream_header(24000, len(it), int(info[j, 1]), int(info[j, 2])) + y[int(info[j, 0]): end].tobytes())
    for it, got in zip(items, _clips(eng, files)):
        assert not isinstance(got, Exception) and got[1:] == (2, 24000) and np.array_equal(got[0][:, 0], it)


def _bank(eng, **kw):
    from vietvoice_tts_amd.voice_bank import VoiceBank
    return VoiceBank(eng, 24000, **kw)


def _pair(rate, nch, n=5000, seed=0):
    x = U._tone(n, nch, 16, np.random.default_rng(rate + nch + seed))
    flac = U.simple_stream(x, rate=rate, block=1152, assign=10 if nch == 2 else None, subs=lambda f, c, s: dict(kind="fixed", order=2, method=1))
    return flac, U.wav_bytes(x, 16, rate)


def test_voice_bank_entries_from_flac_equal_entries_from_wav(eng, tmp_path):
    ap = _ap()
    pairs = [_pair(rate, nch) for rate in (16000, 24000, 44100) for nch in (1, 2)]
    pairs.append((U.simple_stream(U._tone(900, 3, 24, np.random.default_rng(3)), bits=24, rate=48000, block=256),
                  U.wav_bytes(U._tone(900, 3, 24, np.random.default_rng(3)), 24, 48000)))
    from_wav = _bank(eng).ingest_many([w for _f, w in pairs])
    from_flac = _bank(eng).ingest_many([f for f, _w in pairs])
    for (f, w), a, b in zip(pairs, from_flac, from_wav):
        assert a.pcm_host.dtype == np.int16 and np.array_equal(a.pcm_host, b.pcm_host)
        assert np.array_equal(a.pcm_dev.cpu().numpy(), b.pcm_dev.cpu().numpy()) and np.array_equal(a.pcm_host, ap.AudioProcessor.load_audio(w, 24000))
    # FLAC and WAV mixed in one ingest_many, a path among them; a second request is a cache hit
    p = tmp_path / "voice.flac"
    p.write_bytes(pairs[5][0])
    bank = _bank(eng)
    mixed = bank.ingest_many([pairs[0][1], pairs[1][0], str(p), pairs[2][1], pairs[3][0]])
    for e, j in zip(mixed, (0, 1, 5, 2, 3)):
        assert np.array_equal(e.pcm_host, from_wav[j].pcm_host) and np.array_equal(e.pcm_dev.cpu().numpy(), from_wav[j].pcm_host)
    hits, misses = bank.hits, bank.misses
    again = bank.ingest_many([pairs[1][0], str(p)])
    assert (bank.hits, bank.misses) == (hits + 2, misses) and again[0] is mixed[1] and again[1] is mixed[2]
    poly = _bank(eng, resampler="polyphase")
    assert np.array_equal(poly.get(pairs[4][0]).pcm_host, poly.get(pairs[4][1]).pcm_host)       # the opt-in path: frames copied back


@pytest.fixture(scope="module")
def tiny(tmp_path_factory):
    from vietvoice_tts_amd.core import ModelConfig, TTSEngine
    e = TTSEngine(ModelConfig(model_cache_dir=str(tmp_path_factory.mktemp("flac_in_models")), synthetic_model=True, nfe_step=5, acoustic_dtype="fp32",
                              max_chunk_duration=8.0, model_spec="tiny", noise_source="device", output_stage="device"))
    yield e
    e.cleanup()


def _say(e, **kw):
    """One call from call serial 0 (the same start noise every time); a user clip excludes the config's voice filters."""
    c = e.config
    saved = (c.gender, c.group, c.area, c.emotion)
    if kw:
        c.gender = c.group = c.area = c.emotion = None
    e.model_session_manager.noise_serial = 0
    try:
        return e.synthesize(TEXT, **kw)[0]
    finally:
        c.gender, c.group, c.area, c.emotion = saved


def test_engine_with_a_flac_reference_equals_the_wav_reference(tiny, tmp_path):
    e = tiny
    x = (speechlike(24000 * 2).astype(np.int64) // 2).reshape(-1, 1)
    (tmp_path / "ref.flac").write_bytes(U.simple_stream(x, rate=24000, block=4096, subs=lambda f, c, s: dict(kind="fixed", order=2, method=1)))
    (tmp_path / "ref.wav").write_bytes(U.wav_bytes(x, 16, 24000))
    a = _say(e, reference_audio=str(tmp_path / "ref.flac"), reference_text=REF_TEXT)
    b = _say(e, reference_audio=str(tmp_path / "ref.wav"), reference_text=REF_TEXT)
    assert a.dtype == np.int16 and a.size > 0 and np.array_equal(a, b)
    assert e.validate_configuration(str(tmp_path / "ref.flac")) == e.validate_configuration(str(tmp_path / "ref.wav")) is True
    # the engine's own FLAC output (LPC 8) fed back as the voice == its PCM fed back as WAV
    e.config.output_encoding, e.config.flac_lpc_order = "flac", 8
    try:
        made = _say(e)
    finally:
        e.config.output_encoding, e.config.flac_lpc_order = "pcm16", 0
    pcm = _say(e)
    assert made.dtype == np.uint8 and np.array_equal(_ap().flac_decode(made.tobytes())[0][:, 0], pcm)
    (tmp_path / "own.flac").write_bytes(made.tobytes())
    (tmp_path / "own.wav").write_bytes(U.wav_bytes(pcm.reshape(-1, 1), 16, e.config.sample_rate))
    a = _say(e, reference_audio=str(tmp_path / "own.flac"), reference_text=TEXT)
    b = _say(e, reference_audio=str(tmp_path / "own.wav"), reference_text=TEXT)
    assert a.size > 0 and np.array_equal(a, b)


def test_batching_frontend_flac_voice_alone_equals_inside_a_mixed_batch(tmp_path):
    from vietvoice_tts_amd.batching import BatchingFrontend
    from vietvoice_tts_amd.core import ModelConfig, TTSEngine
    tiny = TTSEngine(ModelConfig(model_cache_dir=str(tmp_path), synthetic_model=True, model_spec="tiny", nfe_step=5, acoustic_dtype="fp32",
                                 max_chunk_duration=8.0))
    c = tiny.config
    c.gender = c.group = c.area = c.emotion = None                          # a user clip excludes the config's voice filters
    x = (speechlike(24000 * 2, seed=9).astype(np.int64) // 2).reshape(-1, 1)
    (tmp_path / "v.flac").write_bytes(U.simple_stream(x, rate=24000, block=4096, subs=lambda f, c, s: dict(kind="fixed", order=1)))
    (tmp_path / "v.wav").write_bytes(U.wav_bytes(x[::-1], 16, 24000))
    voice = dict(reference_audio=str(tmp_path / "v.flac"), reference_text=REF_TEXT)
    fe = BatchingFrontend(tiny, max_wait_ms=300.0, max_requests=8)
    try:
        alone = fe.submit(TEXT, speed=1.0, serial=7, **voice).result(timeout=300)[0]
        n0 = fe.batches_run
        futs = [fe.submit("Tạm biệt và hẹn gặp lại.", speed=1.3, serial=8, gender="male"), fe.submit(TEXT, speed=1.0, serial=7, **voice),
                fe.submit("Hẹn gặp lại các bạn.", speed=0.9, serial=9, reference_audio=str(tmp_path / "v.wav"), reference_text=REF_TEXT)]
        outs = [f.result(timeout=300)[0] for f in futs]
        assert fe.batches_run == n0 + 1
        assert outs[1].shape == alone.shape and int(np.abs(outs[1].astype(np.int32) - alone.astype(np.int32)).max()) <= 2
        assert all(o.dtype == np.int16 and o.size > 0 for o in outs)
    finally:
        fe.close()
        tiny.cleanup()


# one stream per reason class; every one of them went through the kernels on the CPU under address and undefined-behaviour sanitizers first
# (tools/flac_decode_host_check.py runs the whole of flac_decode_util.malformed(); tests/test_flac_decode_cpu.py repeats that)
REFUSALS = ("header_bit", "crc16_bit", "cut_last_frame", "reserved_subframe_type", "partition_misfit", "sample_out_of_range")


def test_refusals_give_the_mirrors_reason_and_byte_and_a_valid_clip_beside_them_still_decodes(eng):
    ap = _ap()
    bad = {m[0]: m for m in U.malformed()}
    good = next(c for c in U.cases() if c[0] == "stereo_10")
    got = _clips(eng, [bad[n][1] for n in REFUSALS[:3]] + [good[1]] + [bad[n][1] for n in REFUSALS[3:]])
    assert not isinstance(got[3], Exception) and np.array_equal(got[3][0], U.layout(good[2], good[3]))
    for name, g in zip(REFUSALS, got[:3] + got[4:]):
        _n, data, code, position = bad[name]
        with pytest.raises(ap.FlacError) as e:
            ap.flac_decode(data)
        assert isinstance(g, ap.FlacError) and (g.code, g.position) == (e.value.code, e.value.position) == (code, position), name
        assert str(g) == str(e.value)
    with pytest.raises(ValueError, match="malformed FLAC: header CRC-8 mismatch"):
        _bank(eng).ingest_many([good[1], bad["header_bit"][1]])


def test_refusals_of_the_c_entries_launch_nothing_and_leave_the_context_usable(eng):
    lib, ctx, st = eng.lib, eng.ctx, eng._stream()
    data = torch.zeros(64, dtype=torch.uint8, device=eng.device)
    rows_h = torch.tensor([[0, 40, 1, 16, 16, 4096, 24000, 0]], dtype=torch.int64)
    rows_d = rows_h.to(eng.device)
    info = torch.full((1, 4), -7, dtype=torch.int64, device=eng.device)
    need = int(lib.vv_flac_index_ws_bytes(64, 1))
    ws = torch.zeros(need // 8 + 1, dtype=torch.int64, device=eng.device)

    def index(**kw):
        a = dict(data=data.data_ptr(), n=64, rows=rows_d.data_ptr(), rows_h=rows_h.data_ptr(), R=1, info=info.data_ptr(), ws=ws.data_ptr(), ws_bytes=ws.numel() * 8)
        a.update(kw)
        return lib.vv_flac_index(ctx, a["data"], a["n"], a["rows"], a["rows_h"], a["R"], a["info"], a["ws"], a["ws_bytes"], st)
    no_pad = torch.tensor([[0, 60, 1, 16, 16, 4096, 24000, 0]], dtype=torch.int64)
    bad_bits = torch.tensor([[0, 40, 1, 20, 16, 4096, 24000, 0]], dtype=torch.int64)
    odd_off = torch.tensor([[2, 40, 1, 16, 16, 4096, 24000, 0]], dtype=torch.int64)
    for kw in (dict(data=None), dict(rows=None), dict(rows_h=None), dict(info=None), dict(ws=None), dict(data=data.data_ptr() + 1), dict(info=info.data_ptr() + 4),
               dict(R=0), dict(R=65536), dict(n=4), dict(ws_bytes=need - 8), dict(rows_h=no_pad.data_ptr()), dict(rows_h=bad_bits.data_ptr()),
               dict(rows_h=odd_off.data_ptr()), dict(info=ws.data_ptr()), dict(ws=data.data_ptr(), ws_bytes=64)):
        assert index(**kw) == -22, kw
    torch.cuda.synchronize()
    assert bool((info == -7).all()) and bool((ws == 0).all())                  # nothing was launched
    assert index() == 0
    assert info.cpu().tolist() == [[1, 0, 0, 0]]                               # zeros are no frame: bad header at the clip's first byte
    lay_h = torch.tensor([[0, 0, 0, 0, 0, 0]], dtype=torch.int64)
    lay_d = lay_h.to(eng.device)
    pcm = torch.full((16,), 0x55, dtype=torch.uint8, device=eng.device)
    info2 = torch.full((1, 2), -7, dtype=torch.int64, device=eng.device)
    ws2 = torch.zeros(4, dtype=torch.int64, device=eng.device)

    def decode(**kw):
        a = dict(data=data.data_ptr(), lay=lay_d.data_ptr(), lay_h=lay_h.data_ptr(), ws=ws.data_ptr(), ws_bytes=ws.numel() * 8, pcm=pcm.data_ptr(), n_pcm=16,
                 info2=info2.data_ptr(), ws2=ws2.data_ptr(), ws2_bytes=32)
        a.update(kw)
        return lib.vv_flac_decode(ctx, a["data"], 64, rows_d.data_ptr(), rows_h.data_ptr(), 1, a["lay"], a["lay_h"], a["ws"], a["ws_bytes"], a["pcm"], a["n_pcm"],
                                  a["info2"], a["ws2"], a["ws2_bytes"], st)
    too_big = torch.tensor([[0, 1, 16, 0, 0, 0]], dtype=torch.int64)             # 32 bytes of PCM into 16
    bad_sums = torch.tensor([[0, 0, 0, 1, 0, 0]], dtype=torch.int64)
    for kw in (dict(data=None), dict(lay=None), dict(lay_h=None), dict(pcm=None), dict(info2=None), dict(ws2=None), dict(ws_bytes=need - 8), dict(ws2_bytes=0),
               dict(lay_h=too_big.data_ptr()), dict(lay_h=bad_sums.data_ptr()), dict(info2=info2.data_ptr() + 4), dict(pcm=data.data_ptr(), n_pcm=64),
               dict(ws2=ws.data_ptr(), ws2_bytes=32)):
        assert decode(**kw) == -22, kw
    torch.cuda.synchronize()
    assert bool((info2 == -7).all()) and bool((pcm == 0x55).all())
    assert decode() == 0 and bool((pcm.cpu() == 0x55).all())                     # a refused clip: nothing of it is written
    good = next(c for c in U.cases() if c[0] == "channels_3")
    (got,) = _clips(eng, [good[1]])
    assert np.array_equal(got[0], U.layout(good[2], good[3]))                   # and the context still decodes
