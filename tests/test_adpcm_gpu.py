"""-m gpu: IMA ADPCM output and ADPCM / G.711 input on the device (csrc/vv_adpcm.hip) against the Python mirror -- byte for
byte over the encoder list of tests/adpcm_util.py as one ragged batch, a request alone against itself in the batch, a canary around the
rows; sample for sample over the decoder files in one call, a bad step index with the mirror's reason and byte, voice-bank entries from
coded clips against the PCM16 WAV of the mirror-decoded samples; and the engine writing, streaming and reading back its own files.  On the
commit before N25 every test here fails with ``output_encoding must be one of ...``, ``unsupported WAVE format tag ...`` or a missing entry."""
import struct

import numpy as np
import pytest
import torch

from tests import adpcm_util as U
from tests.flac_util import speechlike

pytestmark = pytest.mark.gpu

TEXT = "Xin chào các bạn, hôm nay thế nào?"
CANARY = 0xA5


def _ap():
    from vietvoice_tts_amd.core import audio_processor
    return audio_processor


@pytest.fixture(scope="module")
def eng(hip_tiny):
    return hip_tiny["f32"]


# ------------------------------------------------------------------ encoder
def _batch(spb):
    """The CPU list packed as R = 5 ragged requests: the lengths of the issue's list joined pairwise, then silence, square and ramp."""
    items = dict(U.encoder_inputs(spb))
    speech = [items[f"speech_{n}"] for n in U.lengths(spb)]
    return [np.concatenate(speech[:3]), np.concatenate(speech[3:5]), np.concatenate(speech[5:]), np.concatenate([items["silence"], items["square"]]),
            items["ramp"]] + speech


@pytest.fixture(scope="module")
def mirror():
    ap = _ap()
    return {spb: [ap.adpcm_encode_blocks(s, spb) for s in _batch(spb)] for spb in U.SPBS}


def _encode(eng, sigs, spb, order=None, gap=8):
    """One pcm_adpcm call over ``sigs`` (rows in ``order``), y pre-filled with a canary -> (y on the host, [(offset, bytes)] per signal)."""
    ba = (spb - 1) // 2 + 4
    order = list(range(len(sigs))) if order is None else order
    src, pos = {}, 3
    for j in range(len(sigs)):
        src[j] = pos
        pos += len(sigs[j]) + 5
    x = np.full(pos, 12345, np.int16)
    for j, s in enumerate(sigs):
        x[src[j]: src[j] + len(s)] = s
    rows, at, spans = [], gap, {}
    for j in order:
        nb = -(-len(sigs[j]) // spb)
        rows.append([src[j], len(sigs[j]), at])
        spans[j] = (at, nb * ba)
        at += nb * ba + gap
    y = torch.full((at,), CANARY, dtype=torch.uint8, device=eng.device)
    eng.pcm_adpcm(torch.from_numpy(x).to(eng.device), rows, spb, out=y)
    return y.cpu().numpy(), [spans[j] for j in range(len(sigs))]


@pytest.mark.parametrize("spb", U.SPBS)
def test_device_equals_mirror_byte_for_byte_in_ragged_batches_and_leaves_the_rest_alone(eng, mirror, spb):
    sigs = _batch(spb)
    for lo in (0, 5, 7):                                     # 5 requests per call; the last call has the short ones (n = 1, 2) among its rows
        part, want = sigs[lo: lo + 5], mirror[spb][lo: lo + 5]
        y, spans = _encode(eng, part, spb)
        owned = np.zeros(y.size, bool)
        for k, ((off, n), w) in enumerate(zip(spans, want)):
            owned[off: off + n] = True
            assert n == w.size and np.array_equal(y[off: off + n], w), (spb, lo + k)
        assert (y[~owned] == CANARY).all()                    # nothing outside the rows' ranges


@pytest.mark.parametrize("spb", U.SPBS)
def test_a_request_alone_equals_itself_in_the_batch_and_at_another_row(eng, mirror, spb):
    sigs = _batch(spb)[:5]
    y, spans = _encode(eng, [sigs[2]], spb)
    assert np.array_equal(y[spans[0][0]: spans[0][0] + spans[0][1]], mirror[spb][2])
    y, spans = _encode(eng, sigs, spb, order=[4, 2, 0, 3, 1], gap=12)
    for (off, n), w in zip(spans, mirror[spb][:5]):
        assert np.array_equal(y[off: off + n], w)


def test_pcm_adpcm_refuses_rows_that_do_not_fit(eng):
    x = torch.zeros(4000, dtype=torch.int16, device=eng.device)
    for rows, spb in (([[0, 0, 0]], 505), ([[0, 10, 2]], 505), ([[3995, 10, 0]], 505), ([[0, 10, 0]], 504), ([[0, 600, 0], [0, 10, 256]], 505)):
        with pytest.raises(ValueError):
            eng.pcm_adpcm(x, rows, spb)
    rows_d = torch.tensor([[0, 10, 2]], dtype=torch.int64)
    y = torch.zeros(1024, dtype=torch.uint8, device=eng.device)
    with eng._lock:                                           # the C entry checks the same on its own
        rc = eng.lib.vv_pcm_adpcm(eng.ctx, x.data_ptr(), 4000, rows_d.to(eng.device).data_ptr(), rows_d.data_ptr(), 1, 505, y.data_ptr(), 1024, None)
    assert rc == -22 and not y.cpu().numpy().any()


# ------------------------------------------------------------------ decoder
def _clips(eng, files):
    ap = _ap()
    pcm, res = eng.wav_clips([ap.wav_container(d) for d in files])
    host, out = pcm.cpu().numpy(), []
    for r in res:
        if isinstance(r, Exception):
            out.append(r)
            continue
        off, n, width, rate, ch = r
        out.append((host[off: off + n * ch * 2].view(np.int16).reshape(n, ch).copy(), width, rate))
    return out


def test_wav_decode_equals_mirror_sample_for_sample_in_one_call(eng):
    ap = _ap()
    files = U.decoder_files()
    got = _clips(eng, [f[1] for f in files])
    kinds = set()
    for (name, data, want, rate), g in zip(files, got):
        assert not isinstance(g, Exception), (name, g)
        frames, width, mrate = ap._decode_wav(data)
        assert g[1:] == (2, rate) == (width, mrate) and g[0].shape == frames.shape and np.array_equal(g[0], frames), name
        if not isinstance(want, tuple):
            assert np.array_equal(g[0], want), name           # and both equal the plain-Python reference
        kinds.add(name.split("_")[0] + ("2" if frames.shape[1] == 2 else "1"))
    assert {"ulaw1", "alaw1", "adpcm1", "adpcm2"} <= kinds


def test_a_bad_step_index_sets_its_own_status_and_leaves_the_other_clips_intact(eng):
    ap = _ap()
    files = {f[0]: f[1] for f in U.decoder_files()}
    for ch in (1, 2):
        bad, at = U.bad_index_file(ch, block=2)
        with pytest.raises(ap.WavError) as e:
            ap._decode_wav(bad)
        batch = [files["adpcm_8000_2ch"], bad, files["ulaw_1ch"], files["adpcm_24000_1ch"]]
        got = _clips(eng, batch)
        assert isinstance(got[1], ap.WavError) and (got[1].code, got[1].position) == (e.value.code, e.value.position) == (ap.WavStatus.STEP_INDEX, at)
        for k in (0, 2, 3):
            assert np.array_equal(got[k][0], ap._decode_wav(batch[k])[0])


def _bank(eng, **kw):
    from vietvoice_tts_amd.voice_bank import VoiceBank
    return VoiceBank(eng, 24000, **kw)


def _pcm16_wav(frames, rate):
    x = np.ascontiguousarray(frames, dtype="<i2")
    return U.wav_file(1, x.shape[1], rate, 2 * x.shape[1], 16, x.tobytes())


def test_voice_bank_entries_from_coded_clips_equal_entries_from_their_decoded_pcm16(eng, tmp_path):
    ap = _ap()
    coded = []
    for rate, ch in ((8000, 1), (16000, 2)):                 # ADPCM: mono at 8 kHz, stereo at 16 kHz
        x = np.stack([speechlike(7 * 505 + 100, seed=40 + c, sr=rate) for c in range(ch)], axis=1)[: 7 * 505]
        coded.append(U.wav_file(0x11, ch, rate, 256 * ch, 4, U.adpcm_payload(x, 256 * ch, seed=rate), fact=7 * 505 - 33, samples_per_block=505))
    for rate, ch in ((8000, 1), (16000, 2)):                 # mu-law, and A-law in stereo
        x = speechlike(4001 * ch, seed=50 + ch, sr=rate)
        coded.append(U.wav_file(7 if ch == 1 else 6, ch, rate, ch, 8, (ap.lin2ulaw if ch == 1 else ap.lin2alaw)(x), fact=4001))
    plain = [_pcm16_wav(ap._decode_wav(d)[0], ap._decode_wav(d)[2]) for d in coded]
    from_plain = _bank(eng).ingest_many(plain)
    from_coded = _bank(eng).ingest_many(coded)
    for d, a, b in zip(coded, from_coded, from_plain):
        assert a.pcm_host.dtype == np.int16 and a.pcm_host.size > 0 and np.array_equal(a.pcm_host, b.pcm_host)
        assert np.array_equal(a.pcm_dev.cpu().numpy(), b.pcm_dev.cpu().numpy()) and np.array_equal(a.pcm_host, ap.AudioProcessor.load_audio(d, 24000))
    # coded, plain and a path mixed in one ingest_many
    p = tmp_path / "voice.wav"
    p.write_bytes(coded[1])
    mixed = _bank(eng).ingest_many([plain[0], coded[2], str(p), coded[0], plain[3]])
    for e, j in zip(mixed, (0, 2, 1, 0, 3)):
        assert np.array_equal(e.pcm_host, from_plain[j].pcm_host) and np.array_equal(e.pcm_dev.cpu().numpy(), from_plain[j].pcm_host)
    poly = _bank(eng, resampler="polyphase")
    assert np.array_equal(poly.get(coded[1]).pcm_host, poly.get(plain[1]).pcm_host)              # the opt-in path: frames copied back
    bad, _at = U.bad_index_file(1)
    with pytest.raises(ap.WavError):
        _bank(eng).ingest_many([plain[0], bad])


# ------------------------------------------------------------------ engine
@pytest.fixture(scope="module")
def tiny(tmp_path_factory):
    from vietvoice_tts_amd.core import ModelConfig, TTSEngine
    e = TTSEngine(ModelConfig(model_cache_dir=str(tmp_path_factory.mktemp("adpcm_models")), synthetic_model=True, nfe_step=5, acoustic_dtype="fp32",
                              max_chunk_duration=8.0, model_spec="tiny", noise_source="device", output_stage="device"))
    yield e
    e.cleanup()


def _say(e, stream=False, **kw):
    """One call from call serial 0 (the same start noise every time); a user clip excludes the config's voice filters."""
    c = e.config
    saved = (c.gender, c.group, c.area, c.emotion)
    if kw:
        c.gender = c.group = c.area = c.emotion = None
    e.model_session_manager.noise_serial = 0
    try:
        return list(e.synthesize_stream(TEXT, **kw)) if stream else e.synthesize(TEXT, **kw)[0]
    finally:
        c.gender, c.group, c.area, c.emotion = saved


class _Spy:
    """The library handle with the names of the entries that were fetched from it."""

    def __init__(self, lib):
        self.lib, self.names = lib, []

    def __getattr__(self, name):
        self.names.append(name)
        return getattr(self.lib, name)


@pytest.mark.parametrize("rate,limiter", [(None, None), (8000, None), (None, "sample")])
def test_engine_writes_streams_and_reads_back_its_own_adpcm(tiny, tmp_path, rate, limiter):
    ap = _ap()
    e, c = tiny, tiny.config
    hip = e.model_session_manager.engine
    try:
        c.output_sample_rate, c.output_limiter = rate, limiter
        spy = _Spy(hip.lib)
        hip.lib = spy
        try:
            pcm = _say(e)
        finally:
            hip.lib = spy.lib
        assert pcm.dtype == np.int16 and "vv_join_chunks" in spy.names
        assert "vv_pcm_adpcm" not in spy.names and "vv_wav_decode" not in spy.names               # unset: neither entry is called
        c.output_encoding = "adpcm"
        path = tmp_path / f"own_{rate}_{limiter}.wav"
        hip.lib = spy = _Spy(hip.lib)
        try:
            e.model_session_manager.noise_serial = 0
            made = e.synthesize(TEXT, output_path=str(path))[0]
        finally:
            hip.lib = spy.lib
        assert "vv_pcm_adpcm" in spy.names and "vv_pcm_flac" not in spy.names and "vv_pcm_encode" not in spy.names
        out_rate = rate or c.sample_rate
        assert made.dtype == np.uint8 and np.array_equal(made, ap.encode_output(pcm, "adpcm", out_rate))      # the mirror of the PCM result
        assert path.read_bytes() == made.tobytes() and struct.unpack("<I", made[48:52].tobytes())[0] == pcm.size
        blocks = _say(e, stream=True)
        assert all(b.dtype == np.uint8 for b in blocks) and np.array_equal(np.concatenate(blocks), made[60:])    # the file's data chunk
        c.output_encoding, c.output_sample_rate, c.output_limiter = "pcm16", None, None
        # its own file as the voice == the PCM16 WAV of the samples the mirror decodes from it
        frames, _w, frate = ap._decode_wav(made.tobytes())
        assert frate == out_rate
        (tmp_path / "own_pcm.wav").write_bytes(_pcm16_wav(frames, frate))
        hip.lib = spy = _Spy(hip.lib)
        try:
            a = _say(e, reference_audio=str(path), reference_text=TEXT)
        finally:
            hip.lib = spy.lib
        b = _say(e, reference_audio=str(tmp_path / "own_pcm.wav"), reference_text=TEXT)
        assert "vv_wav_decode" in spy.names and a.dtype == np.int16 and a.size > 0 and np.array_equal(a, b)
        assert e.validate_configuration(str(path)) is True
    finally:
        c.output_encoding, c.output_sample_rate, c.output_limiter = "pcm16", None, None


def test_engine_takes_its_own_ulaw_file_back_as_a_voice(tiny, tmp_path):
    ap = _ap()
    e, c = tiny, tiny.config
    try:
        c.output_encoding, c.output_sample_rate = "ulaw", 8000
        path = tmp_path / "own_ulaw.wav"
        e.model_session_manager.noise_serial = 0
        codes = e.synthesize(TEXT, output_path=str(path))[0]
    finally:
        c.output_encoding, c.output_sample_rate = "pcm16", None
    frames, _w, rate = ap._decode_wav(path.read_bytes())
    assert rate == 8000 and np.array_equal(frames[:, 0], ap.ulaw2lin(codes))
    (tmp_path / "own_ulaw_pcm.wav").write_bytes(_pcm16_wav(frames, rate))
    a = _say(e, reference_audio=str(path), reference_text=TEXT)
    b = _say(e, reference_audio=str(tmp_path / "own_ulaw_pcm.wav"), reference_text=TEXT)
    assert a.size > 0 and np.array_equal(a, b)
