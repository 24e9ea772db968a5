"""-m gpu: N15, the FLAC encoder on the device (csrc/vv_flac.hip) and the FLAC end of the output stage.  The yardstick is the host mirror
(core/audio_processor.py: flac_encode_frames), which the kernels must equal BYTE FOR BYTE, frame sizes and offsets included; what the
bytes mean is checked by the stand-alone decoder of tests/flac_util.py.  The mirror itself is held against that decoder and a brute-force
reference in tests/test_flac_cpu.py."""
import numpy as np
import pytest
import torch

from tests.flac_util import BLOCK, decode_frames, decode_stream, device_cases, mirror_layout, signals
from tests.output_util import lsb_condition, pack_requests

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
SR = 24000
GUARD = 256
FILL = 0xAA
SHORT = "Xin chào các bạn, hôm nay trời đẹp quá."
LONG = "Hôm nay trời đẹp quá, chúng ta cùng nhau đi dạo quanh hồ nhé. " * 4


@pytest.fixture(scope="module")
def eng(hip_tiny):
    return hip_tiny["f32"]


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


@pytest.fixture(scope="module")
def cases():
    """The rows of the device tests with the mirror's frames, computed once: [(name, pcm, frame0, last, frames)]."""
    from vietvoice_tts_amd.core.audio_processor import flac_encode_frames
    res = [c + (flac_encode_frames(c[1], SR, c[2], bool(c[3]))[0],) for c in device_cases()]
    assert {c[0] for c in res} >= set(signals()) and any(c[3] == 0 for c in res) and any(c[1].size == 1 for c in res)
    return res


def _raw(eng, items, gap=3, rate=SR):
    """Device buffers of one vv_pcm_flac call over ``items``, made ahead of it: sources at odd offsets with junk between, y between guard
    bands.  -> (call(**overrides), whole y buffer, info, rows, n_y, buffers)."""
    plane, reqs = pack_requests([[c[1]] for c in items], gap=gap)
    rows = [[so, n, c[2], c[3]] for c, ((so, n),) in zip(items, reqs)]
    _want, _info, n_y = mirror_layout([c[:4] for c in items], rate)
    x = _dev(plane)
    whole = torch.full((GUARD + n_y + GUARD,), FILL, dtype=torch.uint8, device=DEV)
    info = torch.full((len(items) + 1, 3), -7, dtype=torch.int64, device=DEV)
    rows_h = torch.tensor(rows, dtype=torch.int64)
    rows_d = rows_h.to(DEV)
    frames = sum(-(-r[1] // BLOCK) for r in rows)
    ws = torch.zeros((int(eng.lib.vv_pcm_flac_ws_bytes(frames, len(rows))) // 8 + 1,), dtype=torch.int64, device=DEV)

    def call(**kw):
        a = dict(x=x.data_ptr(), n_x=x.numel(), rows=rows_d.data_ptr(), rows_h=rows_h.data_ptr(), R=len(rows), rate=rate,
                 y=whole.data_ptr() + GUARD, n_y=n_y, info=info.data_ptr(), ws=ws.data_ptr(), ws_bytes=ws.numel() * 8)
        a.update(kw)
        return eng.lib.vv_pcm_flac(eng.ctx, a["x"], a["n_x"], a["rows"], a["rows_h"], a["R"], a["rate"], a["y"], a["n_y"], a["info"], a["ws"],
                                   a["ws_bytes"], torch.cuda.current_stream().cuda_stream)
    return call, whole, info, rows, n_y, (x, rows_h, rows_d, ws)


def _launch(eng, items, order=None, gap=3, rate=SR):
    """One call over ``items`` in ``order``, everything checked against the mirror.  -> {name: the request's frames}."""
    items = [items[i] for i in (range(len(items)) if order is None else order)]
    call, whole, info, _rows, n_y, _keep = _raw(eng, items, gap, rate)
    assert call() == 0
    torch.cuda.synchronize()
    host, got_info = whole.cpu().numpy(), info.cpu().numpy()
    want, want_info, bound = mirror_layout([c[:4] for c in items], rate)
    assert bound == n_y and np.array_equal(got_info, want_info)
    total = int(got_info[-1, 0])
    assert total == want.size and np.array_equal(host[GUARD: GUARD + total], want)
    assert (host[:GUARD] == FILL).all() and (host[GUARD + total:] == FILL).all(), "a byte outside the frames was written"
    return {c[0]: host[GUARD + int(got_info[j, 0]): GUARD + int(got_info[j + 1, 0])].copy() for j, c in enumerate(items)}


@pytest.fixture(scope="module")
def batch(eng, cases):
    order = list(np.random.default_rng(4).permutation(len(cases)))
    return _launch(eng, cases, order)


def test_one_call_over_every_signal_equals_the_mirror_and_decodes(cases, batch):
    assert len(batch) == len(cases)
    kinds = set()
    for name, x, frame0, _last, frames in cases:
        assert np.array_equal(batch[name], frames), name
        samples, what, _numbers = decode_frames(batch[name], SR, frame0)
        assert np.array_equal(samples, x), name
        kinds.update((w[0], w[1], w[2]) for w in what)
    assert {k[0] for k in kinds} == {"constant", "verbatim", "fixed"}
    ties = [c for c in cases if c[0].startswith("verbatim_tie_")]      # best Fixed == 8 + 16 m bits: the device keeps Fixed(0, 0) as well
    assert len(ties) == 3
    for name, x, frame0, _last, _frames in ties:
        what = decode_frames(batch[name], SR, frame0)[1]
        assert what[0][:3] == ("fixed", 0, 0) and 8 * (what[0][4] - 10) == 8 + 16 * x.size, name     # 8 header bytes, 2 of CRC-16
    assert {k[1] for k in kinds if k[0] == "fixed"} == {0, 1, 2, 3, 4} and {k[2] for k in kinds if k[0] == "fixed"} == {0, 1, 2, 3, 4}


def test_the_same_rows_one_per_call(eng, cases, batch):
    for i, c in enumerate(cases):
        alone = _launch(eng, cases, [i], gap=2 + i % 5)
        assert np.array_equal(alone[c[0]], batch[c[0]]), c[0]


def test_other_rates_and_neighbours(eng, cases):
    from vietvoice_tts_amd.core.audio_processor import flac_encode_frames
    pick = [i for i, c in enumerate(cases) if c[0] in ("speech_13288", "one", "noise_17", "stream_block", "stream_tail", "sine_4101")]
    for rate in (8000, 11025, 65540, 65541):
        got = _launch(eng, cases, pick[::-1], gap=1, rate=rate)
        for i in pick:
            name, x, frame0, last, _f = cases[i]
            assert np.array_equal(got[name], flac_encode_frames(x, rate, frame0, bool(last))[0]), (rate, name)


def test_one_sample_and_33_rows_of_4097(eng):
    x = signals(BLOCK + 1)
    one = [("one", np.array([12345], np.int16), 0, 1)]
    assert decode_frames(_launch(eng, one)["one"], SR, 0)[0].tolist() == [12345]
    names = list(x)
    many = [(f"row{r}", np.roll(x[names[r % len(names)]], r), r * 3, 1) for r in range(33)]             # 66 frames
    got = _launch(eng, many)
    for name, pcm, frame0, _last in many:
        assert np.array_equal(decode_frames(got[name], SR, frame0)[0], pcm), name


def test_captured_into_a_graph_equals_eager(eng, cases):
    items = [c for c in cases if c[0] in ("speech_13288", "switch256", "two", "stream_block")]
    call, whole, info, _rows, _n_y, _keep = _raw(eng, items)
    assert call() == 0
    torch.cuda.synchronize()
    eager, eager_info = whole.clone(), info.clone()
    whole.fill_(FILL)
    info.fill_(-7)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        assert call() == 0                                                            # no synchronisation, no host read-back: capturable
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(whole, eager) and torch.equal(info, eager_info)
    assert np.array_equal(eager.cpu().numpy()[GUARD: GUARD + int(eager_info[-1, 0])], np.concatenate([c[4] for c in items]))


def test_refusals_launch_nothing_and_leave_the_context_usable(eng, cases):
    items = [c for c in cases if c[0] in ("walk_4097", "stream_block", "five")]
    call, whole, info, rows, n_y, (x, rows_h, _rows_d, ws) = _raw(eng, items)
    variants = {k: rows_h.clone() for k in ("past_x", "neg_src", "neg_n", "neg_frame0", "neg_last", "empty", "frames_past_2_31", "partial_block",
                                            "last_2")}
    variants["past_x"][0, 1] = x.numel()
    for col, k in ((0, "neg_src"), (1, "neg_n"), (2, "neg_frame0"), (3, "neg_last")):
        variants[k][0, col] = -1
    variants["empty"][2, 1] = 0
    variants["frames_past_2_31"][0, 2] = (1 << 31) - 1                               # two frames from 2^31 - 1
    variants["partial_block"][1, 1] = 2 * BLOCK - 1                                  # last = 0 with a partial frame
    variants["last_2"][0, 3] = 2
    bads = [dict(R=0), dict(R=-1), dict(R=65536), dict(x=None), dict(rows=None), dict(rows_h=None), dict(y=None), dict(info=None), dict(ws=None),
            dict(x=x.data_ptr() + 1), dict(rows=_rows_d.data_ptr() + 4), dict(info=info.data_ptr() + 4), dict(ws=ws.data_ptr() + 4),
            dict(ws_bytes=ws.numel() * 8 - 64), dict(ws_bytes=0), dict(n_y=n_y - 1), dict(n_y=0), dict(rate=0), dict(rate=-5), dict(rate=655351),
            dict(n_x=100)]
    bads += [dict(rows_h=v.data_ptr()) for v in variants.values()]
    for bad in bads:
        assert call(**bad) == -22, bad
        assert b"vv_pcm_flac" in eng.lib.vv_last_error(eng.ctx)
    torch.cuda.synchronize()
    assert (whole.cpu().numpy() == FILL).all() and (info.cpu().numpy() == -7).all()   # nothing was launched
    for bad_rows in ([[0, 10, 0]], [[x.numel() - 5, 10, 0, 1]], [[0, 0, 0, 1]], [[0, 10, -1, 1]], [[0, 10, 1 << 31, 1]], [[0, 10, 0, 0]], [[0, 10, 0, 2]], []):
        with pytest.raises(ValueError):
            eng.pcm_flac(x, bad_rows, SR)
    for bad_rate in (0, 655351, 8000.5):
        with pytest.raises(ValueError):
            eng.pcm_flac(x, [[0, 10, 0, 1]], bad_rate)
    assert call() == 0                                                                # the context still works
    torch.cuda.synchronize()
    total = int(info[-1, 0])
    assert np.array_equal(whole.cpu().numpy()[GUARD: GUARD + total], np.concatenate([c[4] for c in items]))
    y, inf = eng.pcm_flac(x, rows, SR)                                                # the wrapper: the same bytes
    assert np.array_equal(y[: int(inf[-1, 0])].cpu().numpy(), np.concatenate([c[4] for c in items]))


# ------------------------------------------------------------------ engine, tiny preset
def _engine(tmp, **kw):
    from vietvoice_tts_amd.core import ModelConfig, TTSEngine
    kw = {**dict(model_spec="tiny", noise_source="device"), **kw}
    return TTSEngine(ModelConfig(model_cache_dir=str(tmp), synthetic_model=True, nfe_step=5, acoustic_dtype="fp32", max_chunk_duration=8.0, **kw))


_PLAIN = dict(output_stage="host", output_sample_rate=None, output_encoding="pcm16", output_loudness=None, output_limiter=None,
              output_peak_dbfs=-1.0, output_pitch=None, output_tempo=None)


def _call(e, fn, *a, stage="host", rate=None, enc="pcm16", loud=None, lim=None, peak=-1.0, pitch=None, tempo=None, **k):
    """One engine call under the given output options, from call serial 0 (the same start noise every time)."""
    opts = dict(output_stage=stage, output_sample_rate=rate, output_encoding=enc, output_loudness=loud, output_limiter=lim, output_peak_dbfs=peak,
                output_pitch=pitch, output_tempo=tempo)
    for key, v in opts.items():
        setattr(e.config, key, v)
    e.model_session_manager.noise_serial = 0
    try:
        out = fn(*a, **k)
        return list(out) if fn == e.synthesize_stream else out
    finally:
        for key, v in _PLAIN.items():
            setattr(e.config, key, v)


@pytest.fixture(scope="module")
def tiny(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("flac_models")
    e = _engine(tmp)
    base = {t: _call(e, e.synthesize, t)[0] for t in (SHORT, LONG)}
    assert len(e._last_plan) >= 3 and base[LONG].dtype == np.int16 and base[LONG].size > 2 * BLOCK
    yield e, base
    e.cleanup()


def test_other_encodings_never_call_the_new_entry(tiny, monkeypatch):
    e, base = tiny
    lib, calls = e.model_session_manager.engine.lib, []
    real = lib.vv_pcm_flac
    monkeypatch.setattr(lib, "vv_pcm_flac", lambda *a: calls.append("vv_pcm_flac") or real(*a))
    for kw in (dict(), dict(stage="device"), dict(rate=8000, enc="ulaw"), dict(enc="alaw"), dict(lim="true")):
        _call(e, e.synthesize, LONG, **kw)
    _call(e, e.synthesize_stream, LONG, rate=8000, enc="ulaw")
    assert not calls
    e.config.output_encoding = "flac"
    try:
        assert e._device_output()                             # the HIP engine takes the device stage for it
    finally:
        e.config.output_encoding = "pcm16"
    _call(e, e.synthesize, LONG, enc="flac")
    assert calls == ["vv_pcm_flac"]


def test_flac_file_decodes_to_the_pcm_of_the_same_call(tiny, tmp_path):
    from vietvoice_tts_amd.core.audio_processor import encode_output
    e, base = tiny
    for text in (SHORT, LONG):                                # one chunk and several
        path = tmp_path / f"{len(text)}.flac"
        got, _ = _call(e, e.synthesize, text, enc="flac", output_path=str(path))
        samples, frames, info = decode_stream(path.read_bytes())
        assert got.dtype == np.uint8 and path.read_bytes() == got.tobytes()
        assert np.array_equal(samples, base[text]) and info["rate"] == SR and info["total"] == base[text].size
        assert (info["min_frame"], info["max_frame"]) == (min(f[4] for f in frames), max(f[4] for f in frames))
        assert np.array_equal(got, encode_output(base[text], "flac", SR))            # host and device files are equal


def test_finish_output_against_the_host_finish(tiny):
    """The FLAC end of finish_output against what _finish_host computes.  The 8 kHz case is NOT a host/device file comparison: the
    device's rate conversion is held to the host chain only under N10's 1-LSB resampler bound, so the file is compared with
    encode_output of the DEVICE's own 8 kHz PCM (the FLAC step itself is exact) and the decoded samples with the host chain under that
    bound.  The limiter case is exact end to end: the whole file equals the host's."""
    from vietvoice_tts_amd.core.audio_processor import encode_output, limit_peaks, resample_output
    e, base = tiny
    # a request of several chunks at 8 kHz: the device's rate conversion is held to N10's bound, the FLAC step on top of it is exact
    pcm8, _ = _call(e, e.synthesize, LONG, rate=8000)
    got, _ = _call(e, e.synthesize, LONG, rate=8000, enc="flac")
    samples, _f, info = decode_stream(got)
    assert info["rate"] == 8000 and np.array_equal(samples, pcm8) and np.array_equal(got, encode_output(pcm8, "flac", 8000))
    lsb_condition(samples, resample_output(base[LONG], SR, 8000))
    # a request with a limiter: bit-exact on the device, so the whole file equals the host's
    want = encode_output(limit_peaks(base[LONG], SR, -1.0, "true")[0], "flac", SR)
    got, _ = _call(e, e.synthesize, LONG, lim="true", enc="flac")
    assert np.array_equal(got, want)
    # finish_output itself: two requests in one call, each equal to itself alone
    eng_ = e.model_session_manager.engine
    a, b = base[SHORT], base[LONG][: 2 * BLOCK + 77]
    plane = torch.from_numpy(np.concatenate([a, b])).to(DEV)
    outs = eng_.finish_output(plane, [[(0, a.size)], [(a.size, b.size)]], e.config.cross_fade_duration, SR, None, "flac")
    assert np.array_equal(outs[0], encode_output(a, "flac", SR)) and np.array_equal(outs[1], encode_output(b, "flac", SR))


def test_stream_blocks_decode_to_the_pcm_of_synthesize(tiny):
    e, base = tiny
    for step in (1, 2):
        blocks = _call(e, e.synthesize_stream, LONG, enc="flac", chunks_per_step=step)
        samples, _f, info = decode_stream(np.concatenate(blocks))
        assert len(blocks) > 1 and all(b.dtype == np.uint8 for b in blocks) and info["total"] == 0
        assert np.array_equal(samples, base[LONG]), step
    pcm8, _ = _call(e, e.synthesize, LONG, rate=8000, lim="sample")
    blocks = _call(e, e.synthesize_stream, LONG, rate=8000, lim="sample", enc="flac")
    samples, _f, info = decode_stream(np.concatenate(blocks))
    assert info["rate"] == 8000 and np.array_equal(samples, pcm8)
