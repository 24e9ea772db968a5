"""-m gpu: N22, the keyed audio watermark on the device (csrc/vv_watermark.hip) and its place in the output stage.  The yardstick is the host
mirror (core/audio_processor.py: watermark_embed, watermark_cells, watermark_stats), which the kernels must equal BIT FOR BIT -- the int16
output, every int32 cell value and every int64 of the statistic.  What the mirror detects is measured in tests/test_watermark_cpu.py."""
import numpy as np
import pytest
import torch

from tests import watermark_util as wu
from tests.output_util import pack_requests

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
SR = wu.SR
GUARD = 64
SENTINEL = 0x5555
SHORT = "Xin chào các bạn, hôm nay trời đẹp quá."
LONG = "Hôm nay trời đẹp quá, chúng ta cùng nhau đi dạo quanh hồ nhé. " * 4


def _ap():
    from vietvoice_tts_amd.core import audio_processor
    return audio_processor


@pytest.fixture(scope="module")
def eng(hip_tiny):
    return hip_tiny["f32"]


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _embed(eng, sigs, payloads, strength, gap=3, lead=0):
    """One vv_pcm_watermark call: the signals at offsets that are no multiple of the hop with junk between, y between guard samples of
    0x5555 with gaps.  -> [z] per signal; asserts that nothing outside the spans was written."""
    plane, reqs = pack_requests([[s] for s in sigs], gap=gap)
    plane = np.concatenate([np.full(lead, 32767, np.int16), plane])
    rows, dst = [], GUARD + 1
    for k, ((xo, n),) in enumerate(reqs):
        rows.append([xo + lead, n, dst])
        dst += n + 1 + (k % 4)
    out = torch.full((dst + GUARD,), SENTINEL, dtype=torch.int16, device=DEV)
    host = eng.pcm_watermark(_dev(plane), rows, wu.KEY, payloads, strength, out=out).cpu().numpy()
    written = np.zeros(host.size, bool)
    res = []
    for row in rows:
        written[row[2]: row[2] + row[1]] = True
        res.append(host[row[2]: row[2] + row[1]].copy())
    assert (host[~written] == SENTINEL).all(), "a sample outside a request's output was written"
    return res


# ------------------------------------------------------------------ the embedder
@pytest.mark.parametrize("strength", (0.0, 0.2, 0.5))
def test_embed_equals_the_mirror_bit_for_bit(eng, strength):
    ap = _ap()
    sigs = [wu.speechlike(n, 300 + n) for n in wu.LENGTHS]
    payloads = [0x1234, 0xBEEF, 0]
    for group in (sigs[0:3], sigs[3:6], [sigs[6], sigs[0], sigs[4]]):                 # R = 3 ragged rows per call, every length
        got = _embed(eng, group, payloads, strength)
        for x, p, z in zip(group, payloads, got):
            want = ap.watermark_embed(x, wu.KEY, p, strength)
            assert z.dtype == np.int16 and np.array_equal(z, want), (x.size, np.nonzero(z != want)[0][:8])
            if strength == 0.0:
                assert np.array_equal(z, x)                                           # strength 0 returns the input sample for sample
    if strength:
        assert not np.array_equal(got[0], sigs[6])


def test_a_row_in_a_batch_equals_itself_alone(eng):
    sigs = [wu.speechlike(n, 700 + n) for n in (1, 257, 3000, 5000)]
    payloads = [1, 0xFFFF, 0x1234, 0xBEEF]
    batch = _embed(eng, sigs, payloads, 0.2, gap=7)
    for k, x in enumerate(sigs):
        alone = _embed(eng, [x], [payloads[k]], 0.2, gap=1, lead=4321 if k == 3 else 0)[0]
        assert np.array_equal(alone, batch[k]), x.size
    other = _embed(eng, [sigs[3]], [payloads[2]], 0.2)[0]
    assert not np.array_equal(other, batch[3])                                        # the payload is in the audio


# ------------------------------------------------------------------ the detector
@pytest.mark.parametrize("marked", (True, False))
def test_detect_stats_and_cells_equal_the_mirror_exactly(eng, marked):
    ap = _ap()
    make = (lambda n, seed: ap.watermark_embed(wu.speechlike(n, seed), wu.KEY, 0x1234, 0.2)) if marked else wu.speechlike
    sigs = {n: make(n, 40 + n % 7) for n in (1, 1023, 5000, 96000)}
    for lens in ((1, 1023, 5000), (96000, 1, 5000)):                                  # R = 3 ragged rows per call
        plane, reqs = pack_requests([[sigs[n]] for n in lens], gap=5)
        rows = [[xo, n] for ((xo, n),) in reqs]
        stats, cells, frame_offs = eng.pcm_watermark_detect(_dev(plane), rows, wu.KEY, cells=True)
        stats, cells = stats.cpu().numpy(), cells.cpu().numpy()
        assert stats.shape == (3, wu.Q, wu.NB, 2) and stats.dtype == np.int64 and cells.dtype == np.int32
        assert frame_offs == list(np.cumsum([0] + [wu.frames_of(n) for n in lens]))
        for k, n in enumerate(lens):
            want_cells = ap.watermark_cells(sigs[n])
            got_cells = cells[frame_offs[k]: frame_offs[k + 1]]
            assert np.array_equal(got_cells, want_cells), (n, np.argwhere(got_cells != want_cells)[:4])
            want = ap.watermark_stats(sigs[n], wu.KEY)
            assert np.array_equal(stats[k], want), (n, np.argwhere(stats[k] != want)[:4])
        plain = eng.pcm_watermark_detect(_dev(plane), rows, wu.KEY).cpu().numpy()     # without cells_out: the cells stay in the workspace
        assert np.array_equal(plain, stats)
    r = ap.watermark_decide(stats[0])                                                 # the 4 s clip
    print(f"marked {marked}: score {r.score:.3f} offset {r.offset}")
    assert (r.present, r.payload) == ((True, 0x1234) if marked else (False, r.payload)) and (not marked or r.offset == 0)
    other = eng.pcm_watermark_detect(_dev(plane), rows, wu.WRONG_KEY).cpu().numpy()   # another key: another table on the device
    assert np.array_equal(other[0], ap.watermark_stats(sigs[96000], wu.WRONG_KEY)) and not ap.watermark_decide(other[0]).present


# ------------------------------------------------------------------ refusals
def _raw(eng):
    """Device buffers of one two-row call of each entry, made ahead of it."""
    ap = _ap()
    window, tw = eng._denoise_tables
    chips = eng._watermark_chips(wu.KEY)
    sigs = [wu.speechlike(700, 41), wu.speechlike(257, 42)]
    plane, reqs = pack_requests([[s] for s in sigs], gap=3)
    rows, dst = [], GUARD
    for ((xo, n),), p in zip(reqs, (0x1234, 0xBEEF)):
        rows.append([xo, n, dst, ap.watermark_message(p)])
        dst += n + 3
    x = _dev(plane)
    y = torch.full((dst + GUARD,), SENTINEL, dtype=torch.int16, device=DEV)
    rows_h = torch.tensor(rows, dtype=torch.int64)
    rows_d = rows_h.to(DEV)
    drows_h = torch.tensor([[r[0], r[1], 0, 0] for r in rows], dtype=torch.int64)
    drows_d = drows_h.to(DEV)
    frames = sum(wu.frames_of(s.size) for s in sigs)
    stats = torch.full((2 * wu.Q * wu.NB * 2,), -7, dtype=torch.int64, device=DEV)
    cells = torch.full((frames * wu.K,), -7, dtype=torch.int32, device=DEV)
    ws = torch.zeros((int(eng.lib.vv_pcm_watermark_ws_bytes(2)) // 8 + 1,), dtype=torch.int64, device=DEV)
    dws = torch.zeros((int(eng.lib.vv_pcm_watermark_detect_ws_bytes(frames, 2)) // 8 + 1,), dtype=torch.int64, device=DEV)

    def embed(stream, **kw):
        a = dict(x=x.data_ptr(), n_x=x.numel(), rows=rows_d.data_ptr(), rows_h=rows_h.data_ptr(), R=2, chips=chips.data_ptr(), n_chips=chips.numel(),
                 gp=1.2, gm=0.8, win=window.data_ptr(), tw=tw.data_ptr(), y=y.data_ptr(), n_y=y.numel(), ws=ws.data_ptr(), ws_bytes=ws.numel() * 8)
        a.update(kw)
        return eng.lib.vv_pcm_watermark(eng.ctx, a["x"], a["n_x"], a["rows"], a["rows_h"], a["R"], a["chips"], a["n_chips"], a["gp"], a["gm"],
                                        a["win"], a["tw"], a["y"], a["n_y"], a["ws"], a["ws_bytes"], stream)

    def detect(stream, **kw):
        a = dict(x=x.data_ptr(), n_x=x.numel(), rows=drows_d.data_ptr(), rows_h=drows_h.data_ptr(), R=2, chips=chips.data_ptr(),
                 n_chips=chips.numel(), win=window.data_ptr(), tw=tw.data_ptr(), stats=stats.data_ptr(), n_stats=stats.numel(),
                 cells=cells.data_ptr(), n_cells=cells.numel(), ws=dws.data_ptr(), ws_bytes=dws.numel() * 8)
        a.update(kw)
        return eng.lib.vv_pcm_watermark_detect(eng.ctx, a["x"], a["n_x"], a["rows"], a["rows_h"], a["R"], a["chips"], a["n_chips"], a["win"], a["tw"],
                                               a["stats"], a["n_stats"], a["cells"], a["n_cells"], a["ws"], a["ws_bytes"], stream)
    return embed, detect, sigs, rows, dict(x=x, y=y, rows_h=rows_h, drows_h=drows_h, stats=stats, cells=cells, ws=ws, dws=dws, window=window, tw=tw,
                                           chips=chips, keep=(rows_d, drows_d))


def test_refusals_launch_nothing_and_leave_the_context_usable(eng):
    ap = _ap()
    embed, detect, sigs, rows, b = _raw(eng)
    x, y, window, tw, chips = b["x"], b["y"], b["window"], b["tw"], b["chips"]
    s = torch.cuda.current_stream().cuda_stream
    variants = {k: b["rows_h"].clone() for k in ("past_x", "past_y", "on_y", "message", "neg_x", "neg_n", "neg_y", "neg_m", "big_n")}
    variants["past_x"][1, 0] = x.numel() - 10
    variants["past_y"][1, 2] = y.numel() - 10
    variants["on_y"][1, 2] = variants["on_y"][0, 2] + 10                              # rows overlapping on y
    variants["message"][0, 3] = 1 << 24
    variants["big_n"][0, 1] = (1 << 30) + 1
    for col, k in ((0, "neg_x"), (1, "neg_n"), (2, "neg_y"), (3, "neg_m")):
        variants[k][0, col] = -1
    common = [dict(R=0), dict(R=-1), dict(R=65536), dict(x=None), dict(rows=None), dict(rows_h=None), dict(chips=None), dict(win=None),
              dict(tw=None), dict(ws=None), dict(x=x.data_ptr() + 1), dict(chips=chips.data_ptr() + 1), dict(win=window.data_ptr() + 4),
              dict(tw=tw.data_ptr() + 4), dict(ws_bytes=8), dict(ws_bytes=0), dict(n_chips=wu.P * wu.K - 1), dict(n_x=100)]
    bads = common + [dict(y=None), dict(y=y.data_ptr() + 1), dict(ws=b["ws"].data_ptr() + 4), dict(y=x.data_ptr(), n_y=x.numel()),
                     dict(y=x.data_ptr() + 2 * (x.numel() - 8), n_y=y.numel()), dict(n_y=500), dict(gp=0.99), dict(gp=1.51), dict(gm=0.49),
                     dict(gm=1.01), dict(gp=float("nan")), dict(gm=float("nan"))]
    bads += [dict(rows_h=v.data_ptr()) for v in variants.values()]
    for bad in bads:
        assert embed(s, **bad) == -22, bad
        assert b"vv_pcm_watermark" in eng.lib.vv_last_error(eng.ctx)
    dvariants = {k: b["drows_h"].clone() for k in ("past_x", "neg_x", "neg_n", "neg_2", "neg_3", "big_n")}
    dvariants["past_x"][1, 0] = x.numel() - 10
    dvariants["big_n"][0, 1] = (1 << 24) + 1
    for col, k in ((0, "neg_x"), (1, "neg_n"), (2, "neg_2"), (3, "neg_3")):
        dvariants[k][0, col] = -1
    dbads = common + [dict(stats=None), dict(stats=b["stats"].data_ptr() + 4), dict(cells=b["cells"].data_ptr() + 2), dict(ws=b["dws"].data_ptr() + 4),
                      dict(n_stats=b["stats"].numel() - 1), dict(n_cells=b["cells"].numel() - 1), dict(ws_bytes=b["dws"].numel() * 8 - 4000)]
    dbads += [dict(rows_h=v.data_ptr()) for k, v in dvariants.items()]
    for bad in dbads:
        assert detect(s, **bad) == -22, bad
        assert b"vv_pcm_watermark_detect" in eng.lib.vv_last_error(eng.ctx)
    big = torch.tensor([[0, (1 << 24) + 1, 0, 0], [0, 1, 0, 0]], dtype=torch.int64)   # n > 2^24 for the detector, with an n_x that would hold it
    assert detect(s, rows_h=big.data_ptr(), n_x=1 << 25) == -22
    torch.cuda.synchronize()
    assert (y.cpu().numpy() == SENTINEL).all() and (b["stats"].cpu().numpy() == -7).all() and (b["cells"].cpu().numpy() == -7).all()
    for bad_rows in ([[0, 10]], [[x.numel() - 5, 10, 0]], [[0, 10, -1]], [[0, 300, 0], [300, 300, 299]], []):
        with pytest.raises(ValueError):
            eng.pcm_watermark(x, bad_rows, wu.KEY, 1)
    for kw in (dict(payloads=65536), dict(payloads=[1, 2]), dict(strength=0.6), dict(key=-1), dict(key=None)):
        args = dict(key=wu.KEY, payloads=1, strength=0.2)
        args.update(kw)
        with pytest.raises(ValueError):
            eng.pcm_watermark(x, [[0, 10, 0]], args["key"], args["payloads"], args["strength"])
    with pytest.raises(ValueError):
        eng.pcm_watermark(x, [[0, 10, 0]], wu.KEY, 1, out=x)                          # not in place
    for bad_rows in ([[0, x.numel() + 1]], [[-1, 5]], [[0, 5, 0]], []):
        with pytest.raises(ValueError):
            eng.pcm_watermark_detect(x, bad_rows, wu.KEY)
    assert embed(s) == 0 and detect(s, cells=None, n_cells=0) == 0                    # cells_out is optional; the context still works
    torch.cuda.synchronize()
    host = y.cpu().numpy()
    for k, (sig, row, p) in enumerate(zip(sigs, rows, (0x1234, 0xBEEF))):
        assert np.array_equal(host[row[2]: row[2] + row[1]], ap.watermark_embed(sig, wu.KEY, p, 0.2))
        assert np.array_equal(b["stats"].cpu().numpy().reshape(2, wu.Q, wu.NB, 2)[k], ap.watermark_stats(sig, wu.KEY))
    assert (b["cells"].cpu().numpy() == -7).all()


# ------------------------------------------------------------------ PcmStage.finish_output
def _counted(monkeypatch, lib):
    calls = []
    for name in ("vv_pcm_watermark", "vv_pcm_watermark_detect"):
        real = getattr(lib, name)
        monkeypatch.setattr(lib, name, lambda *a, _n=name, _r=real: calls.append(_n) or _r(*a))
    return calls


def test_finish_output_chain_equals_the_mirrors_and_unset_is_todays_bytes(eng, monkeypatch):
    ap = _ap()
    calls = _counted(monkeypatch, eng.lib)
    sigs = [wu.speechlike(5000, 71), wu.speechlike(3000, 72), wu.speechlike(2000, 73)]
    plane, reqs = pack_requests([[s] for s in sigs], gap=7)
    pcm = _dev(plane)
    chain = dict(loudness=-20.0, peak_dbfs=-3.0, limiter=["sample", None, "true"])
    today = eng.finish_output(pcm, reqs, 0.1, SR, 8000, "ulaw", **chain)
    for kw in (dict(watermark=None), dict(watermark=[None, None, None]), dict(watermark=None, watermark_key=wu.KEY), dict(watermark_key=wu.KEY)):
        got = eng.finish_output(pcm, reqs, 0.1, SR, 8000, "ulaw", **chain, **kw)
        assert all(np.array_equal(a, b) for a, b in zip(got, today)) and not calls    # byte for byte, and nothing new is called
    payloads = [0x1234, None, 0xBEEF]
    got = eng.finish_output(pcm, reqs, 0.1, SR, None, "pcm16", **chain, watermark=payloads, watermark_key=wu.KEY, watermark_strength=0.3)
    assert calls == ["vv_pcm_watermark"]
    for x, p, lim, g in zip(sigs, payloads, chain["limiter"], got):                   # behind the join, before the loudness step: every link the mirror's
        marked = x if p is None else ap.watermark_embed(x, wu.KEY, p, 0.3)
        assert np.array_equal(g, ap.normalize_loudness(marked, SR, -20.0, -3.0, limiter=lim))
    for bad in (dict(watermark=1), dict(watermark=65536, watermark_key=wu.KEY), dict(watermark=[1, 2], watermark_key=wu.KEY),
                dict(watermark=1, watermark_key=wu.KEY, watermark_strength=0.0), dict(watermark=1, watermark_key=-1)):
        with pytest.raises(ValueError):
            eng.finish_output(pcm, reqs, 0.1, SR, **bad)


# ------------------------------------------------------------------ engine, tiny preset
@pytest.fixture(scope="module")
def tiny(tmp_path_factory):
    from vietvoice_tts_amd.core import ModelConfig, TTSEngine
    tmp = tmp_path_factory.mktemp("watermark_models")
    e = TTSEngine(ModelConfig(model_cache_dir=str(tmp), synthetic_model=True, nfe_step=5, acoustic_dtype="fp32", max_chunk_duration=8.0,
                              model_spec="tiny", noise_source="device", output_watermark_key=wu.KEY, output_watermark_payload=0x1234))
    assert e._device_output()
    yield e
    e.cleanup()


def _call(e, fn, *a, key=wu.KEY, **cfg):
    """One engine call under the given options, from call serial 0 (the same start noise every time)."""
    old = {k: getattr(e.config, k) for k in cfg}
    old["output_watermark_key"] = e.config.output_watermark_key
    e.config.output_watermark_key = key
    for k, v in cfg.items():
        setattr(e.config, k, v)
    e.model_session_manager.noise_serial = 0
    try:
        return fn(*a)
    finally:
        for k, v in old.items():
            setattr(e.config, k, v)


def test_engine_device_and_host_finishes_agree_and_files_are_detected(tiny, monkeypatch, tmp_path):
    ap = _ap()
    e = tiny
    calls = _counted(monkeypatch, e.model_session_manager.engine.lib)
    base = _call(e, e.synthesize, LONG, key=None)[0]
    assert not calls                                                                  # no key: nothing new is called
    got = _call(e, e.synthesize, LONG)[0]
    assert calls == ["vv_pcm_watermark"]
    calls.clear()
    want = ap.watermark_embed(base, wu.KEY, 0x1234, 0.2)
    assert got.dtype == np.int16 and np.array_equal(got, want) and not np.array_equal(got, base)
    with monkeypatch.context() as m:                                                  # the same call finished on the host
        m.setattr(e, "_device_output", lambda *a, **k: False)
        host = _call(e, e.synthesize, LONG)[0]
    assert np.array_equal(host, got) and not calls
    r = e.detect_watermark(got)
    print(f"{got.size / SR:.1f} s of the tiny model: score {r.score:.3f} offset {r.offset}")
    assert calls == ["vv_pcm_watermark_detect"] and r == ap.watermark_detect(got, wu.KEY)
    assert r.present and r.crc_ok and r.payload == 0x1234 and r.offset == 0
    assert not e.detect_watermark(base).present and not e.detect_watermark(got, key=wu.WRONG_KEY).present
    flac = _call(e, e.synthesize, LONG, output_encoding="flac")[0]                    # the engine's own FLAC and WAV output, as bytes and as a path
    wav = str(tmp_path / "marked.wav")
    e.audio_processor.save_audio(got, wav, SR)
    calls.clear()
    many = e.detect_watermark([flac.tobytes(), wav, got[wu.CUT:]])
    assert calls == ["vv_pcm_watermark_detect"]                                       # one device call for all clips
    assert [(m_.present, m_.payload) for m_ in many] == [(True, 0x1234)] * 3 and many[2].offset in (20, 21)
    with pytest.raises(ValueError, match="output_watermark_key"):
        _call(e, e.synthesize_stream, SHORT)


def test_front_end_carries_each_requests_payload_through_loudness_limiter_and_mu_law(tiny):
    from vietvoice_tts_amd.batching import BatchingFrontend
    e = tiny
    texts = [(LONG, 0, dict(watermark_payload=0xBEEF)), (LONG + SHORT, 1, dict(watermark_payload=7)), (LONG, 2, {})]
    old = (e.config.output_encoding, e.config.output_loudness, e.config.output_limiter)
    e.config.output_encoding, e.config.output_loudness, e.config.output_limiter = "ulaw", -20.0, "sample"
    fe = BatchingFrontend(e, max_wait_ms=300.0, max_requests=8)
    try:
        alone = fe.submit(LONG, serial=0, watermark_payload=0xBEEF).result(timeout=300)[0]
        n0 = fe.batches_run
        outs = [f.result(timeout=300)[0] for f in [fe.submit(t, serial=s, **kw) for t, s, kw in texts]]
        assert fe.batches_run == n0 + 1
    finally:
        fe.close()
        e.config.output_encoding, e.config.output_loudness, e.config.output_limiter = old
    assert outs[0].dtype == np.uint8 and np.array_equal(alone, outs[0])               # alone == in a batch with other payloads
    found = e.detect_watermark([wu.ulaw_decode(o) for o in outs])                     # the mu-law decoded here, in the test
    print([(round(r.score, 2), r.offset, r.payload) for r in found])
    assert [(r.present, r.payload, r.offset) for r in found] == [(True, 0xBEEF, 0), (True, 7, 0), (True, 0x1234, 0)]


def test_edit_speech_honours_the_option(tiny):
    ap = _ap()
    e = tiny
    clip = _call(e, e.synthesize, SHORT, key=None)[0]
    dur = clip.size / SR
    parts, fix, text = [(0.3 * dur, 0.5 * dur)], [0.3 * dur], "Xin chào các anh, hôm nay trời đẹp quá."
    base = _call(e, lambda: e.edit_speech(clip, text, parts, fix_duration=fix, seed=11)[0], key=None)
    got = _call(e, lambda: e.edit_speech(clip, text, parts, fix_duration=fix, seed=11)[0])
    assert np.array_equal(got, ap.watermark_embed(base, wu.KEY, 0x1234, 0.2)) and not np.array_equal(got, base)


def test_rows_of_no_samples_and_of_exactly_a_frame_equal_the_mirror(eng):
    """The lengths tests/watermark_util.LENGTHS lacks, 0 and 1024, between the others around a hop and a frame: embedder and detector."""
    ap = _ap()
    lens = (0, 1, 255, 256, 257, 1023, 1024, 1025)
    sigs = [wu.speechlike(n, 300 + n) for n in lens]
    payloads = [(0x1234, 0xBEEF, 0)[k % 3] for k in range(len(sigs))]
    marked = _embed(eng, sigs, payloads, 0.2)
    for x, p, z in zip(sigs, payloads, marked):
        assert z.dtype == np.int16 and np.array_equal(z, ap.watermark_embed(x, wu.KEY, p, 0.2)), x.size
    plane, reqs = pack_requests([[s] for s in marked], gap=5)
    stats, cells, frame_offs = eng.pcm_watermark_detect(_dev(plane), [[xo, n] for ((xo, n),) in reqs], wu.KEY, cells=True)
    stats, cells = stats.cpu().numpy(), cells.cpu().numpy()
    for k, x in enumerate(marked):
        assert np.array_equal(cells[frame_offs[k]: frame_offs[k + 1]], ap.watermark_cells(x)), x.size
        assert np.array_equal(stats[k], ap.watermark_stats(x, wu.KEY)), x.size
