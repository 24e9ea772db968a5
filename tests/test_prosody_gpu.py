"""-m gpu: N14, the WSOLA time stretch on the device (csrc/vv_prosody.hip) and the prosody step of the output stage.  The yardstick is
the host mirror (core/audio_processor.py: time_stretch, shift_prosody), which the kernels must equal BIT FOR BIT -- frame positions and
PCM with array_equal.  The mirror itself is held against an independent loop reference in tests/test_prosody_cpu.py."""
import numpy as np
import pytest
import torch

from tests.output_util import lsb_condition, pack_requests
from tests.prosody_util import HS, LENGTHS, RATIOS, stretch_cases

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
SR = 24000
GUARD = 64
SENTINEL = -21846     # 0xAAAA
SHORT = "Xin chào các bạn, hôm nay trời đẹp quá."
LONG = "Hôm nay trời đẹp quá, chúng ta cùng nhau đi dạo quanh hồ nhé. " * 4


@pytest.fixture(scope="module")
def eng(hip_tiny):
    return hip_tiny["f32"]


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


@pytest.fixture(scope="module")
def cases():
    """Every length under every ratio with the mirror's results, computed once."""
    from vietvoice_tts_amd.core.audio_processor import time_stretch
    res = []
    for name, x, p, q in stretch_cases():
        y, pos = time_stretch(x, p, q)
        res.append(dict(name=name, x=x, p=p, q=q, y=y, pos=pos))
    assert len(res) == len(LENGTHS) * len(RATIOS) + 2
    return res


def _launch(eng, items, order=None, odd=3, shift=0):
    """One vv_pcm_stretch call over ``items`` (in ``order``): sources at odd offsets with junk between, destination between guard bands
    with gaps, its base ``shift`` samples (2 * shift bytes) past an allocation's start.  -> {name: (pcm, pos)}."""
    order = list(range(len(items))) if order is None else order
    plane, reqs = pack_requests([[items[i]["x"]] for i in order], gap=odd)
    rows, dst = [], GUARD
    for k, (i, ((so, n),)) in enumerate(zip(order, reqs)):
        rows.append([so, n, dst, items[i]["p"], items[i]["q"]])
        dst += items[i]["y"].size + 1 + (k % 4)              # every alignment of the destination's 8-byte grid
    total = dst + GUARD
    whole = torch.full((total + shift,), SENTINEL, dtype=torch.int16, device=DEV)
    out = whole[shift:]
    assert out.data_ptr() % 8 == (2 * shift) % 8
    y, pos, pos_offs = eng.pcm_stretch(_dev(plane), rows, out=out)
    host, pos = y.cpu().numpy(), pos.cpu().numpy()
    written = np.zeros(total, bool)
    res = {}
    for k, (i, (_so, _n, do, _p, _q)) in enumerate(zip(order, rows)):
        n_s = items[i]["y"].size
        written[do: do + n_s] = True
        res[items[i]["name"]] = (host[do: do + n_s].copy(), pos[pos_offs[k]: pos_offs[k + 1]].copy())
    assert (host[~written] == SENTINEL).all(), "a sample outside a request's output was written"
    assert (whole[:shift].cpu().numpy() == SENTINEL).all(), "a sample in front of the destination was written"
    return res


def _same(res, items):
    for c in items:
        if c["name"] in res:
            y, pos = res[c["name"]]
            assert pos.dtype == np.int32 and np.array_equal(pos, c["pos"]), c["name"]
            assert y.size == -(-c["x"].size * c["p"] // c["q"]) and np.array_equal(y, c["y"]), c["name"]


@pytest.fixture(scope="module")
def batch(eng, cases):
    return _launch(eng, cases)


def test_the_cases_exercise_the_search(cases):
    moved = [c for c in cases if c["pos"].size > 2 and any(c["pos"][m] != (m - 1) * HS * c["q"] // c["p"] for m in range(1, c["pos"].size))]
    assert len(moved) > len(cases) // 2                      # the search leaves the nominal positions on most signals
    assert any(c["pos"].size == 1 for c in cases) and max(c["pos"].size for c in cases) == -(-5003 * 2 // HS) + 1


def test_one_launch_equals_the_mirror_bit_for_bit(cases, batch):
    assert len(batch) == len(cases)
    _same(batch, cases)


def test_a_request_alone_equals_itself_among_others(eng, cases, batch):
    by = {c["name"]: i for i, c in enumerate(cases)}
    pick = [by[n] for n in ("len5003_25over21", "len1000_2over3", "len513_32over31", "len0_3over2", "len5003_1over2", "len257_2over1")]
    other = _launch(eng, cases, order=pick[::-1], odd=2)                              # other neighbours, another index and offset
    alone = _launch(eng, cases, order=[pick[0]], odd=9)
    _same(other, cases)
    _same(alone, cases)
    for name in other:
        assert np.array_equal(other[name][0], batch[name][0]) and np.array_equal(other[name][1], batch[name][1])
    name = cases[pick[0]]["name"]
    assert np.array_equal(alone[name][0], batch[name][0]) and np.array_equal(alone[name][1], batch[name][1])


@pytest.mark.parametrize("shift", [1, 2, 3])
def test_destination_2_4_6_bytes_past_the_8_byte_grid(eng, cases, shift):
    items = cases[shift::5]
    _same(_launch(eng, items, shift=shift), items)


def _raw(eng, items):
    """Device buffers of one call, made ahead of it: -> (call(stream, **overrides), out, pos, rows, buffers)."""
    eng.pcm_stretch(_dev(np.zeros(600, np.int16)), [[0, 600, 0, 3, 2]])              # the window table is on the device
    plane, reqs = pack_requests([[c["x"]] for c in items], gap=3)
    rows, dst, po = [], GUARD, 0
    for c, ((so, n),) in zip(items, reqs):
        rows.append([so, n, dst, c["p"], c["q"], po])
        dst, po = dst + c["y"].size + 3, po + c["pos"].size
    x = _dev(plane)
    out = torch.full((dst + GUARD,), SENTINEL, dtype=torch.int16, device=DEV)
    pos = torch.full((po,), -7, dtype=torch.int32, device=DEV)
    rows_h = torch.tensor(rows, dtype=torch.int64)
    rows_d = rows_h.to(DEV)
    ws = torch.zeros((int(eng.lib.vv_pcm_stretch_ws_bytes(len(items))) // 8 + 1,), dtype=torch.int64, device=DEV)
    win = eng._wsola_window

    def call(stream, **kw):
        a = dict(x=x.data_ptr(), n_x=x.numel(), rows=rows_d.data_ptr(), rows_h=rows_h.data_ptr(), R=len(items), win=win.data_ptr(),
                 y=out.data_ptr(), n_y=out.numel(), pos=pos.data_ptr(), n_pos=pos.numel(), ws=ws.data_ptr(), ws_bytes=ws.numel() * 8)
        a.update(kw)
        return eng.lib.vv_pcm_stretch(eng.ctx, a["x"], a["n_x"], a["rows"], a["rows_h"], a["R"], a["win"], a["y"], a["n_y"], a["pos"], a["n_pos"],
                                      a["ws"], a["ws_bytes"], stream)
    return call, out, pos, rows, (x, rows_h, rows_d, ws, win)


def _check_raw(items, rows, out, pos):
    host, hpos = out.cpu().numpy(), pos.cpu().numpy()
    for c, (_so, _n, do, _p, _q, po) in zip(items, rows):
        assert np.array_equal(host[do: do + c["y"].size], c["y"]) and np.array_equal(hpos[po: po + c["pos"].size], c["pos"]), c["name"]


def test_captured_into_a_graph_equals_eager(eng, cases):
    items = [c for c in cases if c["name"] in ("len5003_3over2", "len0_2over3", "len767_23over29", "len1000_1over2")]
    call, out, pos, rows, _keep = _raw(eng, items)
    assert call(torch.cuda.current_stream().cuda_stream) == 0
    torch.cuda.synchronize()
    eager_out, eager_pos = out.clone(), pos.clone()
    out.fill_(SENTINEL)
    pos.fill_(-7)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        assert call(torch.cuda.current_stream().cuda_stream) == 0          # no synchronisation, no host read-back: capturable
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(out, eager_out) and torch.equal(pos, eager_pos)
    _check_raw(items, rows, out, pos)


def test_refusals_launch_nothing_and_leave_the_context_usable(eng, cases):
    items = [c for c in cases if c["name"] in ("len1000_3over2", "len513_2over3")]
    call, out, pos, rows, (x, rows_h, _rows_d, ws, win) = _raw(eng, items)
    s = torch.cuda.current_stream().cuda_stream
    variants = {k: rows_h.clone() for k in ("past_x", "past_y", "past_pos", "on_y", "on_pos", "p_eq_q", "p_0", "q_0", "p_big", "q_big", "slow",
                                            "fast", "neg_src", "neg_n", "neg_dst", "neg_pos")}
    variants["past_x"][1, 1] = x.numel()
    variants["past_y"][1, 2] = out.numel() - 10
    variants["past_pos"][1, 5] = pos.numel() - 1
    variants["on_y"][1, 2] = variants["on_y"][0, 2] + 10                              # rows overlapping on y
    variants["on_pos"][1, 5] = 0
    variants["p_eq_q"][0, 3:5] = torch.tensor([7, 7])
    variants["p_0"][0, 3] = 0
    variants["q_0"][0, 4] = 0
    variants["p_big"][0, 3:5] = torch.tensor([2049, 1024])
    variants["q_big"][0, 3:5] = torch.tensor([1024, 2049])
    variants["slow"][0, 3:5] = torch.tensor([9, 2])                                   # p / q > 4
    variants["fast"][0, 3:5] = torch.tensor([2, 9])                                   # p / q < 1 / 4
    for col, k in ((0, "neg_src"), (1, "neg_n"), (2, "neg_dst"), (5, "neg_pos")):
        variants[k][0, col] = -1
    bads = [dict(R=0), dict(R=-1), dict(x=None), dict(rows=None), dict(rows_h=None), dict(win=None), dict(pos=None), dict(ws=None),
            dict(x=x.data_ptr() + 1), dict(y=out.data_ptr() + 1), dict(pos=pos.data_ptr() + 2), dict(ws=ws.data_ptr() + 4),
            dict(win=win.data_ptr() + 4), dict(ws_bytes=ws.numel() * 8 - 24), dict(ws_bytes=0), dict(y=x.data_ptr(), n_y=x.numel()),
            dict(n_y=500), dict(n_pos=3)]
    bads += [dict(rows_h=v.data_ptr()) for v in variants.values()]
    for bad in bads:
        assert call(s, **bad) == -22, bad
        assert b"vv_pcm_stretch" in eng.lib.vv_last_error(eng.ctx)
    torch.cuda.synchronize()
    assert (out.cpu().numpy() == SENTINEL).all() and (pos.cpu().numpy() == -7).all()  # nothing was launched
    for bad_rows in ([[0, 10, 0, 3]], [[0, 10, 0, 3, 2], [20, 10, 5, 3, 2]], [[x.numel() - 5, 10, 0, 3, 2]], [[0, 10, 0, 5, 5]], [[0, 10, 0, 1, 5]],
                     [[0, 10, 0, 4096, 2048]], [[0, 10, -1, 3, 2]], []):
        with pytest.raises(ValueError):
            eng.pcm_stretch(x, bad_rows)
    with pytest.raises(ValueError):
        eng.pcm_stretch(x, [[0, 10, 0, 3, 2]], out=x)                                 # not in place
    assert call(s, y=None, n_y=0) == 0                                                # the search alone: positions, no sample written
    torch.cuda.synchronize()
    hpos = pos.cpu().numpy()
    assert (out.cpu().numpy() == SENTINEL).all() and all(np.array_equal(hpos[r[5]: r[5] + c["pos"].size], c["pos"]) for c, r in zip(items, rows))
    pos.fill_(-7)
    assert call(s) == 0                                                               # the context still works
    torch.cuda.synchronize()
    _check_raw(items, rows, out, pos)
    _none, only_pos, offs = eng.pcm_stretch(x, [r[:5] for r in rows], out="positions")
    assert _none is None and np.array_equal(only_pos.cpu().numpy()[offs[1]: offs[2]], items[1]["pos"])


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
        return fn(*a, **k)
    finally:
        for key, v in _PLAIN.items():
            setattr(e.config, key, v)


@pytest.fixture(scope="module")
def tiny(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("prosody_models")
    e = _engine(tmp)
    base = {t: _call(e, e.synthesize, t)[0] for t in (SHORT, LONG)}
    assert len(e._last_plan) >= 3 and base[LONG].dtype == np.int16
    yield e, base
    e.cleanup()


def test_unset_options_never_call_the_new_entry(tiny, monkeypatch):
    e, base = tiny
    lib, calls = e.model_session_manager.engine.lib, []
    real = lib.vv_pcm_stretch
    monkeypatch.setattr(lib, "vv_pcm_stretch", lambda *a: calls.append("vv_pcm_stretch") or real(*a))
    assert not e._device_output()
    for kw in (dict(), dict(stage="device"), dict(rate=8000, enc="ulaw"), dict(loud=-23.0), dict(lim="true")):
        _call(e, e.synthesize, LONG, **kw)
    assert np.array_equal(_call(e, e.synthesize, LONG)[0], base[LONG]) and not calls
    assert np.array_equal(_call(e, e.synthesize, LONG, stage="device")[0], base[LONG]) and not calls
    for key in ("output_pitch", "output_tempo"):
        setattr(e.config, key, 1.5)
        try:
            assert e._device_output()                         # the HIP engine takes the device stage when either option is set
        finally:
            setattr(e.config, key, None)
    _call(e, e.synthesize, LONG, tempo=1.25)
    assert calls == ["vv_pcm_stretch"]
    with pytest.raises(ValueError, match="output_tempo"):
        _call(e, e.synthesize_stream, LONG, tempo=1.25)


def test_engine_tempo_equals_the_mirror_exactly(tiny):
    from vietvoice_tts_amd.core.audio_processor import shift_prosody
    e, base = tiny
    for text in (SHORT, LONG):                                # one chunk and several
        want = shift_prosody(base[text], None, 1.25)
        got, _ = _call(e, e.synthesize, text, tempo=1.25)
        assert got.dtype == np.int16 and want.size == -(-base[text].size * 4 // 5) and np.array_equal(got, want)
    slow, _ = _call(e, e.synthesize, SHORT, tempo=0.8)
    assert np.array_equal(slow, shift_prosody(base[SHORT], None, 0.8)) and slow.size == -(-base[SHORT].size * 5 // 4)


def test_engine_pitch_is_held_to_the_resampler_bound(tiny):
    from vietvoice_tts_amd.core.audio_processor import shift_prosody
    e, base = tiny
    for text in (SHORT, LONG):
        got, _ = _call(e, e.synthesize, text, pitch=3)
        want = shift_prosody(base[text], 3, None)
        assert got.size == base[text].size                    # tempo 1: the length stays
        print("pitch 3", len(text), "samples differing by 1 LSB:", lsb_condition(got, want))      # N10's bound: 1 LSB, <= 1 sample in 10^4
    both, _ = _call(e, e.synthesize, LONG, pitch=-4, tempo=1.5)
    lsb_condition(both, shift_prosody(base[LONG], -4, 1.5))
    octave, _ = _call(e, e.synthesize, SHORT, pitch=12, tempo=2.0)                    # the stretch cancels: the rate conversion alone
    lsb_condition(octave, shift_prosody(base[SHORT], 12, 2.0))


def test_engine_chain_with_loudness_and_limiter_equals_the_mirror_chain(tiny):
    from vietvoice_tts_amd.core.audio_processor import lin2ulaw, normalize_loudness, resample_output, shift_prosody
    e, base = tiny
    stretched = shift_prosody(base[LONG], None, 1.25)
    peak = float(np.clip(20 * np.log10(np.abs(stretched.astype(np.int32)).max() / 32767.0) - 6.0, -20.0, -1.0))
    want = normalize_loudness(stretched, SR, -20.0, peak, limiter="true")             # levels and ceiling of what is heard
    got, _ = _call(e, e.synthesize, LONG, tempo=1.25, loud=-20.0, lim="true", peak=peak)
    assert np.array_equal(got, want) and not np.array_equal(want, stretched)
    assert np.array_equal(_call(e, e.synthesize, LONG, tempo=1.25, loud=-20.0, peak=peak)[0], normalize_loudness(stretched, SR, -20.0, peak))
    pcm8, _ = _call(e, e.synthesize, LONG, tempo=1.25, loud=-20.0, lim="true", peak=peak, rate=8000)
    lsb_condition(pcm8, resample_output(want, SR, 8000))
    assert np.array_equal(_call(e, e.synthesize, LONG, tempo=1.25, loud=-20.0, lim="true", peak=peak, rate=8000, enc="ulaw")[0], lin2ulaw(pcm8))


def test_edit_speech_honours_the_options(tiny):
    from vietvoice_tts_amd.core.audio_processor import shift_prosody
    e, base = tiny
    clip = base[SHORT]
    dur = clip.size / SR
    args = (clip, "Xin chào các anh, hôm nay trời đẹp quá.", [(0.3 * dur, 0.5 * dur)])
    plain, _ = _call(e, e.edit_speech, *args, seed=7)
    fast, _ = _call(e, e.edit_speech, *args, seed=7, tempo=1.5)
    assert np.array_equal(fast, shift_prosody(plain, None, 1.5)) and fast.size == -(-plain.size * 2 // 3)
    high, _ = _call(e, e.edit_speech, *args, seed=7, pitch=2)
    lsb_condition(high, shift_prosody(plain, 2, None))


def test_front_end_request_with_its_own_pitch(tiny):
    from vietvoice_tts_amd.batching import BatchingFrontend
    from vietvoice_tts_amd.core.audio_processor import shift_prosody
    e, base = tiny
    texts = [(LONG, 0, dict(pitch=3)), (SHORT, 1, {}), ("Tạm biệt và hẹn gặp lại.", 2, {})]
    fe = BatchingFrontend(e, max_wait_ms=300.0, max_requests=8)
    try:
        alone = [fe.submit(t, serial=s, **kw).result(timeout=300)[0] for t, s, kw in texts]
        plain = [fe.submit(t, serial=s).result(timeout=300)[0] for t, s, _kw in texts]
        n0 = fe.batches_run
        outs = [f.result(timeout=300)[0] for f in [fe.submit(t, serial=s, **kw) for t, s, kw in texts]]
        assert fe.batches_run == n0 + 1
        tempo = fe.submit(LONG, serial=0, tempo=1.25).result(timeout=300)[0]
    finally:
        fe.close()
    for a, o in zip(alone, outs):
        assert o.dtype == np.int16 and np.array_equal(a, o)                           # alone == in a batch with two plain requests
    assert np.array_equal(outs[1], plain[1]) and np.array_equal(outs[2], plain[2])    # the plain neighbours: bit-equal to today's output
    assert np.array_equal(plain[0], base[LONG]) and outs[0].size == base[LONG].size
    lsb_condition(outs[0], shift_prosody(base[LONG], 3, None))
    assert np.array_equal(tempo, shift_prosody(base[LONG], None, 1.25))
