"""-m gpu: N12, loudness normalisation on the device (csrc/vv_loudness.hip).  The yardstick is the host mirror
(core/audio_processor.py: normalize_loudness), which the kernels must equal BIT FOR BIT -- stats with ==, PCM with array_equal; the
mirror itself and the device are also held against the sequential scipy reference of tests/loudness_util.py under the bounds of
tests/test_loudness_cpu.py (zbar relative 1e-9, PCM output_util.lsb_condition).  Sample rate 24000 throughout."""
import numpy as np
import pytest
import torch

from tests.loudness_util import ref_normalize, speechlike, threshold_margin
from tests.output_util import lsb_condition, pack_requests

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
SR = 24000
GUARD = 64
SENTINEL = -21846     # 0xAAAA
LENGTHS = [0, 1, 127, 128, 2399, 2400, 2401, 9599, 9600, 9601, 12000, 50003]
PEAK = -1.0
SHORT = "Xin chào các bạn, hôm nay trời đẹp quá."
LONG = "Hôm nay trời đẹp quá, chúng ta cùng nhau đi dạo quanh hồ nhé. " * 4


@pytest.fixture(scope="module")
def eng(hip_tiny):
    return hip_tiny["f32"]


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _cases():
    """[(name, int16 signal, target or None)]: the gated signals of every length, then the special requests."""
    out = [(f"len{n}", speechlike(n, SR, seed=100 + i), -23.0) for i, n in enumerate(LENGTHS)]
    out.append(("zeros", np.zeros(12000, np.int16), -23.0))
    out.append(("noise3", np.random.default_rng(5).integers(-3, 4, 12000).astype(np.int16), -23.0))       # 3 LSB: below the absolute gate
    quiet = speechlike(24000, SR, seed=41, amp=600.0)
    quiet[5000:5003] = 4000                                  # a click on a quiet clip: the gain to -16 LUFS would push it past the ceiling
    out.append(("quiet_ceiling", quiet, -16.0))
    lone = speechlike(12000, SR, seed=42)
    lone[777] = -32768
    out.append(("lone_min", lone, -23.0))
    out.append(("measure_only", speechlike(12000, SR, seed=43), None))
    # sound, then 2 s of exact zeros (padded output): the filter's free decay runs down into float64 denormals; held against the mirror
    # bit for bit like every case (the silent blocks are gated, so zbar and the PCM also stay inside the reference's bounds)
    out.append(("loud_then_zeros", np.concatenate([speechlike(12000, SR, seed=44), np.zeros(48000, np.int16)]), -23.0))
    return out


@pytest.fixture(scope="module")
def cases():
    """The cases with their reference (scipy) and mirror results, computed once."""
    from vietvoice_tts_amd.core.audio_processor import loudness_ceiling, loudness_gain, loudness_target, measure_loudness, normalize_loudness
    res = []
    for name, x, target in _cases():
        ref_y, m, g, limited = ref_normalize(x, SR, target, PEAK)
        _L, zbar, kept, peak = measure_loudness(x, SR)
        gain = loudness_gain(zbar, kept, peak, loudness_target(target), loudness_ceiling(PEAK))
        res.append(dict(name=name, x=x, target=target, ref_y=ref_y, ref=m, ref_g=g, limited=limited,
                        stats=np.array([zbar, kept, peak, gain], np.float64), y=normalize_loudness(x, SR, target, PEAK)))
    return res


def _launch(eng, items, order=None, odd=3, in_place=False, shift=0):
    """One vv_pcm_loudness call over ``items`` (in ``order``): sources at odd offsets with junk between, destination between guard bands
    with gaps, its base ``shift`` samples (2 * shift bytes) past an allocation's start.  -> {name: (pcm, stats row)}."""
    order = list(range(len(items))) if order is None else order
    plane, reqs = pack_requests([[items[i]["x"]] for i in order], gap=odd)
    rows, pos = [], GUARD
    for (so, n), in reqs:
        rows.append([so, n, so if in_place else pos])
        pos += n + 1 + (len(rows) % 4)                       # every alignment of the destination's 8-byte grid
    if in_place:
        whole = _dev(np.concatenate([np.full(shift, SENTINEL, np.int16), plane]))
        x = out = whole[shift:]
        total = plane.size
    else:
        x = _dev(plane)
        total = pos + GUARD
        whole = torch.full((total + shift,), SENTINEL, dtype=torch.int16, device=DEV)
        out = whole[shift:]
    assert out.data_ptr() % 8 == (2 * shift) % 8
    y, st = eng.pcm_loudness(x, rows, SR, [items[i]["target"] for i in order], PEAK, out=out, stats=True)
    host, st = y.cpu().numpy(), st.cpu().numpy()
    written = np.zeros(total, bool)
    res = {}
    for k, (i, (_so, n, do)) in enumerate(zip(order, rows)):
        written[do: do + n] = True
        res[items[i]["name"]] = (host[do: do + n].copy(), st[k].copy())
    untouched = plane if in_place else np.full(total, SENTINEL, np.int16)
    assert np.array_equal(host[~written], untouched[~written]), "a sample outside a request's slice was written"
    assert (whole[:shift].cpu().numpy() == SENTINEL).all(), "a sample in front of the destination was written"
    return res


def test_reference_side_of_the_cases(cases):
    """What the cases are meant to exercise holds on the reference side, away from every threshold."""
    by = {c["name"]: c for c in cases}
    dropped = 0
    for c in cases:
        m = c["ref"]
        if m["kept"]:
            margin = threshold_margin(m)
            print(c["name"], "blocks", m["z"].size, "kept", m["kept"], "margin", margin, "lufs", m["lufs"], "gain", c["ref_g"], c["limited"])
            assert margin >= 1e-3, (c["name"], margin)
            dropped += int(((m["z"] > m["thresholds"][0]) & ~m["keep"]).sum())
    assert dropped >= 1                                       # the relative gate drops a block somewhere
    assert by["len50003"]["ref"]["kept"] < by["len50003"]["ref"]["z"].size
    assert by["quiet_ceiling"]["limited"] and by["lone_min"]["limited"] and by["lone_min"]["ref"]["peak"] == 32768
    assert not by["len12000"]["limited"] and not by["len50003"]["limited"]
    assert by["zeros"]["ref"]["kept"] == 0 and by["noise3"]["ref"]["kept"] == 0 and by["noise3"]["ref"]["z"].size > 0
    assert all(by[f"len{n}"]["ref"]["kept"] == 0 for n in LENGTHS if n < 9600) and by["len9600"]["ref"]["kept"] == 1
    for c in cases:                                           # the mirror agrees with the reference on every case
        assert c["stats"][1] == c["ref"]["kept"] and c["stats"][2] == c["ref"]["peak"]
        assert abs(c["stats"][0] - c["ref"]["zbar"]) <= 1e-9 * c["ref"]["zbar"]
        lsb_condition(c["y"], c["ref_y"])


@pytest.fixture(scope="module")
def batch(eng, cases):
    return _launch(eng, cases)


def test_one_launch_equals_the_mirror_bit_for_bit(cases, batch):
    for c in cases:
        pcm, st = batch[c["name"]]
        print(c["name"], "device", st.tolist(), "mirror", c["stats"].tolist())
        assert np.all(st == c["stats"]), (c["name"], st.tolist(), c["stats"].tolist())
        assert pcm.dtype == np.int16 and np.array_equal(pcm, c["y"]), (c["name"], int((pcm != c["y"]).sum()))
        if c["target"] is None or c["stats"][1] == 0:
            assert st[3] == 1.0 and np.array_equal(pcm, c["x"])          # gain exactly 1: copied through


def test_one_launch_against_the_scipy_reference(cases, batch):
    for c in cases:
        pcm, st = batch[c["name"]]
        assert st[1] == c["ref"]["kept"] and st[2] == c["ref"]["peak"]
        assert abs(st[0] - c["ref"]["zbar"]) <= 1e-9 * c["ref"]["zbar"], (c["name"], st[0], c["ref"]["zbar"])
        n_diff = lsb_condition(pcm, c["ref_y"])
        print(c["name"], "zbar", st[0], "reference", c["ref"]["zbar"], "samples differing", n_diff)


def test_a_request_alone_equals_itself_among_others(eng, cases, batch):
    names = ["len50003", "len9601", "quiet_ceiling", "len2401"]
    idx = [i for i, c in enumerate(cases) if c["name"] in names]
    for i in idx:                                             # alone, at another source offset
        pcm, st = _launch(eng, cases, order=[i], odd=9)[cases[i]["name"]]
        want_pcm, want_st = batch[cases[i]["name"]]
        assert torch.equal(torch.from_numpy(st), torch.from_numpy(want_st)) and torch.equal(torch.from_numpy(pcm), torch.from_numpy(want_pcm))
    other = _launch(eng, cases, order=list(reversed(idx)) + [0, 13, 5], odd=2)      # another index, other neighbours, even offsets
    for i in idx:
        pcm, st = other[cases[i]["name"]]
        want_pcm, want_st = batch[cases[i]["name"]]
        assert torch.equal(torch.from_numpy(st), torch.from_numpy(want_st)) and torch.equal(torch.from_numpy(pcm), torch.from_numpy(want_pcm))


def test_in_place_equals_out_of_place(eng, cases, batch):
    res = _launch(eng, cases, in_place=True)
    for c in cases:
        assert np.array_equal(res[c["name"]][0], batch[c["name"]][0]) and np.all(res[c["name"]][1] == batch[c["name"]][1]), c["name"]


@pytest.mark.parametrize("shift", [1, 2, 3])
def test_destination_2_4_6_bytes_past_the_8_byte_grid(eng, cases, batch, shift):
    """The apply pass lays its 8-byte stores on the destination's ADDRESS: any 2-byte-aligned base gives the same samples."""
    for in_place in (False, True):
        res = _launch(eng, cases, shift=shift, in_place=in_place)
        for c in cases:
            assert np.array_equal(res[c["name"]][0], c["y"]) and np.all(res[c["name"]][1] == c["stats"]), (c["name"], shift, in_place)


def _raw(eng, items, peak=PEAK):
    """Device buffers of one call, made ahead of it: -> (call(stream), out, stats, rows)."""
    from vietvoice_tts_amd.core.audio_processor import loudness_ceiling, loudness_target
    from vietvoice_tts_amd.runtime import LOUD_RUN
    plane, reqs = pack_requests([[c["x"]] for c in items], gap=3)
    sub = SR // 10
    rps = -(-sub // LOUD_RUN)
    rows, pos, runs = [], GUARD, 0
    for (so, n), in reqs:
        rows.append([so, n, pos, runs])
        runs += (n // sub) * rps + -(-(n % sub) // LOUD_RUN)
        pos += n + 3
    x = _dev(plane)
    out = torch.full((pos + GUARD,), SENTINEL, dtype=torch.int16, device=DEV)
    rows_h = torch.tensor(rows, dtype=torch.int64)
    rows_d = rows_h.to(DEV)
    par = torch.tensor([[loudness_target(c["target"]), loudness_ceiling(peak)] for c in items], dtype=torch.float64).to(DEV)
    st = torch.zeros((len(items), 4), dtype=torch.float64, device=DEV)
    need = int(eng.lib.vv_pcm_loudness_ws_bytes(runs, len(items)))
    ws = torch.zeros((need // 8 + 1,), dtype=torch.float64, device=DEV)
    tab = eng._loudness_tables(SR)
    keep = (x, rows_h, rows_d, par, ws, tab)

    def call(stream, **kw):
        a = dict(x=x.data_ptr(), n_x=x.numel(), rows=rows_d.data_ptr(), rows_h=rows_h.data_ptr(), R=len(items), sub=sub, tab=tab.data_ptr(),
                 par=par.data_ptr(), y=out.data_ptr(), n_y=out.numel(), st=st.data_ptr(), ws=ws.data_ptr(), ws_bytes=ws.numel() * 8)
        a.update(kw)
        return eng.lib.vv_pcm_loudness(eng.ctx, a["x"], a["n_x"], a["rows"], a["rows_h"], a["R"], a["sub"], a["tab"], a["par"], a["y"], a["n_y"],
                                       a["st"], a["ws"], a["ws_bytes"], stream)
    return call, out, st, rows, keep


def test_captured_into_a_graph_equals_eager(eng, cases):
    items = [c for c in cases if c["name"] in ("len50003", "len2401", "quiet_ceiling", "measure_only", "len0")]
    call, out, st, rows, _keep = _raw(eng, items)
    assert call(torch.cuda.current_stream().cuda_stream) == 0
    torch.cuda.synchronize()
    eager_out, eager_st = out.clone(), st.clone()
    out.fill_(SENTINEL)
    st.zero_()
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        assert call(torch.cuda.current_stream().cuda_stream) == 0          # no synchronisation, no host read-back: capturable
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(out, eager_out) and torch.equal(st, eager_st)
    host = out.cpu().numpy()
    for c, (_so, n, do, _ro) in zip(items, rows):
        assert np.array_equal(host[do: do + n], c["y"]), c["name"]


def test_refusals_launch_nothing_and_leave_the_context_usable(eng, cases):
    items = [c for c in cases if c["name"] in ("len9601", "len2401")]
    call, out, st, rows, (x, rows_h, _rows_d, _par, ws, _tab) = _raw(eng, items)
    s = torch.cuda.current_stream().cuda_stream
    past_x, past_y, bad_run, neg = rows_h.clone(), rows_h.clone(), rows_h.clone(), rows_h.clone()
    past_x[1, 1] = x.numel()
    past_y[1, 2] = out.numel() - 10
    bad_run[1, 3] += 1
    neg[0, 0] = -1
    for bad in (dict(sub=127), dict(R=0), dict(x=None), dict(rows=None), dict(rows_h=None), dict(tab=None), dict(par=None), dict(st=None),
                dict(ws=None), dict(x=x.data_ptr() + 1), dict(y=out.data_ptr() + 1), dict(st=st.data_ptr() + 4), dict(ws=ws.data_ptr() + 4),
                dict(ws_bytes=ws.numel() * 8 - 64), dict(rows_h=past_x.data_ptr()), dict(rows_h=past_y.data_ptr()),
                dict(rows_h=bad_run.data_ptr()), dict(rows_h=neg.data_ptr()), dict(y=x.data_ptr(), n_y=x.numel())):
        assert call(s, **bad) == -22, bad
        assert b"vv_pcm_loudness" in eng.lib.vv_last_error(eng.ctx)
    torch.cuda.synchronize()
    assert (out.cpu().numpy() == SENTINEL).all() and (st.cpu().numpy() == 0).all()          # nothing was launched
    for bad_rows, kw in (([[0, 10]], {}), ([[0, 10, 0], [20, 10, 5]], {}), ([[x.numel() - 5, 10, 0]], {}), ([[0, 10, 0]], dict(targets=-70.0)),
                         ([[0, 10, 0]], dict(sr=22055)), ([[0, 10, 0]], dict(peak_dbfs=1.0))):
        with pytest.raises(ValueError):
            eng.pcm_loudness(x, bad_rows, kw.get("sr", SR), kw.get("targets", -23.0), kw.get("peak_dbfs", PEAK))
    assert call(s) == 0                                       # the context still works
    torch.cuda.synchronize()
    host = out.cpu().numpy()
    for c, (_so, n, do, _ro) in zip(items, rows):
        assert np.array_equal(host[do: do + n], c["y"]), c["name"]
    assert call(s, y=None, n_y=0) == 0                        # measure only: stats, no sample written
    torch.cuda.synchronize()
    assert np.array_equal(out.cpu().numpy(), host) and np.all(st.cpu().numpy() == np.stack([c["stats"] for c in items]))


# ------------------------------------------------------------------ engine, tiny preset
def _engine(tmp, **kw):
    from vietvoice_tts_amd.core import ModelConfig, TTSEngine
    kw = {**dict(model_spec="tiny", noise_source="device"), **kw}
    return TTSEngine(ModelConfig(model_cache_dir=str(tmp), synthetic_model=True, nfe_step=5, acoustic_dtype="fp32", max_chunk_duration=8.0, **kw))


def _call(e, fn, *a, stage="host", rate=None, enc="pcm16", loud=None, **k):
    """One engine call under the given output options, from call serial 0 (the same start noise every time)."""
    c = e.config
    c.output_stage, c.output_sample_rate, c.output_encoding, c.output_loudness = stage, rate, enc, loud
    e.model_session_manager.noise_serial = 0
    try:
        return fn(*a, **k)
    finally:
        c.output_stage, c.output_sample_rate, c.output_encoding, c.output_loudness = "host", None, "pcm16", None


@pytest.fixture(scope="module")
def tiny(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("loudness_models")
    e = _engine(tmp)
    base = {t: _call(e, e.synthesize, t)[0] for t in (SHORT, LONG)}
    assert len(e._last_plan) >= 3 and base[LONG].dtype == np.int16
    yield e, base
    e.cleanup()


def test_unset_option_never_calls_the_new_entry(tiny, monkeypatch):
    e, base = tiny
    lib, calls = e.model_session_manager.engine.lib, []
    real = lib.vv_pcm_loudness
    monkeypatch.setattr(lib, "vv_pcm_loudness", lambda *a: calls.append("vv_pcm_loudness") or real(*a))
    assert not e._device_output()
    for kw in (dict(), dict(stage="device"), dict(rate=8000, enc="ulaw")):
        _call(e, e.synthesize, LONG, **kw)
    assert not calls
    e.config.output_loudness = -23.0
    try:
        assert e._device_output()                             # the HIP engine takes the device stage when a loudness is set
    finally:
        e.config.output_loudness = None
    _call(e, e.synthesize, LONG, loud=-23.0)
    assert calls == ["vv_pcm_loudness"]


@pytest.mark.parametrize("text", [SHORT, LONG])
def test_engine_equals_the_mirror_on_the_default_output(tiny, text):
    from vietvoice_tts_amd.core.audio_processor import lin2ulaw, measure_loudness, normalize_loudness, resample_output
    e, base = tiny
    want = normalize_loudness(base[text], SR, -23.0, -1.0)
    got, _ = _call(e, e.synthesize, text, loud=-23.0)
    assert got.dtype == np.int16 and np.array_equal(got, want)
    assert np.array_equal(_call(e, e.synthesize, text, loud=-23.0, stage="device")[0], want)
    ulaw, _ = _call(e, e.synthesize, text, loud=-23.0, rate=8000, enc="ulaw")
    host8 = resample_output(want, SR, 8000)
    pcm8, _ = _call(e, e.synthesize, text, loud=-23.0, rate=8000)
    lsb_condition(pcm8, host8)                                # the rate conversion's own bound (tests/test_output_gpu.py)
    assert np.array_equal(ulaw, lin2ulaw(pcm8))
    # re-measured: the request is neither ceiling-limited nor empty on the reference side, so it sits at the target
    _y, m, g, limited = ref_normalize(base[text], SR, -23.0, -1.0)
    assert m["kept"] > 0 and not limited
    L = measure_loudness(got, SR)[0]
    print(len(text), "re-measured", L, "gain", g, "before", m["lufs"])
    assert abs(L + 23.0) <= 0.01
    e.config.output_loudness = -23.0
    try:
        with pytest.raises(ValueError, match="output_loudness"):
            e.synthesize_stream(text)                 # at the call, not at the first block
    finally:
        e.config.output_loudness = None


def test_edit_speech_honours_the_option(tiny):
    from vietvoice_tts_amd.core.audio_processor import normalize_loudness
    e, base = tiny
    clip = base[SHORT]
    dur = clip.size / SR
    args = (clip, "Xin chào các anh, hôm nay trời đẹp quá.", [(0.3 * dur, 0.5 * dur)])
    plain, _ = _call(e, e.edit_speech, *args, seed=7)
    loud, _ = _call(e, e.edit_speech, *args, seed=7, loud=-20.0)
    assert np.array_equal(loud, normalize_loudness(plain, SR, -20.0, -1.0)) and not np.array_equal(loud, plain)
    assert np.array_equal(_call(e, e.edit_speech, *args, seed=7, loud=-20.0, stage="device")[0], loud)


def test_front_end_request_with_its_own_loudness(tiny):
    from vietvoice_tts_amd.batching import BatchingFrontend
    from vietvoice_tts_amd.core.audio_processor import normalize_loudness
    e, base = tiny
    texts = [(LONG, 0, -18.0), (SHORT, 1, None), ("Tạm biệt và hẹn gặp lại.", 2, None)]
    fe = BatchingFrontend(e, max_wait_ms=300.0, max_requests=8)
    try:
        alone = [fe.submit(t, serial=s, loudness=l).result(timeout=300)[0] for t, s, l in texts]
        plain = [fe.submit(t, serial=s).result(timeout=300)[0] for t, s, _l in texts]
        n0 = fe.batches_run
        outs = [f.result(timeout=300)[0] for f in [fe.submit(t, serial=s, loudness=l) for t, s, l in texts]]
        assert fe.batches_run == n0 + 1
    finally:
        fe.close()
    for a, o in zip(alone, outs):
        assert o.dtype == np.int16 and np.array_equal(a, o)
    assert np.array_equal(outs[1], plain[1]) and np.array_equal(outs[2], plain[2])          # the plain neighbours are untouched
    assert np.array_equal(plain[0], base[LONG]) and np.array_equal(outs[0], normalize_loudness(base[LONG], SR, -18.0, -1.0))
