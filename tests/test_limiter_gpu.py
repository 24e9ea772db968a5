"""-m gpu: N13, the look-ahead peak limiter on the device (csrc/vv_limiter.hip).  The yardstick is the host mirror
(core/audio_processor.py: limit_peaks), which the kernels must equal BIT FOR BIT -- stats with ==, PCM with array_equal.  The mirror
itself is held against the scipy reference in tests/test_limiter_cpu.py.  Sample rate 24000 throughout; the look-ahead is 3 samples
where the tile seams and the edges are the subject (short signals, every branch) and the engine's 120 for the lengths around W."""
import numpy as np
import pytest
import torch

from tests.limiter_util import H, noisy
from tests.output_util import lsb_condition, pack_requests

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
SR = 24000
GUARD = 64
SENTINEL = -21846     # 0xAAAA
PEAK = -1.0
TILE = 2048           # vv_pcm_limit_tile(3) == vv_pcm_limit_tile(120)
MODES = ("sample", "true")
LENGTHS = {3: [0, 1, 2, 3, 4, 6, 7, 17, 18, 19, TILE - 1, TILE, TILE + 1, 2 * TILE + 5], 120: [119, 120, 121, 251, 252, 253, 50003]}
SHORT = "Xin chào các bạn, hôm nay trời đẹp quá."
LONG = "Hôm nay trời đẹp quá, chúng ta cùng nhau đi dạo quanh hồ nhé. " * 4


@pytest.fixture(scope="module")
def eng(hip_tiny):
    return hip_tiny["f32"]


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _signal(n, L, seed):
    """A signal that stays under the ceiling for long stretches, with full-scale samples on sample 0, on n - 1, on both sides of every
    tile seam and 2L + H before a seam: wherever an index of the kernel changes its rule."""
    x = noisy(n, seed, scale=2500.0)
    at = [0, n - 1]
    for seam in range(TILE, n, TILE):
        at += [seam - 1, seam, seam - (2 * L + H)]
    for k, i in enumerate(at):
        if 0 <= i < n:
            x[i] = (32767, -32768)[k % 2]
    return x


def _cases(L):
    """[(name, int16 signal, pre-gain)] of one look-ahead."""
    return [(f"L{L}_len{n}", _signal(n, L, 300 + i), (1.0, 1.7, 2.5)[i % 3]) for i, n in enumerate(LENGTHS[L])]


def _mirror(x, mode, gain, L):
    from vietvoice_tts_amd.core.audio_processor import limit_peaks
    y, st = limit_peaks(x, SR, PEAK, mode, gain=gain, L=L)
    return y, np.array([st["g"], st["e_max"], st["s_min"], st["n_limited"]], np.float64)


@pytest.fixture(scope="module")
def cases():
    """{(L, mode): [case]} with the mirror's results, computed once."""
    res = {}
    for L in LENGTHS:
        for mode in MODES:
            res[(L, mode)] = []
            for name, x, g in _cases(L):
                y, st = _mirror(x, mode, g, L)
                res[(L, mode)].append(dict(name=name, x=x, gain=g, y=y, stats=st))
    return res


def _launch(eng, items, mode, L, order=None, odd=3, in_place=False, shift=0, windows=None):
    """One vv_pcm_limit call over ``items`` (in ``order``): sources at odd offsets with junk between, destination between guard bands with
    gaps, its base ``shift`` samples (2 * shift bytes) past an allocation's start.  windows = per item (out_lo, out_n), default the whole.
    -> {name: (pcm of the window, stats row)}."""
    order = list(range(len(items))) if order is None else order
    plane, reqs = pack_requests([[items[i]["x"]] for i in order], gap=odd)
    rows, pos = [], GUARD
    for k, ((so, n),) in enumerate(reqs):
        lo, on = (0, n) if windows is None else windows[k]
        rows.append([so, n, so + lo if in_place else pos, lo, on])
        pos += on + 1 + (len(rows) % 4)                      # every alignment of the destination's 8-byte grid
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
    y, st = eng.pcm_limit(x, rows, SR, PEAK, mode, gain=[items[i]["gain"] for i in order], L=L, out=out, stats=True)
    host, st = y.cpu().numpy(), st.cpu().numpy()
    written = np.zeros(total, bool)
    res = {}
    for k, (i, (_so, _n, do, _lo, on)) in enumerate(zip(order, rows)):
        written[do: do + on] = True
        res[items[i]["name"]] = (host[do: do + on].copy(), st[k].copy())
    untouched = plane if in_place else np.full(total, SENTINEL, np.int16)
    assert np.array_equal(host[~written], untouched[~written]), "a sample outside a request's window was written"
    assert (whole[:shift].cpu().numpy() == SENTINEL).all(), "a sample in front of the destination was written"
    return res


@pytest.fixture(scope="module")
def batches(eng, cases):
    return {key: _launch(eng, items, key[1], key[0]) for key, items in cases.items()}


def test_the_cases_exercise_the_limiter(cases):
    for (L, mode), items in cases.items():
        for c in items:
            n = c["x"].size
            assert c["stats"][3] > 0 or n == 0                                       # every signal is limited somewhere ...
            if n > 40 * (2 * L + H):
                assert c["stats"][3] < n                                             # ... and the long ones have stretches with s == 1
    by = {c["name"]: c for c in cases[(3, "true")]}
    assert by[f"L3_len{2 * TILE + 5}"]["stats"][3] < 2 * TILE and by["L3_len0"]["stats"].tolist() == [1.0, 0.0, 1.0, 0.0]


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("L", [3, 120])
def test_one_launch_equals_the_mirror_bit_for_bit(cases, batches, L, mode):
    for c in cases[(L, mode)]:
        pcm, st = batches[(L, mode)][c["name"]]
        print(c["name"], mode, "device", st.tolist(), "mirror", c["stats"].tolist())
        assert np.all(st == c["stats"]), (c["name"], st.tolist(), c["stats"].tolist())
        assert pcm.dtype == np.int16 and np.array_equal(pcm, c["y"]), (c["name"], int((pcm != c["y"]).sum()))


@pytest.mark.parametrize("L,mode", [(3, "true"), (120, "sample")])
def test_a_request_alone_equals_itself_among_others(eng, cases, batches, L, mode):
    items, batch = cases[(L, mode)], batches[(L, mode)]
    idx = [len(items) - 1, len(items) - 2, 2, 5]
    for i in idx[:2]:                                         # alone, at another source offset
        pcm, st = _launch(eng, items, mode, L, order=[i], odd=9)[items[i]["name"]]
        assert np.array_equal(pcm, batch[items[i]["name"]][0]) and np.all(st == batch[items[i]["name"]][1])
    other = _launch(eng, items, mode, L, order=list(reversed(idx)) + [0, 1], odd=2)  # another index, other neighbours, even offsets
    for i in idx:
        pcm, st = other[items[i]["name"]]
        assert np.array_equal(pcm, batch[items[i]["name"]][0]) and np.all(st == batch[items[i]["name"]][1])


@pytest.mark.parametrize("L,mode", [(3, "sample"), (120, "true")])
def test_in_place_equals_out_of_place(eng, cases, batches, L, mode):
    res = _launch(eng, cases[(L, mode)], mode, L, in_place=True)
    for c in cases[(L, mode)]:
        assert np.array_equal(res[c["name"]][0], c["y"]) and np.all(res[c["name"]][1] == c["stats"]), c["name"]


@pytest.mark.parametrize("shift", [1, 2, 3])
def test_destination_2_4_6_bytes_past_the_8_byte_grid(eng, cases, shift):
    """The apply pass lays its 8-byte stores on the destination's ADDRESS: any 2-byte-aligned base gives the same samples."""
    for in_place in (False, True):
        res = _launch(eng, cases[(3, "true")], "true", 3, shift=shift, in_place=in_place)
        for c in cases[(3, "true")]:
            assert np.array_equal(res[c["name"]][0], c["y"]) and np.all(res[c["name"]][1] == c["stats"]), (c["name"], shift, in_place)


@pytest.mark.parametrize("L,mode", [(3, "true"), (120, "true")])
def test_output_windows_equal_slices_of_the_whole(eng, cases, L, mode):
    """out_lo / out_n: the limiter runs over the whole row, the window alone is written -- and the stats still cover the row."""
    items = cases[(L, mode)]
    W = 2 * L + H
    windows = []
    for k, c in enumerate(items):
        n = c["x"].size
        lo = min(n, (0, 1, W, n // 2, TILE - 1)[k % 5])
        windows.append((lo, (n - lo, max(0, min(n - lo, n // 3)), 0, min(n - lo, 1))[k % 4]))
    for in_place in (False, True):
        res = _launch(eng, items, mode, L, windows=windows, in_place=in_place)
        for c, (lo, on) in zip(items, windows):
            assert np.array_equal(res[c["name"]][0], c["y"][lo: lo + on]) and np.all(res[c["name"]][1] == c["stats"]), (c["name"], lo, on)


def test_a_block_with_context_equals_the_interior_of_the_whole(eng, cases):
    """The stream's mechanism on the device: a block with W samples of context on each side, its interior written."""
    L, mode = 120, "true"
    c = cases[(L, mode)][-1]
    W = 2 * L + H
    a, b = 20000, 26000
    y = eng.pcm_limit(_dev(c["x"][a - W: b + W]), [[0, b - a + 2 * W, 0, W, b - a]], SR, PEAK, mode, gain=c["gain"], L=L)
    assert np.array_equal(y[: b - a].cpu().numpy(), c["y"][a: b])
    from vietvoice_tts_amd.core.audio_processor import LimiterStream, limit_peaks
    x = np.clip(c["x"][:30000].astype(np.float64) * 1.7, -32768, 32767).astype(np.int16)
    ls = LimiterStream(SR, PEAK, mode, backend=eng.limiter_stream_backend(SR, PEAK, mode))
    out = [ls.push(x[i: i + 7001]) for i in range(0, x.size, 7001)] + [ls.flush()]
    assert np.array_equal(np.concatenate(out), limit_peaks(x, SR, PEAK, mode)[0])


def test_pregain_from_a_real_loudness_measurement(eng):
    """meas = the stats of a vv_pcm_loudness measure call, read on the device: equal to the mirror's normalize_loudness(limiter=)."""
    from tests.loudness_util import speechlike
    from vietvoice_tts_amd.core.audio_processor import limit_peaks, normalize_loudness
    xs = [speechlike(30000, SR, seed=61), speechlike(12000, SR, seed=62), np.zeros(12000, np.int16), speechlike(2000, SR, seed=63),
          speechlike(14000, SR, seed=64)]
    xs[0][7000] = 32767
    xs[4][::1500] = -32768
    targets = [-12.0, -30.0, -16.0, -16.0, None]              # loud enough to need the limiter; quiet; nothing kept twice; no target
    plane, reqs = pack_requests([[x] for x in xs], gap=3)
    rows = [[so, n, so] for (so, n), in reqs]
    for mode in MODES:
        buf = _dev(plane)
        _none, meas = eng.pcm_loudness(buf, rows, SR, targets, PEAK, out="measure", stats=True)
        assert _none is None and np.array_equal(buf.cpu().numpy(), plane)             # measure only
        y, st = eng.pcm_limit(buf, rows, SR, PEAK, mode, gain=[1.0, 1.0, 1.0, 1.0, 3.0], meas=meas, targets=targets, out=buf, stats=True)
        host, st, m = y.cpu().numpy(), st.cpu().numpy(), meas.cpu().numpy()
        for k, (x, t, (so, n, _do)) in enumerate(zip(xs, targets, rows)):
            want = normalize_loudness(x, SR, t, PEAK, limiter=mode) if t is not None else limit_peaks(x, SR, PEAK, mode, gain=3.0)[0]
            assert np.array_equal(host[so: so + n], want), (mode, k)
            print(mode, k, "target", t, "measured", m[k].tolist(), "limiter", st[k].tolist())
        assert st[0, 0] > m[0, 3] and st[0, 3] > 0            # uncapped: above the capped gain of N12, and the limiter worked
        assert st[1, 3] == 0 and st[2, 0] == 1.0 and st[3, 0] == 1.0 and st[4, 0] == 3.0
        gaps = np.ones(plane.size, bool)
        for so, n, _do in rows:
            gaps[so: so + n] = False
        assert np.array_equal(host[gaps], plane[gaps])


def _raw(eng, items, mode, L):
    """Device buffers of one call, made ahead of it: -> (call(stream, **overrides), out, stats, rows, buffers)."""
    from vietvoice_tts_amd.core.audio_processor import loudness_ceiling
    plane, reqs = pack_requests([[c["x"]] for c in items], gap=3)
    tile = int(eng.lib.vv_pcm_limit_tile(L))
    rows, pos, samples, tiles = [], GUARD, 0, 0
    for (so, n), in reqs:
        rows.append([so, n, pos, 0, n])
        samples, tiles, pos = samples + n, tiles + -(-n // tile), pos + n + 3
    x = _dev(plane)
    out = torch.full((pos + GUARD,), SENTINEL, dtype=torch.int16, device=DEV)
    rows_h = torch.tensor(rows, dtype=torch.int64)
    rows_d = rows_h.to(DEV)
    par = torch.tensor([[0.0, loudness_ceiling(PEAK), c["gain"]] for c in items], dtype=torch.float64).to(DEV)
    st = torch.zeros((len(items), 4), dtype=torch.float64, device=DEV)
    need = int(eng.lib.vv_pcm_limit_ws_bytes(samples, tiles, len(items)))
    ws = torch.zeros((need // 8 + 1,), dtype=torch.float64, device=DEV)
    win, taps, _tile = eng._limiter_tables(L)

    def call(stream, **kw):
        a = dict(x=x.data_ptr(), n_x=x.numel(), rows=rows_d.data_ptr(), rows_h=rows_h.data_ptr(), R=len(items), L=L, mode=MODES.index(mode),
                 win=win.data_ptr(), taps=taps.data_ptr(), par=par.data_ptr(), meas=None, y=out.data_ptr(), n_y=out.numel(), st=st.data_ptr(),
                 ws=ws.data_ptr(), ws_bytes=ws.numel() * 8)
        a.update(kw)
        return eng.lib.vv_pcm_limit(eng.ctx, a["x"], a["n_x"], a["rows"], a["rows_h"], a["R"], a["L"], a["mode"], a["win"], a["taps"], a["par"],
                                    a["meas"], a["y"], a["n_y"], a["st"], a["ws"], a["ws_bytes"], stream)
    return call, out, st, rows, (x, rows_h, rows_d, par, ws, win, taps)


def test_captured_into_a_graph_equals_eager(eng, cases):
    L, mode = 3, "true"
    items = [c for c in cases[(L, mode)] if c["name"] in (f"L3_len{2 * TILE + 5}", "L3_len0", "L3_len7", f"L3_len{TILE}")]
    call, out, st, rows, _keep = _raw(eng, items, mode, L)
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
    for c, (_so, n, do, _lo, _on) in zip(items, rows):
        assert np.array_equal(host[do: do + n], c["y"]), c["name"]


def test_refusals_launch_nothing_and_leave_the_context_usable(eng, cases):
    L, mode = 3, "true"
    items = [c for c in cases[(L, mode)] if c["name"] in (f"L3_len{TILE + 1}", "L3_len19")]
    call, out, st, rows, (x, rows_h, _rows_d, par, ws, win, taps) = _raw(eng, items, mode, L)
    s = torch.cuda.current_stream().cuda_stream
    variants = {k: rows_h.clone() for k in ("past_x", "past_y", "window", "lo", "neg_src", "neg_n", "neg_dst", "neg_lo", "neg_on")}
    variants["past_x"][1, 1] = x.numel()
    variants["past_y"][1, 2] = out.numel() - 10
    variants["window"][1, 4] += 1                             # out_lo + out_n > n
    variants["lo"][0, 3] = 5
    for col, k in enumerate(("neg_src", "neg_n", "neg_dst", "neg_lo", "neg_on")):
        variants[k][0, col] = -1
    bads = [dict(R=0), dict(L=0), dict(L=1025), dict(mode=2), dict(mode=-1), dict(x=None), dict(rows=None), dict(rows_h=None), dict(win=None),
            dict(taps=None), dict(par=None), dict(st=None), dict(ws=None), dict(x=x.data_ptr() + 1), dict(y=out.data_ptr() + 1),
            dict(st=st.data_ptr() + 4), dict(ws=ws.data_ptr() + 4), dict(win=win.data_ptr() + 4), dict(taps=taps.data_ptr() + 4),
            dict(par=par.data_ptr() + 4), dict(meas=st.data_ptr() + 4), dict(ws_bytes=ws.numel() * 8 - 64), dict(y=x.data_ptr(), n_y=x.numel())]
    bads += [dict(rows_h=v.data_ptr()) for v in variants.values()]
    for bad in bads:
        assert call(s, **bad) == -22, bad
        assert b"vv_pcm_limit" in eng.lib.vv_last_error(eng.ctx)
    torch.cuda.synchronize()
    assert (out.cpu().numpy() == SENTINEL).all() and (st.cpu().numpy() == 0).all()          # nothing was launched
    for bad_rows, kw in (([[0, 10]], {}), ([[0, 10, 0], [20, 10, 5]], {}), ([[x.numel() - 5, 10, 0]], {}), ([[0, 10, 0, 5, 6]], {}),
                         ([[0, 10, 0]], dict(mode="peak")), ([[0, 10, 0]], dict(mode=None)), ([[0, 10, 0]], dict(L=0)), ([[0, 10, 0]], dict(L=1025)),
                         ([[0, 10, 0]], dict(peak_dbfs=1.0)), ([[0, 10, 0]], dict(gain=0.0)), ([[0, 10, 0]], dict(targets=-23.0)),
                         ([[0, 10, 0]], dict(sr=400000, L=None))):
        with pytest.raises(ValueError):
            eng.pcm_limit(x, bad_rows, kw.get("sr", SR), kw.get("peak_dbfs", PEAK), kw.get("mode", "true"), gain=kw.get("gain", 1.0),
                          targets=kw.get("targets"), L=kw.get("L", 3))
    assert call(s) == 0                                       # the context still works
    torch.cuda.synchronize()
    host = out.cpu().numpy()
    for c, (_so, n, do, _lo, _on) in zip(items, rows):
        assert np.array_equal(host[do: do + n], c["y"]), c["name"]
    st.zero_()
    assert call(s, y=None, n_y=0) == 0                        # measure only: stats, no sample written
    torch.cuda.synchronize()
    assert np.array_equal(out.cpu().numpy(), host) and np.all(st.cpu().numpy() == np.stack([c["stats"] for c in items]))


# ------------------------------------------------------------------ engine, tiny preset
def _engine(tmp, **kw):
    from vietvoice_tts_amd.core import ModelConfig, TTSEngine
    kw = {**dict(model_spec="tiny", noise_source="device"), **kw}
    return TTSEngine(ModelConfig(model_cache_dir=str(tmp), synthetic_model=True, nfe_step=5, acoustic_dtype="fp32", max_chunk_duration=8.0, **kw))


def _call(e, fn, *a, stage="host", rate=None, enc="pcm16", loud=None, lim=None, peak=-1.0, **k):
    """One engine call under the given output options, from call serial 0 (the same start noise every time)."""
    c = e.config
    c.output_stage, c.output_sample_rate, c.output_encoding, c.output_loudness, c.output_limiter, c.output_peak_dbfs = stage, rate, enc, loud, lim, peak
    e.model_session_manager.noise_serial = 0
    try:
        r = fn(*a, **k)
        return list(r) if fn == e.synthesize_stream else r
    finally:
        c.output_stage, c.output_sample_rate, c.output_encoding, c.output_loudness, c.output_limiter, c.output_peak_dbfs = "host", None, "pcm16", None, None, -1.0


@pytest.fixture(scope="module")
def tiny(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("limiter_models")
    e = _engine(tmp)
    base = {t: _call(e, e.synthesize, t)[0] for t in (SHORT, LONG)}
    assert len(e._last_plan) >= 3 and base[LONG].dtype == np.int16
    # the ceiling of the engine tests: 6 dB under the largest sample of the plain output, so that the limiter has work
    peak = float(np.clip(20 * np.log10(np.abs(base[LONG].astype(np.int32)).max() / 32767.0) - 6.0, -20.0, -1.0))
    yield e, base, peak
    e.cleanup()


def test_unset_option_never_calls_the_new_entry(tiny, monkeypatch):
    e, base, peak = tiny
    lib, calls = e.model_session_manager.engine.lib, []
    real = lib.vv_pcm_limit
    monkeypatch.setattr(lib, "vv_pcm_limit", lambda *a: calls.append("vv_pcm_limit") or real(*a))
    assert not e._device_output()
    for kw in (dict(), dict(stage="device"), dict(rate=8000, enc="ulaw"), dict(loud=-23.0)):
        _call(e, e.synthesize, LONG, **kw)
    assert np.array_equal(_call(e, e.synthesize, LONG)[0], base[LONG]) and not calls
    e.config.output_limiter = "true"
    try:
        assert e._device_output()                             # the HIP engine takes the device stage when a limiter is set
    finally:
        e.config.output_limiter = None
    _call(e, e.synthesize, LONG, lim="true", peak=peak)
    assert calls == ["vv_pcm_limit"]


@pytest.mark.parametrize("mode", MODES)
def test_engine_equals_the_mirror_on_the_default_output(tiny, mode):
    from vietvoice_tts_amd.core.audio_processor import limit_peaks, lin2ulaw, normalize_loudness, resample_output
    e, base, peak = tiny
    for text in (SHORT, LONG):
        want, st = limit_peaks(base[text], SR, peak, mode)
        got, _ = _call(e, e.synthesize, text, lim=mode, peak=peak)
        print(mode, len(text), "ceiling dBFS", peak, "mirror stats", st)
        assert got.dtype == np.int16 and np.array_equal(got, want)
        assert np.array_equal(_call(e, e.synthesize, text, lim=mode, peak=peak, stage="device")[0], want)      # device stage == default stage
    assert st["n_limited"] > 0 and not np.array_equal(want, base[LONG])
    blocks = _call(e, e.synthesize_stream, LONG, lim=mode, peak=peak)
    assert len(blocks) > 1 and np.array_equal(np.concatenate(blocks), want)            # stream == buffered
    ulaw, _ = _call(e, e.synthesize, LONG, lim=mode, peak=peak, rate=8000, enc="ulaw")
    pcm8, _ = _call(e, e.synthesize, LONG, lim=mode, peak=peak, rate=8000)
    lsb_condition(pcm8, resample_output(want, SR, 8000))      # the rate conversion's own bound (tests/test_output_gpu.py)
    assert np.array_equal(ulaw, lin2ulaw(pcm8))
    assert np.array_equal(np.concatenate(_call(e, e.synthesize_stream, LONG, lim=mode, peak=peak, rate=8000, enc="ulaw")), ulaw)
    loud, _ = _call(e, e.synthesize, LONG, lim=mode, peak=peak, loud=-20.0)           # join -> measure -> uncapped gain -> limiter
    assert np.array_equal(loud, normalize_loudness(base[LONG], SR, -20.0, peak, limiter=mode))
    e.config.output_loudness, e.config.output_limiter = -23.0, mode
    try:
        with pytest.raises(ValueError, match="output_loudness"):
            e.synthesize_stream(LONG)
    finally:
        e.config.output_loudness, e.config.output_limiter = None, None


def test_edit_speech_honours_the_option(tiny):
    from vietvoice_tts_amd.core.audio_processor import limit_peaks
    e, base, peak = tiny
    clip = base[SHORT]
    dur = clip.size / SR
    args = (clip, "Xin chào các anh, hôm nay trời đẹp quá.", [(0.3 * dur, 0.5 * dur)])
    plain, _ = _call(e, e.edit_speech, *args, seed=7)
    pk = float(np.clip(20 * np.log10(np.abs(plain.astype(np.int32)).max() / 32767.0) - 6.0, -20.0, -1.0))
    lim, _ = _call(e, e.edit_speech, *args, seed=7, lim="true", peak=pk)
    assert np.array_equal(lim, limit_peaks(plain, SR, pk, "true")[0]) and not np.array_equal(lim, plain)


def test_front_end_request_with_its_own_limiter(tiny):
    from vietvoice_tts_amd.batching import BatchingFrontend
    from vietvoice_tts_amd.core.audio_processor import limit_peaks
    e, base, peak = tiny
    texts = [(LONG, 0, "true"), (SHORT, 1, None), ("Tạm biệt và hẹn gặp lại.", 2, None)]
    e.config.output_peak_dbfs = peak
    fe = BatchingFrontend(e, max_wait_ms=300.0, max_requests=8)
    try:
        alone = [fe.submit(t, serial=s, limiter=l).result(timeout=300)[0] for t, s, l in texts]
        plain = [fe.submit(t, serial=s).result(timeout=300)[0] for t, s, _l in texts]
        n0 = fe.batches_run
        outs = [f.result(timeout=300)[0] for f in [fe.submit(t, serial=s, limiter=l) for t, s, l in texts]]
        assert fe.batches_run == n0 + 1
    finally:
        fe.close()
        e.config.output_peak_dbfs = -1.0
    for a, o in zip(alone, outs):
        assert o.dtype == np.int16 and np.array_equal(a, o)
    assert np.array_equal(outs[1], plain[1]) and np.array_equal(outs[2], plain[2])          # the plain neighbours are untouched
    assert np.array_equal(plain[0], base[LONG]) and np.array_equal(outs[0], limit_peaks(base[LONG], SR, peak, "true")[0])
