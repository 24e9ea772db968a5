"""-m gpu: N18, the formant-preserving pitch shift on the device (csrc/vv_formant.hip) and its place in the output stage.  The yardstick
is the host mirror (core/audio_processor.py: formant_filters, apply_formant_filters), which the kernels must equal BIT FOR BIT -- the
int16 output and, through h_out, every tap of every frame that is not flat.  What the mirror means is measured in
tests/test_formant_cpu.py."""
import numpy as np
import pytest
import torch

from tests import formant_util as fu
from tests.output_util import lsb_condition, pack_requests

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
    """Every case with the mirror's results, computed once."""
    res = [fu.device_case(*c) for c in fu.DEVICE_CASES]
    assert {c["x"].size for c in res} == {0, 1, 255, 256, 257, 700, 1500, 5000}
    return res


def _launch(eng, items, order=None, odd=3, lead=0):
    """One vv_pcm_formant call over ``items`` (in ``order``): x and y at odd offsets with junk between (``lead`` more samples in front),
    z between guard bands with gaps.  -> {name: (z, taps [M + 1][L])}."""
    order = list(range(len(items))) if order is None else order
    xs, xreq = pack_requests([[items[i]["x"]] for i in order], gap=odd)
    ys, yreq = pack_requests([[items[i]["y"]] for i in order], gap=odd + 2)
    xs, ys = (np.concatenate([np.full(lead, 32767, np.int16), a]) for a in (xs, ys))
    rows, dst = [], GUARD
    for k, (i, ((xo, n),), ((yo, n_f),)) in enumerate(zip(order, xreq, yreq)):
        rows.append([xo + lead, n, yo + lead, n_f, dst, items[i]["tn"], items[i]["td"]])
        dst += n_f + 1 + (k % 4)
    out = torch.full((dst + GUARD,), SENTINEL, dtype=torch.int16, device=DEV)
    z, h, frame_offs = eng.pcm_formant(_dev(xs), _dev(ys), rows, out=out, taps=True)
    host, h = z.cpu().numpy(), h.cpu().numpy()
    written = np.zeros(host.size, bool)
    res = {}
    for k, (i, row) in enumerate(zip(order, rows)):
        written[row[4]: row[4] + row[3]] = True
        res[items[i]["name"]] = (host[row[4]: row[4] + row[3]].copy(), h[frame_offs[k]: frame_offs[k + 1]].copy())
    assert (host[~written] == SENTINEL).all(), "a sample outside a request's output was written"
    return res


def _same(res, items):
    for c in items:
        if c["name"] in res:
            z, h = res[c["name"]]
            assert h.shape == c["h"].shape and np.array_equal(h, c["h"]), (c["name"], np.argwhere(h != c["h"])[:4])
            assert z.dtype == np.int16 and np.array_equal(z, c["z"]), (c["name"], np.nonzero(z != c["z"])[0][:8])


@pytest.fixture(scope="module")
def batch(eng, cases):
    return _launch(eng, cases)


def test_the_cases_exercise_flat_frames_saturation_and_the_filter(cases):
    by = {c["name"]: c for c in cases}
    assert by["zeros"]["flat"].all() and not by["len5000"]["flat"].any()
    assert by["quiet_start"]["flat"].any() and not by["quiet_start"]["flat"].all()    # flat frames next to live ones
    assert (np.abs(by["square"]["z"].astype(np.int32)) >= 32767).any()               # the clamp is reached
    assert by["constant"]["flat"].any()
    assert sum(not np.array_equal(c["z"], c["y"]) for c in cases) >= 10              # the filter changes the signal
    assert by["len0"]["h"].shape == (1, fu.L) and by["len5000_up"]["h"].shape == (-(-5000 // fu.H) + 1, fu.L)


def test_one_launch_equals_the_mirror_bit_for_bit(cases, batch):
    assert len(batch) == len(cases)
    _same(batch, cases)


def test_a_request_alone_and_elsewhere_equals_itself_in_the_batch(eng, cases, batch):
    by = {c["name"]: i for i, c in enumerate(cases)}
    pick = [by[n] for n in ("len5000", "len700", "quiet_start_fast", "len257")]       # ragged, at odd offsets
    four = _launch(eng, cases, order=pick, odd=5)
    _same(four, cases)
    for i in pick:
        alone = _launch(eng, cases, order=[i], odd=9)
        name = cases[i]["name"]
        assert np.array_equal(alone[name][0], four[name][0]) and np.array_equal(alone[name][1], four[name][1])
        assert np.array_equal(alone[name][0], batch[name][0]) and np.array_equal(alone[name][1], batch[name][1])
    moved = _launch(eng, cases, order=[pick[0]], odd=2, lead=4321)                    # elsewhere in a larger buffer
    assert np.array_equal(moved["len5000"][0], batch["len5000"][0]) and np.array_equal(moved["len5000"][1], batch["len5000"][1])


def _raw(eng, items):
    """Device buffers of one call, made ahead of it: -> (call(stream, **overrides), z, rows, buffers)."""
    wa, g = eng._formant_tables
    win = eng._wsola_window
    xs, xreq = pack_requests([[c["x"]] for c in items], gap=3)
    ys, yreq = pack_requests([[c["y"]] for c in items], gap=5)
    rows, dst, frames = [], GUARD, 0
    for c, ((xo, n),), ((yo, n_f),) in zip(items, xreq, yreq):
        rows.append([xo, n, yo, n_f, dst, c["tn"], c["td"]])
        dst, frames = dst + n_f + 3, frames + c["h"].shape[0]
    x, y = _dev(xs), _dev(ys)
    z = torch.full((dst + GUARD,), SENTINEL, dtype=torch.int16, device=DEV)
    h = torch.full((frames * fu.L,), -7.0, dtype=torch.float64, device=DEV)
    rows_h = torch.tensor(rows, dtype=torch.int64)
    rows_d = rows_h.to(DEV)
    ws = torch.zeros((int(eng.lib.vv_pcm_formant_ws_bytes(frames, len(items))) // 8 + 1,), dtype=torch.int64, device=DEV)

    def call(stream, **kw):
        a = dict(x=x.data_ptr(), n_x=x.numel(), y=y.data_ptr(), n_y=y.numel(), rows=rows_d.data_ptr(), rows_h=rows_h.data_ptr(), R=len(items),
                 wa=wa.data_ptr(), g=g.data_ptr(), win=win.data_ptr(), z=z.data_ptr(), n_z=z.numel(), h=h.data_ptr(), n_h=h.numel(),
                 ws=ws.data_ptr(), ws_bytes=ws.numel() * 8)
        a.update(kw)
        return eng.lib.vv_pcm_formant(eng.ctx, a["x"], a["n_x"], a["y"], a["n_y"], a["rows"], a["rows_h"], a["R"], a["wa"], a["g"], a["win"], a["z"],
                                      a["n_z"], a["h"], a["n_h"], a["ws"], a["ws_bytes"], stream)
    return call, z, h, rows, (x, y, rows_h, rows_d, ws, wa, g, win)


def _check_raw(items, rows, z, h=None):
    host = z.cpu().numpy()
    for c, row in zip(items, rows):
        assert np.array_equal(host[row[4]: row[4] + row[3]], c["z"]), c["name"]
    if h is not None:
        assert np.array_equal(h.cpu().numpy().reshape(-1, fu.L), np.concatenate([c["h"] for c in items]))


def test_captured_into_a_graph_equals_eager(eng, cases):
    items = [c for c in cases if c["name"] in ("len1500", "len0", "quiet_start_fast", "len257")]
    call, z, h, rows, _keep = _raw(eng, items)
    assert call(torch.cuda.current_stream().cuda_stream) == 0
    torch.cuda.synchronize()
    eager = z.clone()
    _check_raw(items, rows, z, h)
    z.fill_(SENTINEL)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        assert call(torch.cuda.current_stream().cuda_stream) == 0          # no synchronisation, no host read-back: capturable
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(z, eager)


def test_refusals_launch_nothing_and_leave_the_context_usable(eng, cases):
    items = [c for c in cases if c["name"] in ("len700", "len257")]
    call, z, h, rows, (x, y, rows_h, _rows_d, ws, wa, g, win) = _raw(eng, items)
    s = torch.cuda.current_stream().cuda_stream
    variants = {k: rows_h.clone() for k in ("past_x", "past_y", "past_z", "on_z", "n_f", "tn_0", "td_0", "tn_big", "td_big", "neg_x", "neg_n", "neg_y",
                                            "neg_nf", "neg_z")}
    variants["past_x"][1, 0] = x.numel() - 10
    variants["past_y"][1, 2] = y.numel() - 10
    variants["past_z"][1, 4] = z.numel() - 10
    variants["on_z"][1, 4] = variants["on_z"][0, 4] + 10                              # rows overlapping on z
    variants["n_f"][0, 3] += 1                                                        # not ceil(n td / tn)
    variants["tn_0"][0, 5] = 0
    variants["td_0"][0, 6] = 0
    variants["tn_big"][0, 5] = 2049
    variants["td_big"][0, 6] = 2049
    for col, k in ((0, "neg_x"), (1, "neg_n"), (2, "neg_y"), (3, "neg_nf"), (4, "neg_z")):
        variants[k][0, col] = -1
    bads = [dict(R=0), dict(R=-1), dict(R=65536), dict(x=None), dict(y=None), dict(rows=None), dict(rows_h=None), dict(wa=None), dict(g=None),
            dict(win=None), dict(z=None), dict(ws=None), dict(x=x.data_ptr() + 1), dict(y=y.data_ptr() + 1), dict(z=z.data_ptr() + 1),
            dict(h=h.data_ptr() + 4), dict(ws=ws.data_ptr() + 4), dict(wa=wa.data_ptr() + 4), dict(ws_bytes=ws.numel() * 8 - 4096), dict(ws_bytes=0),
            dict(n_h=h.numel() - 1), dict(z=x.data_ptr(), n_z=x.numel()), dict(z=y.data_ptr(), n_z=y.numel()),
            dict(z=y.data_ptr() + 2 * (y.numel() - 8), n_z=z.numel()), dict(n_z=500), dict(n_x=100), dict(n_y=100)]
    bads += [dict(rows_h=v.data_ptr()) for v in variants.values()]
    for bad in bads:
        assert call(s, **bad) == -22, bad
        assert b"vv_pcm_formant" in eng.lib.vv_last_error(eng.ctx)
    torch.cuda.synchronize()
    assert (z.cpu().numpy() == SENTINEL).all() and (h.cpu().numpy() == -7.0).all()    # nothing was launched
    for bad_rows in ([[0, 10, 0, 10, 0, 1]], [[0, 10, 0, 11, 0, 1, 1]], [[x.numel() - 5, 10, 0, 10, 0, 1, 1]], [[0, 10, 0, 10, -1, 1, 1]],
                     [[0, 10, 0, 10, 0, 0, 1]], [[0, 300, 0, 300, 0, 1, 1], [300, 300, 300, 300, 299, 1, 1]], []):
        with pytest.raises(ValueError):
            eng.pcm_formant(x, y, bad_rows)
    with pytest.raises(ValueError):
        eng.pcm_formant(x, y, [[0, 10, 0, 10, 0, 1, 1]], out=y)                       # not in place
    assert call(s, h=None, n_h=0) == 0                                                # h_out is optional; the context still works
    torch.cuda.synchronize()
    _check_raw(items, rows, z)
    assert (h.cpu().numpy() == -7.0).all()


# ------------------------------------------------------------------ PcmStage.finish_output
def _counted(monkeypatch, lib):
    calls, real = [], lib.vv_pcm_formant
    monkeypatch.setattr(lib, "vv_pcm_formant", lambda *a: calls.append("vv_pcm_formant") or real(*a))
    return calls


@pytest.fixture(scope="module")
def three():
    """Three requests of one chunk each (the join copies a single chunk untouched): the plane and the plans of finish_output."""
    sigs = [fu.speechy(5000, 71), fu.speechy(3000, 72), fu.speechy(2000, 73)]
    plane, reqs = pack_requests([[s] for s in sigs], gap=7)
    return sigs, plane, reqs


def test_finish_output_shift_and_unset_are_todays_bytes(eng, three, monkeypatch):
    _sigs, plane, reqs = three
    calls = _counted(monkeypatch, eng.lib)
    pcm = _dev(plane)
    opts = dict(pitch=[4, None, None], tempo=[None, 1.25, None])
    today = eng.finish_output(pcm, reqs, 0.1, SR, **opts)
    for kw in (dict(formants="shift"), dict(formants=None), dict(formants=["shift", "shift", None])):
        got = eng.finish_output(pcm, reqs, 0.1, SR, **opts, **kw)
        assert all(np.array_equal(a, b) for a, b in zip(got, today)) and not calls
    plain = eng.finish_output(pcm, reqs, 0.1, SR)
    kept = eng.finish_output(pcm, reqs, 0.1, SR, formants="keep")                     # "keep" without a pitch anywhere: nothing new runs
    assert all(np.array_equal(a, b) for a, b in zip(kept, plain)) and not calls
    kept = eng.finish_output(pcm, reqs, 0.1, SR, tempo=1.25, formants="keep")         # tempo alone
    assert all(np.array_equal(a, b) for a, b in zip(kept, eng.finish_output(pcm, reqs, 0.1, SR, tempo=1.25))) and not calls
    for bad in ("hold", ["keep", "keep"], [1, 2, 3]):
        with pytest.raises(ValueError):
            eng.finish_output(pcm, reqs, 0.1, SR, **opts, formants=bad)


def test_finish_output_keep_on_a_mixed_batch_equals_the_mirror_chain(eng, three, monkeypatch):
    from vietvoice_tts_amd.core.audio_processor import encode_output, keep_formants, lin2ulaw, normalize_loudness, resample_output
    sigs, plane, reqs = three
    calls = _counted(monkeypatch, eng.lib)
    pcm = _dev(plane)
    opts = dict(pitch=[4, None, None], tempo=[None, 1.25, None])
    shifted = eng.finish_output(pcm, reqs, 0.1, SR, **opts)                           # the device's own converted signal is the filter's input
    want0 = keep_formants(sigs[0], shifted[0], 1, 1)
    assert not np.array_equal(want0, shifted[0]) and not calls
    for kw in (dict(formants="keep"), dict(formants=["keep", "shift", None])):
        got = eng.finish_output(pcm, reqs, 0.1, SR, **opts, **kw)
        assert np.array_equal(got[0], want0) and np.array_equal(got[1], shifted[1]) and np.array_equal(got[2], shifted[2])
    assert calls == ["vv_pcm_formant"] * 2
    both = eng.finish_output(pcm, reqs[:1], 0.1, SR, pitch=-3, tempo=0.75, formants="keep")[0]      # stretched, converted, then corrected
    assert np.array_equal(both, keep_formants(sigs[0], eng.finish_output(pcm, reqs[:1], 0.1, SR, pitch=-3, tempo=0.75)[0], 3, 4))
    direct = eng.finish_output(pcm, reqs[:1], 0.1, SR, pitch=12, tempo=2.0, formants="keep")[0]     # the stretch cancels: converted from the joined signal
    assert np.array_equal(direct, keep_formants(sigs[0], eng.finish_output(pcm, reqs[:1], 0.1, SR, pitch=12, tempo=2.0)[0], 2, 1))
    # with loudness, limiter, output rate, G.711 and FLAC behind it: levels and ceiling are those of the corrected signal
    peak = -3.0
    chain = dict(loudness=-20.0, limiter="true", peak_dbfs=peak)
    loud0 = normalize_loudness(want0, SR, -20.0, peak, limiter="true")
    got = eng.finish_output(pcm, reqs, 0.1, SR, **opts, **chain, formants="keep")
    assert np.array_equal(got[0], loud0) and not np.array_equal(loud0, want0)
    assert np.array_equal(got[1], normalize_loudness(shifted[1], SR, -20.0, peak, limiter="true"))
    pcm8 = eng.finish_output(pcm, reqs, 0.1, SR, 8000, **opts, **chain, formants="keep")[0]
    lsb_condition(pcm8, resample_output(loud0, SR, 8000))
    assert np.array_equal(eng.finish_output(pcm, reqs, 0.1, SR, 8000, "ulaw", **opts, **chain, formants="keep")[0], lin2ulaw(pcm8))
    flac = eng.finish_output(pcm, reqs, 0.1, SR, None, "flac", **opts, **chain, formants="keep")[0]
    assert np.array_equal(flac, encode_output(loud0, "flac", SR))


# ------------------------------------------------------------------ engine, tiny preset
_PLAIN = dict(output_stage="host", output_pitch=None, output_tempo=None, output_formants="shift")


def _call(e, fn, *a, pitch=None, tempo=None, formants="shift", **k):
    """One engine call under the given output options, from call serial 0 (the same start noise every time)."""
    e.config.output_pitch, e.config.output_tempo, e.config.output_formants = pitch, tempo, formants
    e.model_session_manager.noise_serial = 0
    try:
        return fn(*a, **k)
    finally:
        for key, v in _PLAIN.items():
            setattr(e.config, key, v)


@pytest.fixture(scope="module")
def tiny(tmp_path_factory):
    from vietvoice_tts_amd.core import ModelConfig, TTSEngine
    tmp = tmp_path_factory.mktemp("formant_models")
    e = TTSEngine(ModelConfig(model_cache_dir=str(tmp), synthetic_model=True, nfe_step=5, acoustic_dtype="fp32", max_chunk_duration=8.0,
                              model_spec="tiny", noise_source="device", output_pitch=4, output_formants="keep"))
    assert e.config.output_formants == "keep" and e._device_output()
    built_with = _call(e, e.synthesize, LONG, pitch=4, formants="keep")[0]            # the options the engine was built with
    base = {t: _call(e, e.synthesize, t)[0] for t in (SHORT, LONG)}
    yield e, base, built_with
    e.cleanup()


def test_engine_keep_equals_the_mirror_on_its_own_joined_pcm(tiny, monkeypatch):
    from vietvoice_tts_amd.core.audio_processor import keep_formants
    e, base, built_with = tiny
    calls = _counted(monkeypatch, e.model_session_manager.engine.lib)
    for text in (SHORT, LONG):                                # one chunk and several
        shifted, _ = _call(e, e.synthesize, text, pitch=4)
        assert not calls
        got, _ = _call(e, e.synthesize, text, pitch=4, formants="keep")
        assert calls == ["vv_pcm_formant"]
        calls.clear()
        assert got.dtype == np.int16 and got.size == base[text].size
        assert np.array_equal(got, keep_formants(base[text], shifted, 1, 1)) and not np.array_equal(got, shifted)
    assert np.array_equal(built_with, got)
    assert np.array_equal(_call(e, e.synthesize, SHORT, formants="keep")[0], base[SHORT]) and not calls      # no pitch: nothing new
    fast, _ = _call(e, e.synthesize, SHORT, pitch=-3, tempo=1.25, formants="keep")
    assert np.array_equal(fast, keep_formants(base[SHORT], _call(e, e.synthesize, SHORT, pitch=-3, tempo=1.25)[0], 5, 4))
    with pytest.raises(ValueError, match="output_pitch"):
        _call(e, e.synthesize_stream, SHORT, pitch=4, formants="keep")


def test_front_end_request_with_keep_alone_equals_itself_in_a_mixed_batch(tiny):
    from vietvoice_tts_amd.batching import BatchingFrontend
    from vietvoice_tts_amd.core.audio_processor import keep_formants
    e, base, _built_with = tiny
    texts = [(LONG, 0, dict(pitch=4, formants="keep")), (SHORT, 1, dict(pitch=4)), ("Tạm biệt và hẹn gặp lại.", 2, {})]
    fe = BatchingFrontend(e, max_wait_ms=300.0, max_requests=8)
    try:
        alone = [fe.submit(t, serial=s, **kw).result(timeout=300)[0] for t, s, kw in texts]
        n0 = fe.batches_run
        outs = [f.result(timeout=300)[0] for f in [fe.submit(t, serial=s, **kw) for t, s, kw in texts]]
        assert fe.batches_run == n0 + 1
        shifted = fe.submit(LONG, serial=0, pitch=4).result(timeout=300)[0]
    finally:
        fe.close()
    for a, o in zip(alone, outs):
        assert o.dtype == np.int16 and np.array_equal(a, o)                           # alone == in a batch with a shifted and a plain request
    assert np.array_equal(outs[0], keep_formants(base[LONG], shifted, 1, 1))          # the output stage, given equal input: exact
    assert not np.array_equal(outs[0], shifted)


def test_rows_at_the_edges_of_an_analysis_frame_equal_the_mirror(eng):
    """x, and y alone, of one sample less than, equal to and one more than an analysis frame of NA samples, in one call."""
    items = [fu.device_case(*c) for c in fu.FRAME_EDGE_CASES]
    assert {1023, 1024, 1025} <= {c["x"].size for c in items} and {1023, 1024, 1025} <= {c["y"].size for c in items}
    res = _launch(eng, items)
    assert len(res) == len(items)
    _same(res, items)
