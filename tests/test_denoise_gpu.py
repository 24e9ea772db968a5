"""-m gpu: N19, the vocoder-bias denoiser on the device (csrc/vv_denoise.hip) and its place in the output stage.  The yardstick is the host
mirror (core/audio_processor.py: denoise_pcm, denoise_bias), which the kernels must equal BIT FOR BIT -- the int16 output, through mag_out
every magnitude of every frame, and all 513 float64 of a bias.  What the mirror means is measured in tests/test_denoise_cpu.py."""
import numpy as np
import pytest
import torch

from tests import denoise_util as du
from tests.output_util import lsb_condition, pack_requests

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
SR = 24000
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


@pytest.fixture(scope="module")
def biases():
    """Two non-trivial random positive profiles, host and device."""
    b = np.stack([du.random_bias(21), du.random_bias(22, 20000.0)])
    return b, _dev(b)


def _launch(eng, sigs, strengths, bias_rows, bias_d, gap=3, lead=0):
    """One vv_pcm_denoise call: the signals at offsets that are no multiple of the hop with junk between, y between guard samples of 0x5555
    with gaps.  -> [(z, mag [M + 3][N])] per signal; asserts that nothing outside the spans was written."""
    plane, reqs = pack_requests([[s] for s in sigs], gap=gap)
    plane = np.concatenate([np.full(lead, 32767, np.int16), plane])
    rows, dst = [], GUARD + 1
    for k, (((xo, n),), b) in enumerate(zip(reqs, bias_rows)):
        rows.append([xo + lead, n, dst, b])
        dst += n + 1 + (k % 4)
    out = torch.full((dst + GUARD,), SENTINEL, dtype=torch.int16, device=DEV)
    y, mag, frame_offs = eng.pcm_denoise(_dev(plane), rows, strengths, bias_d, out=out, mags=True)
    host, mag = y.cpu().numpy(), mag.cpu().numpy()
    written = np.zeros(host.size, bool)
    res = []
    for k, row in enumerate(rows):
        written[row[2]: row[2] + row[1]] = True
        res.append((host[row[2]: row[2] + row[1]].copy(), mag[frame_offs[k]: frame_offs[k + 1]].copy()))
    assert (host[~written] == SENTINEL).all(), "a sample outside a request's output was written"
    return res


@pytest.mark.parametrize("strength", (0.25, 1.0))
def test_one_launch_equals_the_mirror_bit_for_bit(eng, biases, strength):
    ap = _ap()
    bias, bias_d = biases
    sigs = [du.speechlike(n, 300 + n) for n in du.LENGTHS]
    rows_b = [k % 2 for k in range(len(sigs))]
    got = _launch(eng, sigs, strength, rows_b, bias_d)
    changed = 0
    for x, b, (z, mag) in zip(sigs, rows_b, got):
        want, want_mag = ap.denoise_pcm(x, bias[b], strength, mags=True)
        assert mag.shape == want_mag.shape == (du.frames_of(x.size), du.N)
        assert np.array_equal(mag, want_mag), (x.size, np.argwhere(mag != want_mag)[:4])
        assert z.dtype == np.int16 and np.array_equal(z, want), (x.size, np.nonzero(z != want)[0][:8])
        changed += int(not np.array_equal(z, x))
    assert changed >= len(sigs) - 1                                                   # the subtraction acts (one sample may survive it)


@pytest.mark.parametrize("n", (1024, 1280, 5000))
def test_the_bias_of_a_signal_equals_the_mirror_bit_for_bit(eng, n):
    ap = _ap()
    x = du.speechlike(n, 500 + n)
    plane = np.concatenate([np.full(5, 32767, np.int16), x, np.full(3, 32767, np.int16)])
    got = eng.pcm_denoise_bias(_dev(plane), [[5, n]]).cpu().numpy()
    want = ap.denoise_bias(x)
    assert got.shape == (1, du.BINS) and got.dtype == np.float64 and np.array_equal(got[0], want), np.nonzero(got[0] != want)[0][:8]
    two = eng.pcm_denoise_bias(_dev(plane), [[5, n], [5, 1024]]).cpu().numpy()        # two rows in one call, ragged
    assert np.array_equal(two[0], want) and np.array_equal(two[1], ap.denoise_bias(x[:1024]))


def test_strength_zero_gives_the_input_back_through_the_kernels(eng, biases):
    _bias, bias_d = biases
    sigs = [du.noise(5000, 9), du.alternation(5000)]
    for s, b in ((0.0, bias_d), (1.0, torch.zeros_like(bias_d))):                     # strength 0, and an all-zero bias
        got = _launch(eng, sigs, s, [0, 1], b)
        for x, (z, mag) in zip(sigs, got):
            assert np.array_equal(z, x) and mag.any()                                 # computed: the magnitudes are there


def test_a_request_in_a_batch_equals_itself_alone(eng, biases):
    ap = _ap()
    bias, bias_d = biases
    sigs = [du.speechlike(n, 700 + n) for n in (1, 257, 1024, 3000, 5000)]
    strengths, rows_b = [0.5, 2.0, 1.0, 0.25, 16.0], [0, 1, 1, 0, 1]
    batch = _launch(eng, sigs, strengths, rows_b, bias_d, gap=7)
    for k, x in enumerate(sigs):
        alone = _launch(eng, [x], [strengths[k]], [rows_b[k]], bias_d, gap=1, lead=4321 if k == 4 else 0)[0]
        assert np.array_equal(alone[0], batch[k][0]) and np.array_equal(alone[1], batch[k][1]), x.size
        assert np.array_equal(batch[k][0], ap.denoise_pcm(x, bias[rows_b[k]], strengths[k]))


def _raw(eng, bias_d):
    """Device buffers of one two-row call, made ahead of it: -> (call(stream, **overrides), y, mag, rows, sigs, buffers)."""
    window, tw = eng._denoise_tables
    sigs = [du.speechlike(700, 41), du.speechlike(257, 42)]
    plane, reqs = pack_requests([[s] for s in sigs], gap=3)
    rows, dst = [], GUARD
    for ((xo, n),), b in zip(reqs, (0, 1)):
        rows.append([xo, n, dst, b])
        dst += n + 3
    x = _dev(plane)
    y = torch.full((dst + GUARD,), SENTINEL, dtype=torch.int16, device=DEV)
    frames = sum(du.frames_of(s.size) for s in sigs)
    mag = torch.full((frames * du.N,), -7.0, dtype=torch.float64, device=DEV)
    rows_h = torch.tensor(rows, dtype=torch.int64)
    rows_d = rows_h.to(DEV)
    s_h = torch.tensor([0.5, 1.0], dtype=torch.float64)
    s_d = s_h.to(DEV)
    ws = torch.zeros((int(eng.lib.vv_pcm_denoise_ws_bytes(2)) // 8 + 1,), dtype=torch.int64, device=DEV)

    def call(stream, **kw):
        a = dict(x=x.data_ptr(), n_x=x.numel(), rows=rows_d.data_ptr(), rows_h=rows_h.data_ptr(), R=2, s=s_d.data_ptr(), s_h=s_h.data_ptr(),
                 bias=bias_d.data_ptr(), n_bias=2, win=window.data_ptr(), tw=tw.data_ptr(), y=y.data_ptr(), n_y=y.numel(), mag=mag.data_ptr(),
                 n_mag=mag.numel(), ws=ws.data_ptr(), ws_bytes=ws.numel() * 8)
        a.update(kw)
        return eng.lib.vv_pcm_denoise(eng.ctx, a["x"], a["n_x"], a["rows"], a["rows_h"], a["R"], a["s"], a["s_h"], a["bias"], a["n_bias"], a["win"],
                                      a["tw"], a["y"], a["n_y"], a["mag"], a["n_mag"], a["ws"], a["ws_bytes"], stream)
    return call, y, mag, rows, sigs, (x, rows_h, rows_d, s_h, s_d, ws, window, tw)


def test_refusals_launch_nothing_and_leave_the_context_usable(eng, biases):
    ap = _ap()
    bias, bias_d = biases
    call, y, mag, rows, sigs, (x, rows_h, _rows_d, s_h, _s_d, ws, window, tw) = _raw(eng, bias_d)
    s = torch.cuda.current_stream().cuda_stream
    variants = {k: rows_h.clone() for k in ("past_x", "past_y", "on_y", "bias_row", "neg_x", "neg_n", "neg_y", "neg_b", "big_n")}
    variants["past_x"][1, 0] = x.numel() - 10
    variants["past_y"][1, 2] = y.numel() - 10
    variants["on_y"][1, 2] = variants["on_y"][0, 2] + 10                              # rows overlapping on y
    variants["bias_row"][0, 3] = 2
    variants["big_n"][0, 1] = (1 << 30) + 1
    for col, k in ((0, "neg_x"), (1, "neg_n"), (2, "neg_y"), (3, "neg_b")):
        variants[k][0, col] = -1
    bad_s = [torch.tensor(v, dtype=torch.float64) for v in ([-0.5, 1.0], [0.5, 16.5], [float("nan"), 1.0], [0.5, float("inf")])]
    bads = [dict(R=0), dict(R=-1), dict(R=65536), dict(x=None), dict(rows=None), dict(rows_h=None), dict(s=None), dict(s_h=None), dict(bias=None),
            dict(win=None), dict(tw=None), dict(y=None), dict(ws=None), dict(x=x.data_ptr() + 1), dict(y=y.data_ptr() + 1), dict(mag=mag.data_ptr() + 4),
            dict(ws=ws.data_ptr() + 4), dict(win=window.data_ptr() + 4), dict(tw=tw.data_ptr() + 4), dict(bias=bias_d.data_ptr() + 4),
            dict(ws_bytes=8), dict(ws_bytes=0), dict(n_mag=mag.numel() - 1), dict(n_bias=0), dict(n_bias=1), dict(y=x.data_ptr(), n_y=x.numel()),
            dict(y=x.data_ptr() + 2 * (x.numel() - 8), n_y=y.numel()), dict(n_y=500), dict(n_x=100)]
    bads += [dict(rows_h=v.data_ptr()) for v in variants.values()] + [dict(s_h=v.data_ptr()) for v in bad_s]
    for bad in bads:
        assert call(s, **bad) == -22, bad
        assert b"vv_pcm_denoise" in eng.lib.vv_last_error(eng.ctx)
    out = torch.full((3,), 1.0, dtype=torch.float64, device=DEV)
    bw = torch.zeros((int(eng.lib.vv_pcm_denoise_bias_ws_bytes(1, 1)) // 8 + 1,), dtype=torch.int64, device=DEV)
    short = torch.tensor([[0, 1023, 0, 0]], dtype=torch.int64)
    assert eng.lib.vv_pcm_denoise_bias(eng.ctx, x.data_ptr(), x.numel(), short.to(DEV).data_ptr(), short.data_ptr(), 1, window.data_ptr(), tw.data_ptr(),
                                       out.data_ptr(), du.BINS, bw.data_ptr(), bw.numel() * 8, s) == -22      # no full frame
    torch.cuda.synchronize()
    assert (y.cpu().numpy() == SENTINEL).all() and (mag.cpu().numpy() == -7.0).all() and (out.cpu().numpy() == 1.0).all()      # nothing was launched
    for bad_rows in ([[0, 10, 0]], [[x.numel() - 5, 10, 0, 0]], [[0, 10, -1, 0]], [[0, 10, 0, 2]], [[0, 300, 0, 0], [300, 300, 299, 0]], []):
        with pytest.raises(ValueError):
            eng.pcm_denoise(x, bad_rows, 1.0, bias_d)
    for bad_strengths in (-1.0, 17.0, float("nan"), [1.0, 1.0]):                      # among them: strengths differing in count from the rows
        with pytest.raises(ValueError):
            eng.pcm_denoise(x, [[0, 10, 0, 0]], bad_strengths, bias_d)
    with pytest.raises(ValueError):
        eng.pcm_denoise(x, [[0, 10, 0, 0]], 1.0, bias_d, out=x)                       # not in place
    with pytest.raises(ValueError):
        eng.pcm_denoise_bias(x, [[0, 1023]])
    assert call(s, mag=None, n_mag=0) == 0                                            # mag_out is optional; the context still works
    torch.cuda.synchronize()
    host = y.cpu().numpy()
    for sig, row, st in zip(sigs, rows, s_h.tolist()):
        assert np.array_equal(host[row[2]: row[2] + row[1]], ap.denoise_pcm(sig, bias[row[3]], st))
    assert (mag.cpu().numpy() == -7.0).all()


# ------------------------------------------------------------------ PcmStage.finish_output
def _counted(monkeypatch, lib):
    calls = []
    for name in ("vv_pcm_denoise", "vv_pcm_denoise_bias"):
        real = getattr(lib, name)
        monkeypatch.setattr(lib, name, lambda *a, _n=name, _r=real: calls.append(_n) or _r(*a))
    return calls


def test_finish_output_chain_equals_the_mirrors_and_unset_is_todays_bytes(eng, biases, monkeypatch):
    ap = _ap()
    bias, _bias_d = biases
    calls = _counted(monkeypatch, eng.lib)
    sigs = [du.speechlike(5000, 71), du.speechlike(3000, 72), du.speechlike(2000, 73)]
    plane, reqs = pack_requests([[s] for s in sigs], gap=7)
    pcm = _dev(plane)
    peak = -3.0
    chain = dict(pitch=[4, None, 4], formants="keep", loudness=-20.0, peak_dbfs=peak)
    today = eng.finish_output(pcm, reqs, 0.1, SR, None, "flac", **chain)
    for kw in (dict(denoise=None), dict(denoise=[None, None, None]), dict(denoise=None, denoise_bias=bias[0])):
        got = eng.finish_output(pcm, reqs, 0.1, SR, None, "flac", **chain, **kw)
        assert all(np.array_equal(a, b) for a, b in zip(got, today)) and not calls    # byte for byte, and nothing new is called
    strengths = [1.0, None, 0.5]
    den = dict(denoise=strengths, denoise_bias=bias[0])
    got = eng.finish_output(pcm, reqs, 0.1, SR, None, "flac", **chain, **den)
    assert calls == ["vv_pcm_denoise"]
    # the rate conversion that makes the pitch is held to N10's bound of 1 LSB, not to equality (tests/test_prosody_gpu.py), so as in N18's
    # chain test the device's own converted signal is the envelope correction's input; every other link is the mirror's, exactly
    shifted = eng.finish_output(pcm, reqs, 0.1, SR, pitch=chain["pitch"], **den)
    for x, s, p, g, t, y in zip(sigs, strengths, chain["pitch"], got, today, shifted):
        clean = x if s is None else ap.denoise_pcm(x, bias[0], s)                     # first in the chain: the pitch sees the cleaned signal
        if p is not None:
            lsb_condition(y, ap.shift_prosody(clean, p, None))
            clean = ap.keep_formants(clean, y, 1, 1)
        else:
            assert np.array_equal(y, clean)
        want = ap.encode_output(ap.normalize_loudness(clean, SR, -20.0, peak), "flac", SR)
        assert np.array_equal(g, want)
        assert np.array_equal(g, t) == (s is None)
    plain = eng.finish_output(pcm, reqs, 0.1, SR, denoise=2.0, denoise_bias=_dev(bias[1]))      # one strength for all, the profile as a device tensor
    assert all(np.array_equal(g, ap.denoise_pcm(x, bias[1], 2.0)) for g, x in zip(plain, sigs))
    for bad in (0.0, 17.0, [1.0, 1.0], "1"):
        with pytest.raises(ValueError):
            eng.finish_output(pcm, reqs, 0.1, SR, denoise=bad, denoise_bias=bias[0])
    with pytest.raises(ValueError):
        eng.finish_output(pcm, reqs, 0.1, SR, denoise=1.0, denoise_bias=bias[0][:100])


# ------------------------------------------------------------------ engine, tiny preset
def test_vocoder_bias_equals_the_mirror_under_both_decoders(eng):
    from vietvoice_tts_amd.model_spec import ModelSpec, make_synthetic_weights
    from vietvoice_tts_amd.runtime import HipSynth
    ap = _ap()
    vocos = HipSynth(ModelSpec.tiny_vocos(), make_synthetic_weights(ModelSpec.tiny_vocos(), 9527), device=DEV, acoustic_dtype="fp32", nfe_step=4)
    try:
        for e in (eng, vocos):
            pcm = e.vocoder_bias_pcm()
            assert pcm.dtype == torch.int16 and pcm.numel() >= du.N
            got = e.vocoder_bias()
            assert got.shape == (1, du.BINS) and got.data_ptr() == e.vocoder_bias().data_ptr()      # cached on the device
            assert np.array_equal(got.cpu().numpy()[0], ap.denoise_bias(pcm.cpu().numpy()))
    finally:
        vocos.close()


_PLAIN = dict(output_denoise=None, output_denoise_bias=None)


def _call(e, fn, *a, denoise=None, bias=None, **k):
    """One engine call under the given denoise options, from call serial 0 (the same start noise every time)."""
    e.config.output_denoise, e.config.output_denoise_bias = denoise, bias
    e.model_session_manager.noise_serial = 0
    try:
        return fn(*a, **k)
    finally:
        for key, v in _PLAIN.items():
            setattr(e.config, key, v)


@pytest.fixture(scope="module")
def tiny(tmp_path_factory):
    from vietvoice_tts_amd.core import ModelConfig, TTSEngine
    tmp = tmp_path_factory.mktemp("denoise_models")
    e = TTSEngine(ModelConfig(model_cache_dir=str(tmp), synthetic_model=True, nfe_step=5, acoustic_dtype="fp32", max_chunk_duration=8.0,
                              model_spec="tiny", noise_source="device", output_denoise=1.0))
    assert e.config.output_denoise == 1.0 and e._device_output()
    built_with = _call(e, e.synthesize, LONG, denoise=1.0)[0]                         # the option the engine was built with
    base = {t: _call(e, e.synthesize, t)[0] for t in (SHORT, LONG)}
    yield e, base, built_with
    e.cleanup()


def test_engine_device_and_host_finishes_agree(tiny, monkeypatch):
    ap = _ap()
    e, base, built_with = tiny
    hip = e.model_session_manager.engine
    model_bias = hip.vocoder_bias()[0].cpu().numpy()
    own_bias = [float(v) for v in du.random_bias(31, 3000.0)]
    calls = _counted(monkeypatch, hip.lib)
    for text in (SHORT, LONG):                                                        # one chunk and several
        for bias, profile in ((own_bias, np.asarray(own_bias)), (None, model_bias)):  # the caller's profile, and the model's own
            got, _ = _call(e, e.synthesize, text, denoise=1.0, bias=bias)
            assert calls == ["vv_pcm_denoise"]
            calls.clear()
            want = ap.denoise_pcm(base[text], profile, 1.0)
            assert got.dtype == np.int16 and np.array_equal(got, want) and not np.array_equal(got, base[text])
            with monkeypatch.context() as m:                                          # the same call finished on the host
                m.setattr(e, "_device_output", lambda *a, **k: False)
                host, _ = _call(e, e.synthesize, text, denoise=1.0, bias=bias)
            assert np.array_equal(host, got) and not calls
    assert np.array_equal(built_with, got)
    assert np.array_equal(_call(e, e.synthesize, SHORT)[0], base[SHORT]) and not calls      # unset: nothing new
    with pytest.raises(ValueError, match="output_denoise"):
        _call(e, e.synthesize_stream, SHORT, denoise=1.0)


def test_front_end_honours_a_per_request_strength(tiny):
    from vietvoice_tts_amd.batching import BatchingFrontend
    ap = _ap()
    e, base, _built_with = tiny
    model_bias = e.model_session_manager.engine.vocoder_bias()[0].cpu().numpy()
    texts = [(LONG, 0, dict(denoise=1.0)), (SHORT, 1, dict(denoise=0.5)), ("Tạm biệt và hẹn gặp lại.", 2, {})]
    fe = BatchingFrontend(e, max_wait_ms=300.0, max_requests=8)
    try:
        alone = [fe.submit(t, serial=s, **kw).result(timeout=300)[0] for t, s, kw in texts]
        n0 = fe.batches_run
        outs = [f.result(timeout=300)[0] for f in [fe.submit(t, serial=s, **kw) for t, s, kw in texts]]
        assert fe.batches_run == n0 + 1
        plain = fe.submit(LONG, serial=0).result(timeout=300)[0]
    finally:
        fe.close()
    for a, o in zip(alone, outs):
        assert o.dtype == np.int16 and np.array_equal(a, o)                           # alone == in a batch with another strength and a plain request
    assert np.array_equal(outs[0], ap.denoise_pcm(plain, model_bias, 1.0)) and not np.array_equal(outs[0], plain)


def test_rows_of_no_samples_and_of_exactly_a_frame_equal_the_mirror(eng, biases):
    """The lengths tests/denoise_util.LENGTHS lacks, 0 and 1024, between the others around a hop and a frame, in one call."""
    ap = _ap()
    bias, bias_d = biases
    lens = (0, 1, 255, 256, 257, 1023, 1024, 1025)
    sigs = [du.speechlike(n, 300 + n) for n in lens]
    rows_b = [k % 2 for k in range(len(sigs))]
    for x, b, (z, mag) in zip(sigs, rows_b, _launch(eng, sigs, 1.0, rows_b, bias_d)):
        want, want_mag = ap.denoise_pcm(x, bias[b], 1.0, mags=True)
        assert mag.shape == want_mag.shape == (du.frames_of(x.size), du.N) and np.array_equal(mag, want_mag), x.size
        assert z.dtype == np.int16 and np.array_equal(z, want), x.size
