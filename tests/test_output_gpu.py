"""-m gpu: N10, the output stage on the device (csrc/vv_output.hip): vv_join_chunks against the fixture produced by the reference's own
function (bit for bit), vv_pcm_encode against stdlib audioop's tables (all 65,536 inputs), vv_pcm_resample against
scipy.signal.resample_poly (1 LSB, 1 sample in 10^4), and the engine paths that use them."""
import numpy as np
import pytest
import torch

from tests.output_util import golden, join_cases, lsb_condition, pack_requests, scipy_resample

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
RATES = [8000, 16000, 22050, 44100, 48000]
GUARD = 64            # sentinel samples in front of and behind a call's output
SENTINEL = -21846     # 0xAAAA
SHORT = "Xin chào các bạn, hôm nay trời đẹp quá."
LONG = "Hôm nay trời đẹp quá, chúng ta cùng nhau đi dạo quanh hồ nhé. " * 4


@pytest.fixture(scope="module")
def eng(hip_tiny):
    return hip_tiny["f32"]


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _join(eng, chunk_sets, d, sr):
    """One vv_join_chunks call between guard bands -> the requests' results (host); the guards and the gaps between the slices are checked."""
    plane, reqs = pack_requests(chunk_sets)
    total = sum(max(sum(c.size for c in cs), 8) + 8 for cs in chunk_sets) + 2 * GUARD
    out = torch.full((total,), SENTINEL, dtype=torch.int16, device=DEV)
    _o, offs, lens = eng.join_chunks(_dev(plane), reqs, d, sr, out=out, out_base=GUARD)
    host = out.cpu().numpy()
    written = np.zeros(total, bool)
    for o, n in zip(offs, lens):
        written[o: o + n] = True
    assert offs[0] == GUARD and (host[~written] == SENTINEL).all(), "a sample outside a request's slice was written"
    return [host[o: o + n] for o, n in zip(offs, lens)]


# ------------------------------------------------------------------ join
def test_join_equals_the_reference_fixture_case_by_case(eng):
    cases = join_cases()
    assert len(cases) >= 40
    for name, sr, d, chunks, want in cases:
        got = _join(eng, [chunks], d, sr)[0]
        assert got.dtype == np.int16 and got.shape == want.shape, name
        assert torch.equal(torch.from_numpy(got.copy()), torch.from_numpy(want)), (name, int(np.abs(got.astype(int) - want.astype(int)).max()),
                                                                                   int((got != want).sum()))


def test_join_of_many_requests_in_one_call_equals_each_alone(eng):
    groups = {}
    for case in join_cases():
        groups.setdefault((case[1], case[2]), []).append(case)
    assert max(len(g) for g in groups.values()) >= 5
    for (sr, d), cases in groups.items():
        outs = _join(eng, [c[3] for c in cases], d, sr)
        for (name, _sr, _d, _chunks, want), got in zip(cases, outs):
            assert got.shape == want.shape and np.array_equal(got, want), name


def test_join_of_random_chunk_sets_equals_the_host_mirror(eng):
    from vietvoice_tts_amd.core import AudioProcessor
    rng = np.random.default_rng(77)
    for sr, d in ((24000, 0.1), (16000, 0.01), (8000, 0.0)):
        n = int(d * sr)
        sets = []
        for _ in range(12):
            k = int(rng.integers(1, 7))
            lens = [int(rng.choice([1, 2, max(n - 1, 1), n + 1, 2 * n + 3, 3000, 5001])) for _ in range(k)]
            chunks = [np.clip(rng.standard_normal(m) * rng.choice([20, 400, 3000, 12000]), -32768, 32767).astype(np.int16) for m in lens]
            if rng.random() < 0.3:
                chunks[int(rng.integers(k))][0] = 32767
            sets.append(chunks)
        outs = _join(eng, sets, d, sr)
        for chunks, got in zip(sets, outs):
            want = np.asarray(AudioProcessor.concatenate_with_crossfade_improved([c.copy() for c in chunks], d, sr))
            assert np.array_equal(got, want), (sr, d, [c.size for c in chunks])


def test_join_refusals_launch_nothing_and_leave_the_context_usable(eng):
    from vietvoice_tts_amd.runtime import JOIN_MAX_N
    a = np.arange(100, dtype=np.int16)
    pcm = _dev(np.concatenate([a, a]))
    out = torch.full((512,), SENTINEL, dtype=torch.int16, device=DEV)
    ws = torch.zeros((16,), dtype=torch.int32, device=DEV)
    fade = torch.zeros((64,), dtype=torch.float64, device=DEV)
    I64 = (1 << 63) - 1
    rows = torch.tensor([[0, 100, 0, 0, 90, 0, 1, 0], [100, 100, 90, 10, I64, 0, 1, 0]], dtype=torch.int64)
    reqs = torch.tensor([[0, 2, 0, 190]], dtype=torch.int64)
    rows_d, reqs_d = rows.to(DEV), reqs.to(DEV)
    st = torch.cuda.current_stream().cuda_stream

    def call(pcm_p=pcm.data_ptr(), rows_p=rows_d.data_ptr(), rows_h=rows, reqs_p=reqs_d.data_ptr(), reqs_h=reqs, R=1, fade_p=fade.data_ptr(),
             max_n=10, out_p=out.data_ptr(), ws_p=ws.data_ptr()):
        return eng.lib.vv_join_chunks(eng.ctx, pcm_p, 200, rows_p, None if rows_h is None else rows_h.data_ptr(), 2, reqs_p,
                                      None if reqs_h is None else reqs_h.data_ptr(), R, fade_p, 64, max_n, 100, out_p, 512, ws_p, st)
    empty = rows.clone()
    empty[1, 1] = 0
    for bad in (dict(pcm_p=None), dict(rows_p=None), dict(reqs_p=None), dict(out_p=None), dict(ws_p=None), dict(fade_p=None), dict(R=0),
                dict(out_p=out.data_ptr() + 2), dict(max_n=JOIN_MAX_N + 1), dict(rows_h=empty), dict(rows_h=None)):
        assert call(**bad) == -22, bad
        assert b"vv_join_chunks" in eng.lib.vv_last_error(eng.ctx) or b"join_chunks" in eng.lib.vv_last_error(eng.ctx)
    torch.cuda.synchronize()
    assert (out.cpu().numpy() == SENTINEL).all()                       # nothing was launched
    with pytest.raises(ValueError, match="empty chunk"):
        eng.join_chunks(pcm, [[(0, 100), (100, 0)]], 0.1, 24000)
    with pytest.raises(ValueError, match="does not fit"):
        eng.join_chunks(pcm, [[(150, 100)]], 0.1, 24000)
    with pytest.raises(ValueError, match="more than"):
        eng.join_chunks(_dev(np.zeros(120000, np.int16)), [[(0, 60000), (60000, 60000)]], 1.5, 24000)
    got, offs, lens = eng.join_chunks(pcm, [[(0, 100), (100, 100)]], 10 / 24000 + 1e-12, 24000)       # the context still works
    from vietvoice_tts_amd.core import AudioProcessor
    want = AudioProcessor.concatenate_with_crossfade_improved([a.copy(), a.copy()], 10 / 24000 + 1e-12, 24000)
    assert lens == [190] and np.array_equal(got.cpu().numpy()[offs[0]: offs[0] + 190], want)


# ------------------------------------------------------------------ G.711
@pytest.mark.parametrize("enc", ["ulaw", "alaw"])
def test_encode_equals_audioop_for_every_input(eng, enc):
    table = golden()[1][f"g711_{enc}"]
    every = np.arange(-32768, 32768, dtype=np.int16)
    x = _dev(every)
    got = eng.pcm_encode(x, [[0, 65536, 0]], enc).cpu().numpy()
    assert got.dtype == np.uint8 and np.array_equal(got, table)
    # every source offset 0..3 with every length 1..9 at shifting destination offsets: the scalar head and tail, between sentinels
    rows, pos = [], 3
    for so in range(4):
        for n in range(1, 10):
            rows.append([30000 + 1000 * len(rows) + so, n, pos])
            pos += n + (len(rows) % 3)
    y = eng.pcm_encode(x, rows, enc, n_y=pos + 5).cpu().numpy()
    for so, n, do in rows:
        assert np.array_equal(y[do: do + n], table[so: so + n]), (so, n, do)
    with pytest.raises(ValueError):
        eng.pcm_encode(x, [[0, 10, 0], [20, 10, 5]], enc)              # rows overlap on the output
    with pytest.raises(ValueError):
        eng.pcm_encode(x, [[65530, 10, 0]], enc)
    assert eng.lib.vv_pcm_encode(eng.ctx, x.data_ptr(), 65536, None, 1, 8, 1, x.data_ptr(), 8, None) == -22
    assert eng.lib.vv_pcm_encode(eng.ctx, x.data_ptr(), 65536, x.data_ptr(), 1, 8, 3, x.data_ptr(), 8, None) == -22


# ------------------------------------------------------------------ output rate
@pytest.mark.parametrize("dst", RATES)
def test_resample_against_scipy(eng, dst, capsys):
    from vietvoice_tts_amd.core.audio_processor import output_design, resample_len
    x = golden()[1]["poly_x"]
    _taps, up, down, _skip = output_design(24000, dst)
    xd = _dev(x)
    sizes = sorted({n for n in (1, 2, down - 1, down, down + 1, 3001, x.size) if n >= 1})
    alone = {}
    for n in sizes:
        y = eng.pcm_resample(xd, [[0, n, 0, resample_len(n, up, down), 0, 0]], 24000, dst).cpu().numpy()
        n_diff = lsb_condition(y, scipy_resample(x[:n], up, down))
        alone[n] = y
        with capsys.disabled():
            print(f"\n[output] 24000 -> {dst} Hz: {n} samples in, {y.size} out, {n_diff} differ from scipy", end="")
    # a batch of ragged rows (odd source offsets) equals each row alone
    rows, pos = [], 0
    for k, n in enumerate(sizes):
        n = min(n, x.size - k)
        rows.append([k, n, pos, resample_len(n, up, down), 0, 0])
        pos += rows[-1][3] + 1
    y = eng.pcm_resample(xd, rows, 24000, dst, n_y=pos).cpu().numpy()
    for (so, n, do, n_out, _m, _i) in rows:
        one = eng.pcm_resample(xd, [[so, n, 0, n_out, 0, 0]], 24000, dst).cpu().numpy()
        assert np.array_equal(y[do: do + n_out], one), (dst, so, n)
    # the clip cut into blocks with (m0, i0) rows (what OutputStream hands over) equals the whole clip bit for bit
    from vietvoice_tts_amd.core.audio_processor import OutputStream
    resample, _enc = eng.output_stream_backends(24000, dst, "pcm16")
    for block in (997, 2500):
        s = OutputStream(24000, dst, "pcm16", resample, None)
        got = np.concatenate([s.push(x[i: i + block]) for i in range(0, x.size, block)] + [s.flush()])
        assert np.array_equal(got, alone[x.size]), (dst, block)


# ------------------------------------------------------------------ engine, tiny preset
def _engine(tmp, **kw):
    from vietvoice_tts_amd.core import ModelConfig, TTSEngine
    kw = {**dict(model_spec="tiny", noise_source="device"), **kw}
    return TTSEngine(ModelConfig(model_cache_dir=str(tmp), synthetic_model=True, nfe_step=5, acoustic_dtype="fp32", max_chunk_duration=8.0, **kw))


def _call(e, fn, *a, stage="host", rate=None, enc="pcm16", **k):
    """One engine call under the given output options, from call serial 0 (the same start noise every time)."""
    e.config.output_stage, e.config.output_sample_rate, e.config.output_encoding = stage, rate, enc
    e.model_session_manager.noise_serial = 0
    return fn(*a, **k)


@pytest.fixture(scope="module")
def tiny(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("output_models")
    e = _engine(tmp)
    base = {t: _call(e, e.synthesize, t)[0] for t in (SHORT, LONG)}
    plan = list(e._last_plan)
    assert len(plan) >= 3 and base[LONG].dtype == np.int16
    yield e, base
    e.cleanup()


def test_default_options_call_none_of_the_new_entries(tiny, monkeypatch):
    e, base = tiny
    lib, calls = e.model_session_manager.engine.lib, []
    for name in ("vv_join_chunks", "vv_pcm_resample", "vv_pcm_encode"):
        real = getattr(lib, name)
        monkeypatch.setattr(lib, name, lambda *a, _n=name, _r=real: calls.append(_n) or _r(*a))
    assert not e._device_output()
    wave = _call(e, e.synthesize, LONG)[0]
    assert not calls and np.array_equal(wave, base[LONG])
    wave = _call(e, e.synthesize, LONG, stage="device")[0]
    assert calls == ["vv_join_chunks"] and np.array_equal(wave, base[LONG])
    del calls[:]
    _call(e, e.synthesize, LONG, rate=8000, enc="ulaw")
    assert calls == ["vv_join_chunks", "vv_pcm_resample", "vv_pcm_encode"]


@pytest.mark.parametrize("text", [SHORT, LONG])
def test_device_stage_equals_the_default_path(tiny, text):
    e, base = tiny
    wave, secs = _call(e, e.synthesize, text, stage="device")
    assert wave.dtype == np.int16 and secs > 0 and np.array_equal(wave, base[text])
    e.config.max_batch_chunks = 2                                     # several chunk groups: their planes back to back
    try:
        again = _call(e, e.synthesize, text, stage="device")[0]
        host = _call(e, e.synthesize, text)[0]
    finally:
        e.config.max_batch_chunks = 32
    assert np.array_equal(again, host)


def test_rate_and_mu_law_equal_the_host_mirrors(tiny, capsys, tmp_path):
    from vietvoice_tts_amd.core.audio_processor import lin2ulaw, resample_len, resample_output
    e, base = tiny
    pcm8, _ = _call(e, e.synthesize, LONG, rate=8000)
    assert pcm8.dtype == np.int16 and pcm8.size == resample_len(base[LONG].size, 1, 3)
    n_diff = lsb_condition(pcm8, resample_output(base[LONG], 24000, 8000))
    with capsys.disabled():
        print(f"\n[output] engine 24000 -> 8000 Hz: {n_diff} of {pcm8.size} samples differ from the host mirror", end="")
    path = tmp_path / "u.wav"
    ulaw, _ = _call(e, e.synthesize, LONG, rate=8000, enc="ulaw", output_path=str(path))
    assert ulaw.dtype == np.uint8 and np.array_equal(ulaw, lin2ulaw(pcm8))          # companding is exact: the same integers
    data = path.read_bytes()
    assert data[20:22] == b"\x07\x00" and data[24:28] == (8000).to_bytes(4, "little") and data.endswith(ulaw.tobytes() + b"\0" * (ulaw.size & 1))
    for step in (1, 2):
        blocks = list(_call(e, e.synthesize_stream, LONG, rate=8000, enc="ulaw", chunks_per_step=step))
        got = np.concatenate(blocks)
        assert len(blocks) > 1 and got.dtype == np.uint8 and np.array_equal(got, ulaw), step
    for step in (1, 2):                                               # the device stage alone: the stream keeps the host join
        got = np.concatenate(list(_call(e, e.synthesize_stream, LONG, stage="device", chunks_per_step=step)))
        assert np.array_equal(got, base[LONG]), step


def test_edit_speech_with_a_rate(tiny):
    from vietvoice_tts_amd.core.audio_processor import resample_output
    e, base = tiny
    clip = base[SHORT]
    dur = clip.size / 24000
    args = (clip, "Xin chào các anh, hôm nay trời đẹp quá.", [(0.3 * dur, 0.5 * dur)])
    plain, _ = _call(e, e.edit_speech, *args, seed=7)
    dev, _ = _call(e, e.edit_speech, *args, seed=7, stage="device")
    assert np.array_equal(dev, plain)
    out, _ = _call(e, e.edit_speech, *args, seed=7, rate=16000)
    assert out.dtype == np.int16 and out.size == -(-plain.size * 2 // 3)
    lsb_condition(out, resample_output(plain, 24000, 16000))


def test_front_end_batch_of_three_equals_each_alone(tiny):
    from vietvoice_tts_amd.batching import BatchingFrontend
    e, base = tiny
    texts = [(LONG, 0), (SHORT, 1), ("Tạm biệt và hẹn gặp lại.", 2)]
    e.config.output_stage, e.config.output_sample_rate, e.config.output_encoding = "device", None, "pcm16"
    fe = BatchingFrontend(e, max_wait_ms=300.0, max_requests=8)
    try:
        alone = [fe.submit(t, serial=s).result(timeout=300)[0] for t, s in texts]
        n0 = fe.batches_run
        outs = [f.result(timeout=300)[0] for f in [fe.submit(t, serial=s) for t, s in texts]]
        assert fe.batches_run == n0 + 1
    finally:
        fe.close()
        e.config.output_stage = "host"
    for a, o in zip(alone, outs):
        assert o.dtype == np.int16 and np.array_equal(a, o)
    assert np.array_equal(alone[0], base[LONG])                       # serial 0 = the engine's first call


def test_vocos_preset_lengths(tmp_path):
    e = _engine(tmp_path, model_spec="tiny-vocos")
    try:
        host = _call(e, e.synthesize, LONG)[0]
        plan = list(e._last_plan)
        dev = _call(e, e.synthesize, LONG, stage="device")[0]
    finally:
        e.cleanup()
    assert len(plan) > 1 and host.size > 0
    assert dev.shape == host.shape and np.array_equal(dev, host)      # hop * max(T - 1, 0) per chunk, from the host's own frame counts


# ------------------------------------------------------------------ the edge rows of tools/output_host_check.py
@pytest.mark.parametrize("n,sr,d", [(0, 8000, 0.0), (1, 8000, 1 / 8000 + 1e-9), (16, 8000, 0.002 + 1e-9), (100, 16000, 100 / 16000 + 1e-9),
                                    (2400, 24000, 0.1)])
def test_join_edge_sets_equal_the_host_mirror(eng, n, sr, d):
    """Junction sizes 0, 1, exactly the ring and more; chunks of 1, 2, 7, 8, 9 samples, one shorter than n and one shorter than 2 n, single
    chunks, a 32767 first and last in a chunk, and eight chunks that start 0 ... 7 samples past a 16-byte boundary."""
    from tests.host_check_util import tool
    from vietvoice_tts_amd.core import AudioProcessor
    t = tool("output")
    assert int(d * sr) == n
    sets, residues = t.edge_sets(n, seed=n)
    plane, reqs = t.pack(sets, residues)
    assert [so % 8 for so, _n in reqs[4]] == list(range(8))                        # torch's allocations are 16-byte aligned and more
    total = sum(max(sum(c.size for c in cs), 8) + 8 for cs in sets) + 2 * GUARD
    out = torch.full((total,), SENTINEL, dtype=torch.int16, device=DEV)
    pd = _dev(plane)
    assert pd.data_ptr() % 16 == 0
    _o, offs, lens = eng.join_chunks(pd, reqs, d, sr, out=out, out_base=GUARD)
    host = out.cpu().numpy()
    written = np.zeros(total, bool)
    for cs, o, m in zip(sets, offs, lens):
        written[o: o + m] = True
        want = np.asarray(AudioProcessor.concatenate_with_crossfade_improved([c.copy() for c in cs], d, sr))
        assert np.array_equal(host[o: o + m], want), (n, [c.size for c in cs])
    assert (host[~written] == SENTINEL).all(), "a sample outside a request's slice was written"


def test_join_with_a_junction_whose_pairwise_tree_is_seven_deep(eng):
    """8191 samples: the deepest tree numpy's pairwise sum builds over one buffer (the fixture's 8192 and 8193 stay 6 deep)."""
    from tests.host_check_util import tool
    from vietvoice_tts_amd.core import AudioProcessor
    t = tool("output")
    n, sr, d = t.DEEP
    sets = t.deep_tree_sets()
    for cs, got in zip(sets, _join(eng, sets, d, sr)):
        want = np.asarray(AudioProcessor.concatenate_with_crossfade_improved([c.copy() for c in cs], d, sr))
        assert np.array_equal(got, want), [c.size for c in cs]
