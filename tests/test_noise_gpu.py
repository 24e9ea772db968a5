"""-m gpu: N9, the flow ODE's start noise drawn on the device (vv_noise_fill, csrc/vv_noise.hip).  Kernel level: the uniforms equal the
test-local Philox reference bit for bit, the normals stay inside a bound derived from the documented errors of the math calls, a value
depends on (seed, stream, frame, bin) alone, refusals launch nothing, and 2^22 draws pass fixed distribution conditions.  Engine level
(``noise_source="device"``): every path of the engine starts a request from the same noise, a chunk's noise does not depend on its
neighbours, and the default host source still draws from the seeded torch generator."""
import ctypes as C
import math

import numpy as np
import pytest
import torch

from tests import philox_reference as pr

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
B, N, SEQ = 3, 37, [37, 1, 0]
ONES = (1 << 64) - 1
SEEDS = [0, 9527, ONES]
STREAMS = [0, 1, (1 << 63) | 5, ONES]
PAIRS = [(s, t) for s in SEEDS for t in STREAMS]           # every key and stream word sees all-ones
NORMAL_BOUND = 2.0 ** -20       # x r.  Derived: logf 1 ulp (1/2 on r) + sqrtf 1 + sinpif / cospif 2 + one product 1/2 = 4.5 ulp <= 9 x 2^-24 of r;
                                # 16 x 2^-24 leaves under 2x margin.  Never fitted to a measurement.
LONG = "Hôm nay trời đẹp quá, chúng ta cùng nhau đi dạo quanh hồ nhé. " * 4


def _i32(v):
    return torch.tensor(list(v), dtype=torch.int32, device=DEV)


def _keys(rows):
    return np.array([[int(a), int(b)] for a, b in rows], dtype=np.uint64)


def _fill(eng, keys, seq, n, n_mel, kind):
    """vv_noise_fill into a buffer that held NaN: every element the call must write shows."""
    out = torch.full((len(keys), n, n_mel), float("nan"), dtype=torch.float32, device=DEV)
    eng.noise(keys, _i32(seq), n, kind=kind, n_mel=n_mel, out=out)
    torch.cuda.synchronize()
    return out.cpu()


def _triples():
    """The 12 (seed, stream) pairs, each once at position 0 (the item with all 37 rows), its two successors behind it."""
    return [_keys([PAIRS[(i + j) % len(PAIRS)] for j in range(B)]) for i in range(len(PAIRS))]


@pytest.fixture(scope="module")
def eng(hip_tiny):
    return hip_tiny["f32"]


# ------------------------------------------------------------------------------------------------ kernel level
@pytest.mark.parametrize("n_mel", [100, 8])
def test_uniform_mode_equals_the_reference_bit_for_bit(eng, n_mel):
    assert eng.spec.n_mel == 100                            # the tiny preset's width is the full model's
    for keys in _triples():
        got = _fill(eng, keys, SEQ, N, n_mel, 1)
        want = torch.from_numpy(pr.fill(keys, SEQ, N, n_mel, 1).astype(np.float32))
        assert torch.equal(got, want), keys.tolist()
        assert float(got[0].min()) > 0.0 and float(got[0].max()) < 1.0
        pad = torch.cat([got[1, 1:].reshape(-1), got[2].reshape(-1)])
        assert bool((pad == 0).all()) and not bool(torch.signbit(pad).any())        # exactly +0.0f behind seq_len
    keys = _keys(PAIRS[4:7])
    got = _fill(eng, keys, [-3, N + 9, 5], N, n_mel, 1)                              # lengths are clamped to [0, N]
    assert torch.equal(got, torch.from_numpy(pr.fill(keys, [0, N, 5], N, n_mel, 1).astype(np.float32)))
    assert not bool(torch.signbit(got[0]).any()) and bool((got[0] == 0).all())


def test_normal_mode_stays_inside_the_derived_bound(eng, capsys):
    worst = 0.0
    for keys in _triples():
        got = _fill(eng, keys, SEQ, N, 100, 0).double().numpy()
        z, r = pr.fill(keys, SEQ, N, 100, 0)
        live = r > 0
        assert np.isfinite(got).all()
        ratio = np.abs(got - z)[live] / r[live]
        worst = max(worst, float(ratio.max()))
        pad = torch.from_numpy(got[~live])
        assert bool((pad == 0).all()) and not bool(torch.signbit(pad).any())
    with capsys.disabled():
        print(f"\n[noise] normal mode: max |z_dev - z_ref| / r = {worst / 2.0 ** -24:.3f} x 2^-24 (bound 16 x 2^-24)")
    assert worst <= NORMAL_BOUND, worst / 2.0 ** -24


def test_the_host_check_cases_on_the_device(eng):
    """tools/noise_host_check.py's list (n_mel 4 and 100, N 1 and 37, seq_len of -3, 0 and N + 5, all-ones key words), which the sanitizer
    builds run on exact-size buffers: the device gives the reference's bits (uniform) and stays inside NORMAL_BOUND (normal)."""
    from tests.host_check_util import tool
    for n_mel, n, seq, keys in tool("noise").CASES:
        k = _keys(keys)
        got = _fill(eng, k, list(seq), n, n_mel, 1)
        assert torch.equal(got, torch.from_numpy(pr.fill(k, list(seq), n, n_mel, 1).astype(np.float32))), (n_mel, n, seq)
        got = _fill(eng, k, list(seq), n, n_mel, 0).double().numpy()
        z, r = pr.fill(k, list(seq), n, n_mel, 0)
        live = r > 0
        assert np.isfinite(got).all() and (np.abs(got - z)[live] <= NORMAL_BOUND * r[live]).all(), (n_mel, n, seq)
        assert not got[~live].any() and not np.signbit(got[~live]).any()


def test_a_value_depends_on_its_key_frame_and_bin_alone(eng):
    key = (9527, (3 << 16) | 2)
    for kind in (0, 1):
        alone = _fill(eng, _keys([key]), [50], 50, 100, kind)                                   # B = 1, N = 50
        batch = _fill(eng, _keys([PAIRS[1], PAIRS[7], key]), [20, 37, 37], N, 100, kind)     # position 2 of three, N = 37
        assert torch.equal(batch[2], alone[0, :N])
        wide = _fill(eng, _keys([PAIRS[1], PAIRS[7], key]), [20, 37, 37], 128, 100, kind)    # N = 128: the first 37 rows agree
        assert torch.equal(wide[:, :N], batch) and bool((wide[:, N:] == 0).all())
        short = _fill(eng, _keys([key]), [9], 50, 100, kind)                                    # a shorter item is a prefix
        assert torch.equal(short[0, :9], alone[0, :9]) and bool((short[0, 9:] == 0).all())


def test_captured_fill_replays_with_new_keys(eng):
    """Keys live in device memory: a captured graph serves a new request by rewriting 16 bytes per item, with no new capture."""
    seq = _i32(SEQ)
    kd = eng.noise_keys_device(_keys(PAIRS[0:3]))
    out = torch.zeros((B, N, 100), dtype=torch.float32, device=DEV)
    eng.noise(kd, seq, N, out=out)                          # warm-up before the capture
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        eng.noise(kd, seq, N, out=out)
    for rows in (PAIRS[5:8], PAIRS[9:12]):
        kd.copy_(eng.noise_keys_device(_keys(rows)))
        g.replay()
        torch.cuda.synchronize()
        assert torch.equal(out.cpu(), _fill(eng, _keys(rows), SEQ, N, 100, 0)), rows


def test_refusals_launch_nothing_and_leave_the_context_usable(eng):
    keys = _keys(PAIRS[0:3])
    kd, seq = eng.noise_keys_device(keys), _i32(SEQ)
    buf = torch.full((B * N * 100 + 8,), 7.0, dtype=torch.float32, device=DEV)
    st = torch.cuda.current_stream().cuda_stream
    call = lambda b, n, m, x, kind: eng.lib.vv_noise_fill(eng.ctx, b, n, m, x, seq.data_ptr(), kd.data_ptr(), kind, st)
    p = buf.data_ptr()
    assert p % 16 == 0
    for args in ((B, N, 6, p, 0), (B, N, 102, p, 0), (B, N, 0, p, 0), (B, N, 100, p + 4, 0), (B, N, 100, p + 8, 1), (0, N, 100, p, 0), (-1, N, 100, p, 0),
                 (B, 0, 100, p, 0), (B, -5, 100, p, 0), (B, N, 100, p, 2), (B, N, 100, p, -1), (B, N, 100, None, 0)):
        assert call(*args) == -22, args
        assert b"vv_noise_fill" in eng.lib.vv_last_error(eng.ctx)
    torch.cuda.synchronize()
    assert bool((buf == 7.0).all())                         # nothing was launched
    got = _fill(eng, keys, SEQ, N, 100, 1)                  # and the next valid call is right
    assert torch.equal(got, torch.from_numpy(pr.fill(keys, SEQ, N, 100, 1).astype(np.float32)))
    with pytest.raises(RuntimeError, match="vv_noise_fill"):
        eng.noise(keys, seq, N, kind=3)


def test_distribution_of_four_million_draws(eng, capsys):
    """One item of n = 2^22 elements under the key (9527, 0); fixed inputs, fixed conditions.  The float64 reference for this key
    gives mean 4.6e-4, variance 0.99934 and KS 4.4e-4.  The grid-stride loop runs more than once at this size: the uniforms under the
    draws are compared with the reference as well."""
    n, n_mel = 1 << 22, 128
    rows = n // n_mel
    u = _fill(eng, _keys([(9527, 0)]), [rows], rows, n_mel, 1)
    assert torch.equal(u.reshape(-1), torch.from_numpy(pr.item_uniform(9527, 0, rows, n_mel).astype(np.float32)).reshape(-1))
    z = _fill(eng, _keys([(9527, 0), (9527, 1)]), [rows, rows], rows, n_mel, 0).double().reshape(2, n)
    z0, z1 = z[0], z[1]
    mean, var = float(z0.mean()), float(z0.var(unbiased=False))
    cdf = torch.special.ndtr(torch.sort(z0).values)
    i = torch.arange(1, n + 1, dtype=torch.float64)
    ks = float(torch.maximum((i / n - cdf).max(), (cdf - (i - 1) / n).max()))
    corr = float(((z0 - z0.mean()) * (z1 - z1.mean())).mean() / (z0.std(unbiased=False) * z1.std(unbiased=False)))
    with capsys.disabled():
        print(f"\n[noise] n = 2^22: mean {mean:.3e} (limit {4 / math.sqrt(n):.3e}), var - 1 {var - 1:.3e} (limit {4 * math.sqrt(2 / n):.3e}), "
              f"KS {ks:.3e} (limit {1.95 / math.sqrt(n):.3e}), corr(stream 0, 1) {corr:.3e} (limit {4 / math.sqrt(n):.3e})")
    assert abs(mean) < 4 / math.sqrt(n)
    assert abs(var - 1) < 4 * math.sqrt(2 / n)
    assert ks < 1.95 / math.sqrt(n)
    assert abs(corr) < 4 / math.sqrt(n)


def test_graphed_steps_with_keys_equals_eager(eng):
    """runtime.GraphedSteps(device_noise=True): the fill is captured in front of the steps and the decode; called with keys, the replay
    is bit-equal to the eager calls, for a second set of keys too."""
    from vietvoice_tts_amd.model_spec import noise_keys
    spec = eng.spec
    g = torch.Generator().manual_seed(3)
    la, lt, gen = [256 * 14, 256 * 9 + 77], [20, 13], [11, 17]
    S, T = max(la), max(lt)
    audio = torch.zeros((2, S), dtype=torch.int16)
    ids = torch.zeros((2, T), dtype=torch.int32)
    for b in range(2):
        audio[b, : la[b]] = (torch.randn(la[b], generator=g) * 3000).to(torch.int16)
        ids[b, : lt[b]] = torch.randint(0, spec.vocab_size, (lt[b],), generator=g, dtype=torch.int32)
    lens = [la[b] // spec.hop_length + 1 + gen[b] for b in range(2)]
    n, t_gen = max(lens), max(gen)
    pre = eng.preprocess(audio.to(DEV), _i32(la), ids.to(DEV), _i32(lt), _i32(lens), n, seq_len_host=lens, audio_len_host=la)
    graph = eng.capture_steps(2, n, lens, t_gen, device_noise=True)
    for serial in (0, 5):
        keys = noise_keys(9527, serial, 2)
        x_e = eng.noise(keys, pre["seq_len"], n)
        assert torch.equal(x_e.cpu(), _fill(eng, keys, lens, n, spec.n_mel, 0))
        eng.transformer_steps(x_e, pre, 0, eng.n_steps)
        pcm_e, len_e = eng.decode(x_e, pre, t_gen)
        x_g, pcm_g, len_g = graph(keys, pre)
        torch.cuda.synchronize()
        assert torch.equal(x_g, x_e) and torch.equal(pcm_g, pcm_e) and torch.equal(len_g, len_e), serial
    # exactly one of noise / noise_keys
    with pytest.raises(ValueError, match="exactly one"):
        eng.synthesize_batch(audio.to(DEV), _i32(la), ids.to(DEV), _i32(lt), _i32(lens), n, None, t_gen)
    with pytest.raises(ValueError, match="exactly one"):
        eng.synthesize_batch(audio.to(DEV), _i32(la), ids.to(DEV), _i32(lt), _i32(lens), n, x_e, t_gen, noise_keys=keys)
    x_b, pcm_b, len_b, _ = eng.synthesize_batch(audio.to(DEV), _i32(la), ids.to(DEV), _i32(lt), _i32(lens), n, None, t_gen, seq_len_host=lens,
                                                audio_len_host=la, noise_keys=keys)
    torch.cuda.synchronize()
    assert torch.equal(x_b, x_e) and torch.equal(pcm_b, pcm_e)


# ------------------------------------------------------------------------------------------------ engine level
def _engine(tmp, **kw):
    from vietvoice_tts_amd.core import ModelConfig, TTSEngine
    kw = {**dict(model_spec="tiny", noise_source="device"), **kw}
    cfg = ModelConfig(model_cache_dir=str(tmp), synthetic_model=True, nfe_step=5, acoustic_dtype="fp32", max_chunk_duration=8.0, **kw)
    return TTSEngine(cfg)


def _lsb(a, b):
    assert a.shape == b.shape, (a.shape, b.shape)
    return int(np.abs(a.astype(np.int32) - b.astype(np.int32)).max())


@pytest.fixture(scope="module")
def device_wave(tmp_path_factory):
    """LONG through ``synthesize`` on a fresh device-noise engine (call serial 0): computed once, compared by several tests."""
    tmp = tmp_path_factory.mktemp("noise_models")
    e = _engine(tmp)
    wave, _ = e.synthesize(LONG)
    plan = list(e._last_plan)
    e.cleanup()
    assert wave.dtype == np.int16 and len(plan) > 1
    return tmp, wave, plan


def test_device_noise_engine_matches_the_engine_on_oracle_sessions(device_wave):
    """The device's noise copied to the host and fed to the CPU oracle chunk by chunk (the same TTSEngine class plans the chunks and
    joins the waves): the PCM of the HIP engine agrees within the +-2 LSB of the oracle test of the host source."""
    from vietvoice_tts_amd.core import ModelConfig, TTSEngine
    from vietvoice_tts_amd.model_spec import noise_keys
    from oracle.vv_oracle import Oracle, OracleSession
    tmp, got, plan = device_wave
    holder = {}

    def factory(spec, weights, config):
        holder["oracle"] = Oracle(spec, weights, nfe_step=config.nfe_step)
        return {k: OracleSession(holder["oracle"], k, seed=config.random_seed) for k in ("preprocess", "transformer", "decode")}
    cfg = ModelConfig(model_cache_dir=str(tmp), synthetic_model=True, model_spec="tiny", nfe_step=5, acoustic_dtype="fp32", max_chunk_duration=8.0)
    ora = TTSEngine(cfg, session_factory=factory)
    orc = holder["oracle"]
    ref_clip, ref_txt = ora.model_session_manager.select_sample()
    inputs = ora._prepare_inputs(ref_clip, ref_txt, LONG)
    assert [int(i[2][0]) for i in inputs] == plan
    hip = _engine(tmp)
    keys = noise_keys(cfg.random_seed, 0, len(inputs))
    waves = []
    for c, (audio, ids, max_dur, _ts) in enumerate(inputs):
        n = int(max_dur[0])
        noise = hip.model_session_manager.engine.noise(keys[c: c + 1], _i32([n]), n).cpu()[0]
        _x, pcm = orc.synthesize(torch.from_numpy(np.asarray(audio).reshape(-1)), torch.from_numpy(np.asarray(ids).reshape(-1)), n, noise)
        waves.append(pcm.numpy().astype(np.int16).reshape(-1))
    hip.cleanup()
    want = np.asarray(ora.audio_processor.concatenate_with_crossfade_improved(waves, cfg.cross_fade_duration, cfg.sample_rate)).reshape(-1)
    ora.cleanup()
    assert got.shape == want.shape
    d = np.abs(got.astype(np.int32) - want.astype(np.int32))
    assert int(d.max()) <= 2 and float((d > 1).mean()) < 1e-3, (int(d.max()), float((d > 1).mean()))


@pytest.mark.parametrize("fuse_nfe", [1, 2])
def test_session_path_starts_from_the_device_paths_noise(device_wave, fuse_nfe):
    tmp, wave_dev, _plan = device_wave
    e = _engine(tmp, fuse_nfe=fuse_nfe)
    m = e.model_session_manager
    ref, txt = m.select_sample()
    inputs = e._prepare_inputs(ref, txt, LONG)
    # the preprocess session returns the very noise the device path starts from (call serial 0, chunk 1) ...
    from vietvoice_tts_amd.model_spec import noise_keys
    n1 = int(inputs[1][2][0])
    want = m.engine.noise(noise_keys(e.config.random_seed, 0, len(inputs))[1:2], _i32([n1]), n1).cpu().numpy()
    waves = e._synthesize_sessions(inputs)      # ... 1 + (nfe - 1) / fuse_nfe + 1 session.run per chunk, the reference's pattern
    assert m.noise_serial == 1
    m.queue_session_keys(noise_keys(e.config.random_seed, 0, len(inputs))[1:2])
    outs = e._run_preprocess(*inputs[1][:3])
    assert outs[0].shape == (1, n1, 100) and np.array_equal(outs[0], want)
    wave_ses = e.audio_processor.concatenate_with_crossfade_improved(waves, e.config.cross_fade_duration, e.config.sample_rate)
    e.cleanup()
    assert _lsb(wave_ses, wave_dev) <= 2


def test_stream_path_starts_from_the_device_paths_noise(device_wave):
    tmp, wave_dev, _plan = device_wave
    e = _engine(tmp)
    blocks = list(e.synthesize_stream(LONG, chunks_per_step=1))          # one call serial for the whole stream
    assert len(blocks) > 1 and e.model_session_manager.noise_serial == 1
    e.cleanup()
    assert _lsb(np.concatenate(blocks), wave_dev) <= 2


def test_front_end_serial_is_the_engines_call_serial(device_wave):
    """Call k of a fresh engine and a front-end request with serial = k start from the same noise: k = 0 against ``device_wave``,
    k = 1 against a second call; and the request's audio does not depend on what shares its batch."""
    from vietvoice_tts_amd.batching import BatchingFrontend
    tmp, wave_dev, _plan = device_wave
    text = "Xin chào các bạn, hôm nay thế nào?"
    e = _engine(tmp)
    e.synthesize("Tạm biệt.")                                             # call 0
    second, _ = e.synthesize(text)                                        # call 1
    e.cleanup()
    e = _engine(tmp)
    fe = BatchingFrontend(e, max_wait_ms=300.0, max_requests=8)
    try:
        first = fe.submit(LONG, serial=0).result(timeout=300)[0]
        alone = fe.submit(text, serial=1).result(timeout=300)[0]
        n0 = fe.batches_run
        futs = [fe.submit("Tạm biệt và hẹn gặp lại.", speed=1.3, serial=8, gender="male"), fe.submit(text, serial=1), fe.submit(LONG, speed=0.8, serial=9)]
        outs = [f.result(timeout=300)[0] for f in futs]
        assert fe.batches_run == n0 + 1
    finally:
        fe.close()
        e.cleanup()
    assert _lsb(first, wave_dev) <= 2
    assert _lsb(alone, second) <= 2
    assert _lsb(outs[1], alone) <= 2                                      # alone vs inside a three-request batch
    assert all(o.dtype == np.int16 and o.size > 0 for o in outs)


def test_seeds(device_wave):
    tmp, wave_dev, _plan = device_wave          # the model pack of tmp stays: only the noise follows random_seed
    a = _engine(tmp)
    wa, _ = a.synthesize(LONG)
    a.cleanup()
    assert np.array_equal(wa, wave_dev)
    b = _engine(tmp, random_seed=9528)
    wb, _ = b.synthesize(LONG)
    b.cleanup()
    assert wb.shape == wave_dev.shape and _lsb(wb, wave_dev) > 2


def test_a_chunks_noise_does_not_depend_on_its_neighbours(device_wave):
    """Two chunks in one call (keys of call serial 0, chunks 0 and 1): lengthening the first chunk's text leaves the second chunk's
    audio as it was.  With the host source the two share one generator stream, and the second chunk's noise moves with the first's length."""
    from vietvoice_tts_amd.model_spec import noise_keys
    tmp = device_wave[0]
    e = _engine(tmp)
    ref, txt = e.model_session_manager.select_sample()
    first = e._prepare_inputs(ref, txt, "Xin chào.")
    longer = e._prepare_inputs(ref, txt, "Xin chào các bạn, hôm nay trời đẹp quá.")
    second = e._prepare_inputs(ref, txt, "Chúng ta cùng nhau đi dạo quanh hồ nhé.")
    assert len(first) == len(longer) == len(second) == 1 and int(longer[0][2][0]) > int(first[0][2][0])
    keys = noise_keys(e.config.random_seed, 0, 2)
    w1 = e._synthesize_device(first + second, noise_keys=keys)
    w2 = e._synthesize_device(longer + second, noise_keys=keys)
    e.cleanup()
    assert w2[0].size > w1[0].size
    assert _lsb(w1[1].reshape(-1), w2[1].reshape(-1)) <= 2


def test_edit_speech_with_device_noise(device_wave):
    from vietvoice_tts_amd.core import AudioProcessor
    from vietvoice_tts_amd.model_spec import noise_keys
    from vietvoice_tts_amd.pack import MAX_POS
    from vietvoice_tts_amd.speech_edit import plan_edit
    tmp = device_wave[0]
    e = _engine(tmp)
    sr = e.config.sample_rate
    clip, _ = e.synthesize("Xin chào các bạn, hôm nay trời đẹp quá.")
    dur = clip.size / sr
    parts, fix, text = [(0.3 * dur, 0.5 * dur)], [0.3 * dur], "Xin chào các anh, hôm nay trời đẹp quá."
    out, _ = e.edit_speech(clip, text, parts, fix_duration=fix, seed=7)
    again, _ = e.edit_speech(clip, text, parts, fix_duration=fix, seed=7)
    other, _ = e.edit_speech(clip, text, parts, fix_duration=fix, seed=8)
    assert out.dtype == np.int16 and np.array_equal(out, again) and not np.array_equal(out, other)
    # the same edit straight through HipSynth.edit_batch with the keys edit_speech maps seed = 7 to: the same PCM, and the kept frames
    # are the conditioning's mel bit for bit whatever the noise
    m = e.model_session_manager
    plan = plan_edit(clip.size, parts, fix, sr, e.config.hop_length, m.spec.n_fft, MAX_POS)
    assert out.size == plan.spliced_len
    entry = e.voice_bank.get(AudioProcessor.to_wav_bytes(clip, sr))
    ids = torch.from_numpy(e.text_processor.text_to_indices([list(e.text_processor.clean_text(text))])).to(DEV)
    tl = torch.tensor([ids.shape[1]], dtype=torch.int32, device=DEV)
    keep = torch.from_numpy(plan.keep[None]).to(DEV)
    run = lambda **kw: m.engine.edit_batch(entry.pcm_dev, plan.rows(), [plan.spliced_len], ids, tl, keep, **kw)
    x7, pcm7, _n = run(noise_keys=noise_keys(7, 0, 1, edit=True))
    x8, _pcm8, _n = run(noise_keys=noise_keys(8, 0, 1, edit=True))
    g = torch.Generator().manual_seed(1)
    xh, _pcmh, _n = run(noise=torch.randn((1, plan.n_frames, m.spec.n_mel), generator=g).to(DEV))
    assert np.array_equal(pcm7[0, : plan.spliced_len].cpu().numpy(), out)
    k = torch.from_numpy(plan.keep[: plan.n_frames].astype(bool))
    assert 0 < int(k.sum()) < plan.n_frames
    assert torch.equal(x7[0].cpu()[k], x8[0].cpu()[k]) and torch.equal(x7[0].cpu()[k], xh[0].cpu()[k])
    assert not torch.equal(x7[0].cpu()[~k], x8[0].cpu()[~k])
    with pytest.raises(ValueError, match="exactly one"):
        run()
    # seedless edits advance the engine's edit serial: two calls differ
    s1, _ = e.edit_speech(clip, text, parts, fix_duration=fix)
    s2, _ = e.edit_speech(clip, text, parts, fix_duration=fix)
    assert m.edit_serial == 2 and not np.array_equal(s1, s2)
    e.cleanup()


def test_vocos_preset_length_plumbing(tmp_path):
    a = _engine(tmp_path, model_spec="tiny-vocos")
    wa, _ = a.synthesize(LONG)
    plan = list(a._last_plan)
    a.cleanup()
    b = _engine(tmp_path, model_spec="tiny-vocos", use_hip_graph=True)   # bucketed N > every seq_len: rows behind a length are zero
    wb, _ = b.synthesize(LONG)
    b.cleanup()
    assert len(plan) > 1 and wa.dtype == np.int16 and wa.size > 0 and int(np.abs(wa).max()) > 0
    assert _lsb(wa, wb) <= 2


def test_host_source_still_draws_from_the_seeded_generator(tmp_path, monkeypatch):
    """The default on the same build: ``_synthesize_device`` draws with torch.randn from the manager's generator (its state advances),
    nothing reaches vv_noise_fill, and the blocks are the ones a generator with the same seed gives."""
    from vietvoice_tts_amd.runtime import HipSynth
    e = _engine(tmp_path, noise_source="host")
    m = e.model_session_manager
    assert e.config.noise_source == "host" and not e._device_noise()
    calls = []
    real = m.engine.lib.vv_noise_fill
    monkeypatch.setattr(m.engine.lib, "vv_noise_fill", lambda *a: calls.append(a) or real(*a))
    monkeypatch.setattr(HipSynth, "noise", lambda self, *a, **k: calls.append(a) or pytest.fail("HipSynth.noise called with the host source"))
    seen = []
    real_randn = torch.randn
    monkeypatch.setattr(torch, "randn", lambda *a, **k: seen.append(k.get("generator")) or real_randn(*a, **k))
    before = m.noise_gen.get_state().clone()
    wave, _ = e.synthesize(LONG)
    monkeypatch.setattr(torch, "randn", real_randn)
    assert not calls and m.noise_serial == 0
    assert len(seen) == len(e._last_plan) > 1 and all(g is m.noise_gen for g in seen)
    assert not torch.equal(m.noise_gen.get_state(), before)
    ref, txt = m.select_sample()
    inputs = e._prepare_inputs(ref, txt, LONG)
    gen = torch.Generator().manual_seed(e.config.random_seed)
    blocks = [torch.randn((int(i[2][0]), 100), generator=gen, dtype=torch.float32) for i in inputs]
    waves = e._synthesize_device(inputs, noise_blocks=blocks)
    again = e.audio_processor.concatenate_with_crossfade_improved(waves, e.config.cross_fade_duration, e.config.sample_rate)
    e.cleanup()
    assert np.array_equal(np.asarray(again).reshape(-1), wave)
