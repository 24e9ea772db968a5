"""-m gpu: the drop-in TTSEngine on the HIP sessions (synthetic tiny model pack): the reference-style session
path (host numpy round trips, one step per run) and the device-resident batched path must produce the same PCM
from the same seed; the hipGraph-bucketed vocoder path must match the eager one; API errors keep their types."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

LONG = "Hôm nay trời đẹp quá, chúng ta cùng nhau đi dạo quanh hồ nhé. " * 4


def _engine(tmp, **kw):
    from vietvoice_tts_amd.core import ModelConfig, TTSEngine
    cfg = ModelConfig(model_cache_dir=str(tmp), synthetic_model=True, model_spec="tiny", nfe_step=5, acoustic_dtype="fp32",
                      max_chunk_duration=8.0, **kw)
    return TTSEngine(cfg)


def test_engine_device_path_equals_session_path(tmp_path):
    e1 = _engine(tmp_path)
    wave_dev, secs = e1.synthesize(LONG)
    assert wave_dev.dtype == np.int16 and wave_dev.ndim == 1 and secs > 0 and len(e1._last_plan) > 1
    e1.cleanup()
    e2 = _engine(tmp_path)                       # fresh engine: same seed -> same noise stream
    ref, txt = e2.model_session_manager.select_sample()
    inputs = e2._prepare_inputs(ref, txt, LONG)
    waves = e2._synthesize_sessions(inputs)      # the reference's own driving pattern: 1 + (nfe-1) + 1 session.run per chunk
    wave_ses = e2.audio_processor.concatenate_with_crossfade_improved(waves, e2.config.cross_fade_duration, e2.config.sample_rate)
    e2.cleanup()
    assert wave_ses.shape == wave_dev.shape
    assert int(np.abs(wave_ses.astype(np.int32) - wave_dev.astype(np.int32)).max()) <= 2


def test_engine_hipgraph_vocoder_matches_eager(tmp_path):
    a = _engine(tmp_path, max_batch_chunks=2)
    wa, _ = a.synthesize(LONG)
    a.cleanup()
    b = _engine(tmp_path, max_batch_chunks=2, use_hip_graph=True)
    wb, _ = b.synthesize(LONG)
    wb2, _ = b.synthesize("Xin chào các bạn.")      # another bucket, graph cache grows
    assert len(b._decode_graphs) >= 1 and wb2.size > 0
    b.cleanup()
    assert wa.shape == wb.shape and int(np.abs(wa.astype(np.int32) - wb.astype(np.int32)).max()) <= 1


def test_engine_session_io_contract_and_errors(tmp_path):
    e = _engine(tmp_path)
    m = e.model_session_manager
    assert m.providers == ["HIPExecutionProvider"]
    ref, txt = m.select_sample()
    audio, ids, max_dur, ts = e._prepare_inputs(ref, txt, "Xin chào.")[0]
    outs = e._run_preprocess(audio, ids, max_dur)
    n = int(max_dur[0])
    assert len(outs) == 8 and outs[0].shape == (1, n, 100) and outs[1].shape == (1, n, 64) and outs[5].shape[:2] == (1, n)
    assert int(outs[7][0]) == audio.shape[-1] // 256 + 1
    noise, ts2 = m.sessions["transformer"].run(m.output_names["transformer"], dict(zip(m.input_names["transformer"], list(outs[:7]) + [ts])))
    assert noise.shape == outs[0].shape and int(ts2[0]) == 1
    pcm = e._run_decode(noise, outs[7])
    assert pcm.dtype == np.int16 and pcm.shape[:2] == (1, 1) and pcm.shape[2] == (n - int(outs[7][0])) * 256
    with pytest.raises(ValueError):
        e.synthesize("x", gender="robot")                       # select_sample errors propagate unwrapped
    with pytest.raises(RuntimeError, match="Speech synthesis failed"):
        e.config.max_chunk_duration = 1.0
        e.synthesize("một câu rất dài " * 30)
    e.cleanup()


def test_transformer_session_reads_fed_rope_tables_per_call(tmp_path):
    """the bf16 model computes the standard rope angles, but a session is FED its tables (reference I/O contract,
    core/tts_engine.py:161-170).  Non-standard tables on ANY call (not only the first) are read for that call and only for it:
    the result equals an engine switched to table reads, and the next standard-table call is the computed form again."""
    import torch
    from vietvoice_tts_amd.core import ModelConfig, TTSEngine
    cfg = ModelConfig(model_cache_dir=str(tmp_path), synthetic_model=True, model_spec="tiny", nfe_step=5, acoustic_dtype="bf16")
    e = TTSEngine(cfg)
    m = e.model_session_manager
    eng = m.engine
    ref, txt = m.select_sample()
    audio, ids, max_dur, ts = e._prepare_inputs(ref, txt, "Xin chào các bạn.")[0]
    outs = e._run_preprocess(audio, ids, max_dur)
    ses = m.sessions["transformer"]
    run = lambda tabs: ses.run(m.output_names["transformer"], dict(zip(m.input_names["transformer"], [outs[0]] + tabs + [outs[5], outs[6], ts])))[0]
    std = [np.ascontiguousarray(o) for o in outs[1:5]]
    first = run(std)
    odd = [np.ascontiguousarray(t[:, ::-1].copy()) for t in std]                     # positions reversed: valid tables, not the standard ones
    got_odd = run(odd)                                                               # second call of this session
    assert not np.array_equal(got_odd, first)
    with eng.reading_rope_tables():                                                  # what reading those tables gives
        x = torch.from_numpy(outs[0].copy()).to(eng.device)
        n = x.shape[1]
        up = lambda a: torch.from_numpy(a).to(eng.device).reshape(n, -1)
        pre = {"rope_cos_q": up(odd[0]), "rope_sin_q": up(odd[1]), "rope_cos_k": up(odd[2]), "rope_sin_k": up(odd[3]),
               "cat_mel_text": torch.from_numpy(outs[5]).to(eng.device), "cat_mel_text_drop": torch.from_numpy(outs[6]).to(eng.device),
               "seq_len": torch.tensor([n], dtype=torch.int32, device=eng.device)}
        eng.transformer_steps(x, pre, 0, 1)
    assert np.array_equal(got_odd, x.cpu().numpy())
    assert np.array_equal(run(std), first)                                           # mode restored: computed angles again, same bits
    e.cleanup()


def test_lone_clip_between_half_and_full_fft_runs_end_to_end(tmp_path):
    """_prepare_inputs admits clips of n_fft/2 + 1 samples, vv_preprocess wants an audio plane of at least n_fft columns.
    A request whose ONLY clip is that short used to fail on the GPU path with a generic error: the plane is padded now (device path
    and session path), the item's own length still bounds what the mel front end reads, and both paths agree."""
    from vietvoice_tts_amd.core import AudioProcessor
    e = _engine(tmp_path)
    n_fft = e.model_session_manager.spec.n_fft
    rng = np.random.default_rng(2)
    for n in (n_fft // 2 + 1, n_fft - 1):
        clip = AudioProcessor.to_wav_bytes((rng.standard_normal(n) * 5000).astype(np.int16), 24000)
        ins = e._prepare_inputs(clip, "a", "Xin chào.")
        assert ins[0][0].shape[-1] == n
        import torch
        blk = [torch.randn((int(ins[0][2][0]), 100), generator=torch.Generator().manual_seed(n))]
        w_dev = e._synthesize_device(ins, noise_blocks=blk)[0].reshape(-1)
        outs = e._run_preprocess(*ins[0][:3])
        assert int(outs[7][0]) == n // 256 + 1
        noise = blk[0].numpy()[None]
        m = e.model_session_manager
        ts = ins[0][3]
        for _ in range(e.config.nfe_step - 1):
            noise, ts = m.sessions["transformer"].run(m.output_names["transformer"], dict(zip(m.input_names["transformer"], [noise] + list(outs[1:7]) + [ts])))
        w_ses = e._run_decode(noise, outs[7]).reshape(-1)
        assert w_dev.size == w_ses.size > 0 and int(np.abs(w_dev.astype(np.int32) - w_ses.astype(np.int32)).max()) <= 2
    e.cleanup()


def test_streaming_equals_buffered_on_device(tmp_path):
    """N4: streamed blocks concatenate to the buffered PCM (same seed, one chunk per GPU wave vs all chunks in one batch:
    ragged batching must not change a sequence's result beyond the fp32 summation-order tolerance)."""
    a = _engine(tmp_path)
    whole, _ = a.synthesize(LONG)
    a.cleanup()
    b = _engine(tmp_path)
    blocks = list(b.synthesize_stream(LONG, chunks_per_step=1))
    b.cleanup()
    got = np.concatenate(blocks)
    assert len(blocks) > 1 and got.shape == whole.shape
    assert int(np.abs(got.astype(np.int32) - whole.astype(np.int32)).max()) <= 2


def test_batching_frontend_batch_composition_invariance(tmp_path):
    """N2: a request's audio does not depend on what shared its GPU batch (per-request noise streams, per-item
    reference clips and lengths on the device); different voices ride in one batch."""
    from vietvoice_tts_amd.batching import BatchingFrontend
    e = _engine(tmp_path)
    fe = BatchingFrontend(e, max_wait_ms=300.0, max_requests=8)
    try:
        alone = fe.submit("Xin chào các bạn, hôm nay thế nào?", speed=1.0, serial=7).result(timeout=300)[0]
        n0 = fe.batches_run
        futs = [fe.submit("Tạm biệt và hẹn gặp lại.", speed=1.3, serial=8, gender="male"),
                fe.submit("Xin chào các bạn, hôm nay thế nào?", speed=1.0, serial=7),
                fe.submit(LONG, speed=0.8, serial=9)]
        outs = [f.result(timeout=300)[0] for f in futs]
        assert fe.batches_run == n0 + 1
        assert outs[1].shape == alone.shape and np.array_equal(outs[1], alone)          # bit for bit (round 4; was <= 2 LSB)
        assert all(o.dtype == np.int16 and o.size > 0 for o in outs)
    finally:
        fe.close()
        e.cleanup()


def test_batching_frontend_mixed_request_options_share_one_batch(tmp_path):
    """Four requests whose own options span all ten fields of RequestOptions ride in ONE batch (device noise, so the serial alone names
    a request's noise): each comes back byte for byte as when it was submitted alone with the same serial."""
    from vietvoice_tts_amd.batching import BatchingFrontend
    e = _engine(tmp_path, noise_source="device")
    fe = BatchingFrontend(e, max_wait_ms=500.0, max_requests=8)
    reqs = [dict(text=LONG, speed=0.8, serial=21),
            dict(text="Xin chào các bạn, hôm nay thế nào?", speed=1.0, serial=22, cfg_strength=1.5, cfg_interval=(0.2, 0.9), loudness=-20.0, limiter="true"),
            dict(text="Tạm biệt và hẹn gặp lại.", speed=1.3, serial=23, gender="male", apg_eta=0.0, apg_norm=2.0, pitch=3.0, formants="keep", denoise=1.0),
            dict(text=LONG, speed=1.1, serial=24, tempo=1.25, denoise=2.0, limiter="sample")]
    try:
        alone = [fe.submit(**r).result(timeout=300)[0] for r in reqs]
        n0 = fe.stats()["batches"]
        assert n0 == len(reqs)
        outs = [f.result(timeout=300)[0] for f in [fe.submit(**r) for r in reqs]]
        assert fe.stats()["batches"] == n0 + 1                       # the four really did share a batch
        for i, (got, want) in enumerate(zip(outs, alone)):
            assert got.dtype == np.int16 and got.size > 0 and got.shape == want.shape and np.array_equal(got, want), i
        assert len({o.tobytes() for o in outs}) == 4
    finally:
        fe.close()
        e.cleanup()


def test_batching_frontend_batch_composition_invariance_full_bf16(tmp_path):
    """The same promise at FULL model size in the throughput arithmetic (bf16), where it used to be false (the split-K
    tail made a row's arithmetic depend on its position in the launch, and a request alone takes the 128 x 128 GEMM while a batch of
    >= 4096 rows takes the persistent kernel).  Round 4: tail off, one epilogue arithmetic for both GEMM kernels -- a request ALONE
    and the same request among eleven others (other voices, speeds, lengths; ~25,000 packed rows) give the SAME PCM, bit for bit."""
    from vietvoice_tts_amd.batching import BatchingFrontend
    from vietvoice_tts_amd.core import ModelConfig, TTSEngine
    import bench
    cfg = ModelConfig(model_cache_dir=str(tmp_path), synthetic_model=True, model_spec="full", acoustic_dtype="bf16", nfe_step=32, max_batch_chunks=32)
    e = TTSEngine(cfg)
    fe = BatchingFrontend(e, max_wait_ms=1500.0, max_requests=12)
    try:
        reqs = bench.serve_requests(12)
        alone = [fe.submit(r["text"], speed=r["speed"], serial=r["serial"], **r["voice"]).result(timeout=600)[0] for r in (reqs[3], reqs[8])]
        n0 = fe.batches_run
        futs = [fe.submit(r["text"], speed=r["speed"], serial=r["serial"], **r["voice"]) for r in reqs]
        outs = [f.result(timeout=600)[0] for f in futs]
        assert fe.batches_run == n0 + 1 and fe.stats()["frames_per_batch"] > 0
        for a_, i in zip(alone, (3, 8)):
            assert outs[i].shape == a_.shape and np.array_equal(outs[i], a_), (i, int(np.abs(outs[i].astype(np.int32) - a_.astype(np.int32)).max()))
        assert len({o.size for o in outs}) > 4 and all(o.dtype == np.int16 and int(np.abs(o).max()) > 0 for o in outs)
    finally:
        fe.close()
        e.cleanup()


def test_overlapped_frontend_equals_single_thread_frontend(tmp_path):
    """the pipelined front end (host preparation of batch n + 1 and the cross-fades of batch n - 1 overlap the GPU work
    of batch n; the waiting batch keeps filling while the GPU is busy) returns the same PCM as the one-thread loop for fixed request
    serials, whatever batches the requests end up in -- 14 requests from 5 client threads, at most 4 per batch."""
    import threading
    from vietvoice_tts_amd.batching import BatchingFrontend
    import bench
    reqs = bench.serve_requests(14)
    results = {}
    for overlap in (False, True):
        e = _engine(tmp_path)
        fe = BatchingFrontend(e, max_wait_ms=20.0, max_requests=4, overlap=overlap)
        got, lock, nxt = {}, threading.Lock(), [0]

        def client():
            while True:
                with lock:
                    i = nxt[0]
                    nxt[0] += 1
                if i >= len(reqs):
                    return
                r = reqs[i]
                w = fe.submit(r["text"], speed=r["speed"], serial=r["serial"], **r["voice"]).result(timeout=600)[0]
                with lock:
                    got[i] = w
        ths = [threading.Thread(target=client) for _ in range(5)]
        for t in ths:
            t.start()
        for t in ths:
            t.join(600)
        st = fe.stats()
        fe.close()
        e.cleanup()
        assert len(got) == len(reqs) and st["requests"] == len(reqs) and st["batches"] >= 4
        results[overlap] = got
    for i in range(len(reqs)):
        assert np.array_equal(results[True][i], results[False][i]), i


def test_engine_outputs_match_the_engine_on_oracle_sessions(tmp_path):
    """a5 / N4 / N2 against the ORACLE rather than against another HIP run.  The same TTSEngine class driven by oracle sessions (CPU
    fp32 restatement, the reference's one-chunk-at-a-time session pattern) and by the HIP path from the same seed -- same chunk plan,
    same noise stream -- must give the same PCM within the fp32 tolerance of the e2e tests (+-2 LSB): (a5) all chunks as one ragged
    GPU batch, (N4) streamed one chunk per wave, (N2) a request through the batching front end, whose noise stream is seeded by
    (random_seed, serial): the oracle is fed the same blocks chunk by chunk and its waves are joined by the same cross-fade."""
    import torch
    from vietvoice_tts_amd.batching import BatchingFrontend
    from vietvoice_tts_amd.core import ModelConfig, TTSEngine
    from oracle.vv_oracle import Oracle, OracleSession
    holder = {}

    def factory(spec, weights, config):
        holder["oracle"] = Oracle(spec, weights, nfe_step=config.nfe_step)
        return {k: OracleSession(holder["oracle"], k, seed=config.random_seed) for k in ("preprocess", "transformer", "decode")}
    cfg = ModelConfig(model_cache_dir=str(tmp_path), synthetic_model=True, model_spec="tiny", nfe_step=5, acoustic_dtype="fp32", max_chunk_duration=8.0)
    ora = TTSEngine(cfg, session_factory=factory)
    want, _ = ora.synthesize(LONG)

    def close(a, b):
        assert a.shape == b.shape, (a.shape, b.shape)
        d = np.abs(a.astype(np.int32) - b.astype(np.int32))
        assert int(d.max()) <= 2 and float((d > 1).mean()) < 1e-3, (int(d.max()), float((d > 1).mean()))
    e = _engine(tmp_path)
    got, _ = e.synthesize(LONG)                                  # a5: every chunk in one ragged GPU batch
    assert len(e._last_plan) > 1
    close(got, want)
    e.cleanup()
    e = _engine(tmp_path)
    blocks = list(e.synthesize_stream(LONG, chunks_per_step=1))  # N4: streamed, one chunk per wave
    assert len(blocks) > 1
    close(np.concatenate(blocks), want)
    e.cleanup()
    # N2
    text, serial = "Xin chào các bạn, hôm nay thế nào? Tôi rất vui được gặp bạn.", 3
    e = _engine(tmp_path)
    fe = BatchingFrontend(e, max_wait_ms=200.0, max_requests=4)
    try:
        futs = [fe.submit(text, speed=1.0, serial=serial), fe.submit("Tạm biệt và hẹn gặp lại.", speed=1.3, serial=4, gender="male")]
        out = futs[0].result(timeout=300)[0]
        futs[1].result(timeout=300)
    finally:
        fe.close()
        e.cleanup()
    orc = holder["oracle"]
    ref_clip, ref_txt = ora.model_session_manager.select_sample()
    inputs = ora._prepare_inputs(ref_clip, ref_txt, text, speed=1.0)
    gen = torch.Generator().manual_seed(cfg.random_seed * 1000003 + serial)          # batching.py: the request's own noise stream
    waves = []
    for audio, ids, max_dur, _ts in inputs:
        n = int(max_dur[0])
        noise = torch.randn((n, orc.spec.n_mel), generator=gen, dtype=torch.float32)
        _x, pcm = orc.synthesize(torch.from_numpy(np.asarray(audio).reshape(-1)), torch.from_numpy(np.asarray(ids).reshape(-1)), n, noise)
        waves.append(pcm.numpy().astype(np.int16).reshape(-1))
    joined = ora.audio_processor.concatenate_with_crossfade_improved(waves, cfg.cross_fade_duration, cfg.sample_rate)
    ora.cleanup()
    close(out, np.asarray(joined).reshape(-1))


def test_voice_bank_cache_and_parity(tmp_path):
    """N3: clips are ingested once (GPU mono mix + rate conversion + normalise), served from HBM afterwards, EQUAL to the host
    loader (both are the reference's arithmetic), and the engine output through the bank equals the output with host-loaded clips."""
    from vietvoice_tts_amd.core import AudioProcessor
    e = _engine(tmp_path)
    bank = e.voice_bank
    assert bank is not None
    rng = np.random.default_rng(11)
    wav48 = AudioProcessor.to_wav_bytes((rng.standard_normal(48000 * 2) * 6000).astype(np.int16), 48000)
    wav24 = AudioProcessor.to_wav_bytes((rng.standard_normal(24000 * 3) * 2000 + 300).astype(np.int16), 24000)
    p = tmp_path / "clip.wav"
    p.write_bytes(wav24)
    ents = bank.ingest_many([wav48, str(p), wav48])
    assert bank.misses == 2 and bank.hits == 1 and ents[0] is ents[2]
    for ent, src in ((ents[0], wav48), (ents[1], wav24)):
        want = AudioProcessor.load_audio(src, 24000)
        assert ent.pcm_host.shape == want.shape and ent.pcm_dev.is_cuda
        assert np.array_equal(ent.pcm_host, want)
        assert np.array_equal(ent.pcm_dev.cpu().numpy(), ent.pcm_host)
    with pytest.raises(FileNotFoundError):
        bank.get(str(tmp_path / "missing.wav"))
    # engine: second call with the same voice is a pure cache hit and reproduces the first call's audio given the same noise
    m0 = bank.misses
    ref, txt = e.model_session_manager.select_sample()
    ins = e._prepare_inputs(ref, txt, "Xin chào các bạn.")
    assert bank.misses == m0 + 1 and bank.entry_for_host(ins[0][0]) is not None
    ins2 = e._prepare_inputs(ref, txt, "Xin chào các bạn.")
    assert bank.misses == m0 + 1 and ins2[0][0].base is ins[0][0].base
    import torch
    blk = [torch.randn((int(ins[0][2][0]), 100), generator=torch.Generator().manual_seed(3))]
    w_bank = e._synthesize_device(ins, noise_blocks=blk)[0]
    host_ins = [(AudioProcessor.load_audio(ref, 24000).reshape(1, 1, -1),) + tuple(ins[0][1:])]
    assert bank.entry_for_host(host_ins[0][0]) is None
    w_host = e._synthesize_device(host_ins, noise_blocks=blk)[0]
    e.cleanup()
    assert np.array_equal(host_ins[0][0].reshape(-1), ins[0][0].reshape(-1))          # same int16 clip either way ...
    assert w_bank.shape == w_host.shape and np.array_equal(w_bank, w_host)            # ... so the same audio, bit for bit


def test_engine_from_reference_layout_onnx_archive(tmp_path):
    """N1: an archive in the reference's layout (preprocess/transformer/decode .onnx, no model_spec.json) goes through the
    protobuf reader -> name recovery -> shape-inferred spec -> device weight pack, and the HIP engine produces the very
    PCM the synthetic pack with the same weights produces.  (The real archive's naming is unpinned: see onnx_import.py.)"""
    import tarfile
    from vietvoice_tts_amd import onnx_import as oi
    from tests import onnx_fixture_writer as ow
    from vietvoice_tts_amd.model_spec import ModelSpec, make_synthetic_weights
    a = _engine(tmp_path)
    wa, _ = a.synthesize("Xin chào các bạn.")
    a.cleanup()
    d2 = tmp_path / "onnx"
    d2.mkdir()
    members = {}
    with tarfile.open(tmp_path / "model-bin.pt") as tar:
        for n in tar.getnames():
            if n != "model_spec.json":
                members[n] = tar.extractfile(n).read()
    spec = ModelSpec.tiny()
    ow.write_onnx_archive(str(d2 / "model-bin.pt"), spec, make_synthetic_weights(spec, 9527), members)
    b = _engine(d2)
    assert b.model_session_manager.spec == spec
    wb, _ = b.synthesize("Xin chào các bạn.")
    b.cleanup()
    assert np.array_equal(wa, wb)


def test_bench_json_contract():
    """bench.py --full prints ONE JSON line with the contract's keys (tiny model, 1 step: this checks the plumbing, not speed)."""
    import json, os, subprocess, sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    r = subprocess.run([sys.executable, os.path.join(root, "bench.py"), "--spec", "tiny", "--steps", "1", "--warmup", "0", "--batch", "4", "--full"],
                       capture_output=True, text=True, timeout=600, cwd=root)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1
    d = json.loads(lines[0])
    for k in ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling", "vs_baseline", "dtype", "data",
              "config", "roofline", "cpu_baseline"):
        assert k in d, k
    assert d["n_gpus"] == 1 and d["steps"] == 1 and d["warmup"] == 0 and d["higher_is_better"] is True and d["scaling"] == "weak"
    assert d["vs_baseline"] is None and d["unit"] == "audio-seconds/sec" and d["value"] > 0 and "workload" in d["config"]
    rf, cb = d["roofline"], d["cpu_baseline"]
    assert set(("bound", "achieved", "peak", "unit", "frac", "traffic")) <= set(rf) and rf["bound"] in ("hbm", "mfma") and 0 < rf["frac"] < 1
    assert abs(rf["frac"] - rf["achieved"] / rf["peak"]) < 1e-3
    assert set(("value", "unit", "cores", "kind", "sample")) <= set(cb) and cb["kind"] in ("port", "reference") and cb["cores"] >= 1
    assert d["median_ms_per_step"] > 0 and "resident in HBM" in d["timed_region"] and "hbm_target_note" in d
    pi = d["pcie_inclusive"]                       # the same step with its PCIe legs, beside `value`, never as `value`
    assert pi["value"] > 0 and pi["steps"] >= 1 and "H2D" in pi["what"] and "D2H" in pi["what"]
    ln = d["lanes"]                                # the class times come from a one-lane pass and add up to (at most) that pass's wall time
    assert ln["option"] == 0 and ln["class_pass_ms"] > 0 and sum(v["ms"] for v in d["kernel_classes"].values()) <= ln["class_pass_ms"] * 1.02
    vs = d["vocoder_stages"]                       # the vocoder convs once more by stage: every launch of voc_conv in exactly one stage
    assert set(vs) == {"voc_pre"} | {f"voc_up{i}" for i in range(4)} | {f"voc_mrf{i}" for i in range(4)}
    assert sum(v["launches"] for v in vs.values()) == d["kernel_classes"]["voc_conv"]["launches"]
    assert abs(sum(v["ms"] for v in vs.values()) - d["kernel_classes"]["voc_conv"]["ms"]) <= 0.02 * d["kernel_classes"]["voc_conv"]["ms"] + 0.05
    assert "resident in HBM" in d["value_definition"]


def test_bench_plain_run_times_its_steps_and_dumps_outputs(tmp_path):
    """A plain run (no --full) times exactly --steps steps, prints the headline keys only, and --dump-outputs writes what the timed
    call returned in its last step: the mel state, the PCM and its lengths, float32 / float64, within 64 MB."""
    import json, os, subprocess, sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    out = tmp_path / "outputs"
    r = subprocess.run([sys.executable, os.path.join(root, "bench.py"), "--spec", "tiny", "--steps", "2", "--warmup", "1", "--batch", "4",
                        "--dump-outputs", str(out)], capture_output=True, text=True, timeout=600, cwd=root)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1
    d = json.loads(lines[0])
    assert d["steps"] == 2 and d["warmup"] == 1 and d["ms_per_step"] > 0 and d["value"] > 0 and d["higher_is_better"] is True
    assert d["unit"] == "audio-seconds/sec" and d["dtype"] == "bf16" and d["metric"].startswith("audio-seconds/sec")
    assert abs(d["value"] * d["ms_per_step"] * 1e-3 - 4 * 1037 * 256 / 24000.0) < 0.01 * 4 * 1037 * 256 / 24000.0
    for k in ("cpu_baseline", "pcie_inclusive", "roofline", "kernel_classes", "vocoder_stages", "lanes"):
        assert k not in d, k
    files = sorted(os.listdir(out))
    assert files == ["mel.npy", "pcm.npy", "pcm_len.npy"], files
    a = {f[:-4]: np.load(out / f) for f in files}
    assert sum(os.path.getsize(out / f) for f in files) <= 64 * 10 ** 6
    assert a["mel"].dtype == np.float32 and a["mel"].shape == (4, 1600, 100) and np.isfinite(a["mel"]).all()
    assert a["pcm"].dtype == np.float32 and a["pcm"].shape == (4, 1037 * 256) and np.abs(a["pcm"]).max() > 0
    assert np.array_equal(a["pcm"], np.round(a["pcm"])) and np.abs(a["pcm"]).max() <= 32768
    assert a["pcm_len"].dtype == np.float64 and a["pcm_len"].tolist() == [1037 * 256] * 4


def test_bench_serve_workload_contract():
    """`bench.py --workload serve` (SURVEY 8f N2 measured) stays alive: tiny model, 12 requests from 4 client threads; one JSON line with
    the serial leg (the reference REST layer's behaviour), the pipelined and the one-thread front end, each with rates, latency
    percentiles and -- for the front ends -- batch fill and GPU-busy fraction; every request served in every leg."""
    import json, os, subprocess, sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    r = subprocess.run([sys.executable, os.path.join(root, "bench.py"), "--workload", "serve", "--spec", "tiny", "--nfe", "5", "--dtype", "fp32",
                        "--requests", "12", "--serial-requests", "4", "--clients", "4", "--batch", "8"],
                       capture_output=True, text=True, timeout=900, cwd=root)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1
    d = json.loads(lines[0])
    assert d["unit"] == "audio-seconds/sec" and d["value"] == d["frontend_overlapped"]["audio_s_per_s"] > 0 and "serve" in d["config"]["workload"]
    assert d["serial"]["requests"] == 4 and d["serial"]["latency_p50_ms"] > 0
    for k in ("frontend_overlapped", "frontend_single_thread"):
        v = d[k]
        assert v["requests"] == 12 and v["audio_s_per_s"] > 0 and v["latency_p95_ms"] >= v["latency_p50_ms"] > 0
        assert 1 <= v["requests_per_batch"] <= 8 and 0 < v["gpu_busy_frac"] <= 1.0 and v["batches"] >= 2


def test_bench_two_rank_branch_over_gloo():
    """The N > 1 branch of bench.py (rendezvous, rank-0 weight pack + broadcast, barriers, MAX-over-ranks time, SUM of audio, one
    JSON line on rank 0) kept alive without multi-GPU hardware: two ranks under torch.distributed.run share cuda:0 with
    VV_BENCH_DIST_BACKEND=gloo.  Started as a FRESH child process tree (this test process never execs; the children initialise
    the GPU themselves).  RCCL over xGMI itself stays unmeasured until the driver's 8-GPU run."""
    import json, os, socket, subprocess, sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    with socket.socket() as sk:
        sk.bind(("127.0.0.1", 0))
        port = sk.getsockname()[1]
    env = dict(os.environ, VV_BENCH_DIST_BACKEND="gloo", MASTER_ADDR="127.0.0.1", HSA_ENABLE_IPC_MODE_LEGACY="0")
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2", "--master-addr", "127.0.0.1",
           "--master-port", str(port), os.path.join(root, "bench.py"), "--gpus", "2", "--spec", "tiny", "--steps", "1", "--warmup", "0", "--batch", "4"]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=900, cwd=root, env=env)
    assert r.returncode == 0, (r.stdout[-1500:], r.stderr[-3000:])
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, r.stdout[-2000:]                       # rank 0 only
    d = json.loads(lines[0])
    assert d["n_gpus"] == 2 and d["scaling"] == "weak" and d["config"]["global_batch"] == 8 and "dp2" in d["config"]["parallelism"]
    assert d["weight_pack_and_broadcast_ms"] > 0 and "cpu_baseline" not in d         # cpu_baseline is an N = 1 leg
    per_rank_audio = 4 * 1037 * 256 / 24000.0
    assert abs(d["value"] * d["ms_per_step"] * 1e-3 - 2 * per_rank_audio) < 0.02 * per_rank_audio      # value = SUM of audio over ranks / MAX time
    assert len(d["devices"]) == 2 and d["devices"][0].startswith("rank 0: cuda:") and d["devices"][1].startswith("rank 1: cuda:")
    # the form the driver uses for N = 1, with N = 2 and NO launcher: bench.py must start the two ranks itself (a child
    # torch.distributed.run), not run one rank and label it --gpus 2
    env2 = {k: v for k, v in env.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_PORT")}
    r2 = subprocess.run([sys.executable, os.path.join(root, "bench.py"), "--gpus", "2", "--spec", "tiny", "--steps", "1", "--warmup", "0", "--batch", "4"],
                        capture_output=True, text=True, timeout=900, cwd=root, env=env2)
    assert r2.returncode == 0, (r2.stdout[-1500:], r2.stderr[-3000:])
    lines2 = [l for l in r2.stdout.splitlines() if l.startswith("{")]
    assert len(lines2) == 1, r2.stdout[-2000:]
    d2 = json.loads(lines2[0])
    assert d2["n_gpus"] == 2 and d2["config"]["global_batch"] == 8 and len(d2["devices"]) == 2 and d2["weight_pack_and_broadcast_ms"] > 0
    # a launcher whose rank count disagrees with --gpus is refused, not silently relabelled
    bad = subprocess.run(cmd[:cmd.index("--gpus") + 1] + ["3"] + cmd[cmd.index("--gpus") + 2:], capture_output=True, text=True, timeout=600, cwd=root, env=env)
    assert bad.returncode != 0 and not [l for l in bad.stdout.splitlines() if l.startswith("{")]


@pytest.mark.parametrize("workload", ["batch32", "mixed256"])
def test_bench_multi_rank_rehearsal_both_workloads(workload):
    """the exact `python bench.py --gpus N` command the driver's scaling run issues, rehearsed without an N-GPU node:
    NO launcher (bench.py starts its ranks as a fresh child process tree), tiny spec, gloo, ranks sharing cuda:0 -- for the headline
    workload and for configs[3]'s LPT-sharded ragged units.  World 4, not 8: a GPU box of this pool admits at most 6 processes on its
    card and this pytest process is one of them (the 8-rank shard plan itself is covered on the CPU: tests/test_multirank_cpu.py).
    Checked: n_gpus, one JSON line, every rank's own ms and shard in it, the shard imbalance, value = SUM audio / MAX time, and that the
    HSA_ENABLE_IPC_MODE_LEGACY default of the self-launch can be overridden from the environment.  RCCL over xGMI: unmeasured on hardware."""
    import json, os, subprocess, sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    W = 4
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_PORT", "HSA_ENABLE_IPC_MODE_LEGACY")}
    env["VV_BENCH_DIST_BACKEND"] = "gloo"
    cmd = [sys.executable, os.path.join(root, "bench.py"), "--gpus", str(W), "--spec", "tiny", "--steps", "1", "--warmup", "0", "--batch", "4",
           "--workload", workload]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=900, cwd=root, env=env)
    assert r.returncode == 0, (r.stdout[-1500:], r.stderr[-3000:])
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, r.stdout[-2000:]
    d = json.loads(lines[0])
    assert d["n_gpus"] == W and d["scaling"] == "weak" and d["config"]["global_batch"] == 4 * W and f"dp{W}" in d["config"]["parallelism"]
    assert len(d["devices"]) == W and [p["rank"] for p in d["per_rank"]] == list(range(W))
    assert all(p["ms_per_step"] > 0 and p["units"] >= 1 and p["rows"] > 0 for p in d["per_rank"])
    assert sum(p["units"] for p in d["per_rank"]) == 4 * W                                   # every unit on exactly one rank
    assert abs(d["value"] * d["ms_per_step"] * 1e-3 - sum(p["audio_s"] for p in d["per_rank"])) < 0.02 * sum(p["audio_s"] for p in d["per_rank"])
    im = d["shard_imbalance"]
    assert 1.0 <= im["rows_max_over_mean"] < (1.001 if workload == "batch32" else 1.5) and im["ms_max_over_mean"] >= 1.0
    assert d["env"]["HSA_ENABLE_IPC_MODE_LEGACY"] == "0"                                      # the self-launch's default (dmabuf IPC) ...
    if workload == "batch32":
        env["HSA_ENABLE_IPC_MODE_LEGACY"] = "1"                                               # ... yields to the caller's environment
        r2 = subprocess.run(cmd[:cmd.index("--gpus") + 1] + ["2"] + cmd[cmd.index("--gpus") + 2:], capture_output=True, text=True, timeout=900, cwd=root, env=env)
        assert r2.returncode == 0, (r2.stdout[-1500:], r2.stderr[-3000:])
        d2 = json.loads([l for l in r2.stdout.splitlines() if l.startswith("{")][0])
        assert d2["n_gpus"] == 2 and d2["env"]["HSA_ENABLE_IPC_MODE_LEGACY"] == "1"


@pytest.mark.parametrize("graph", [False, True])
def test_concurrent_callers_on_one_engine(tmp_path, graph):
    """The REST layer enters one engine from worker threads (/root/reference/vietvoicetts/api/tts_engine.py:64-91: config.speed is
    set, `synthesize_to_bytes` runs under anyio.to_thread, speed is restored; concurrent test: /root/reference/tests/
    test_api_integration.py:148-176).  Four threads call `synthesize` on ONE HIP engine -- two voices, two speeds set by mutating
    `config.speed` the way the REST layer does.  No exception, no deadlock; and because the engine serialises the GPU work, every
    result must equal the same request replayed SERIALLY on a fresh engine in the order in which the threads got the lock (the
    seeded noise stream makes the order matter: it is recorded, not assumed)."""
    import threading
    reqs = [dict(text="Xin chào các bạn, hôm nay trời đẹp quá.", gender="female", speed=0.9),
            dict(text="Chúng ta cùng nhau đi dạo quanh hồ nhé.", gender="male", speed=1.2),
            dict(text=LONG, gender="female", speed=1.2),
            dict(text="Cảm ơn rất nhiều.", gender="male", speed=0.9)]
    eng = _engine(tmp_path, max_batch_chunks=2, use_hip_graph=graph)
    order, results, errors = [], {}, []
    tl = threading.local()
    mut = threading.Lock()                  # the REST layer's event loop is single-threaded: its config mutations do not interleave
    orig_select, orig_prepare = eng.model_session_manager.select_sample, eng._prepare_inputs

    def select(*a, **k):                    # called right after `synthesize` has read config.speed
        tl.entered.set()
        return orig_select(*a, **k)

    def prepare(*a, **k):                   # called under the engine lock: the order of GPU work
        order.append(tl.rid)
        return orig_prepare(*a, **k)
    eng.model_session_manager.select_sample, eng._prepare_inputs = select, prepare

    def worker(rid, entered):
        tl.rid, tl.entered = rid, entered
        try:
            results[rid] = eng.synthesize(reqs[rid]["text"], gender=reqs[rid]["gender"])[0]
        except Exception as e:            # noqa: BLE001
            errors.append((rid, repr(e)))
            entered.set()
    threads = []
    for rid, r in enumerate(reqs):
        with mut:
            entered = threading.Event()
            saved, eng.config.speed = eng.config.speed, r["speed"]
            t = threading.Thread(target=worker, args=(rid, entered), name=f"req{rid}")
            t.start()
            assert entered.wait(60)
            eng.config.speed = saved
        threads.append(t)
    for t in threads:
        t.join(120)
        assert not t.is_alive(), "deadlock: a caller never returned"
    eng.cleanup()
    assert not errors, errors
    assert sorted(order) == [0, 1, 2, 3] and len(results) == 4
    # serial replay in the recorded order on a fresh engine (same seed -> same noise stream)
    ser = _engine(tmp_path, max_batch_chunks=2, use_hip_graph=graph)
    for rid in order:
        ser.config.speed = reqs[rid]["speed"]
        w, _ = ser.synthesize(reqs[rid]["text"], gender=reqs[rid]["gender"])
        assert w.shape == results[rid].shape and np.array_equal(w, results[rid]), f"request {rid} differs from its serial replay"
    ser.cleanup()
    assert len({r.size for r in results.values()}) >= 3           # different texts / speeds really produced different audio


def test_decode_graph_cache_is_bounded(tmp_path):
    """captured decode graphs are kept in an LRU of `decode_graph_cache_entries` entries sharing ONE workspace block;
    a service with varied reference clips cannot grow HBM without limit.  Results do not depend on eviction."""
    from vietvoice_tts_amd.runtime import DecodeGraphCache
    texts = ["Xin chào.", "Xin chào các bạn, hôm nay trời đẹp quá, chúng ta đi dạo nhé.", LONG, "Cảm ơn rất nhiều, hẹn gặp lại các bạn vào ngày mai nhé."]
    a = _engine(tmp_path, max_batch_chunks=2, use_hip_graph=True, decode_graph_cache_entries=2)
    wa = [a.synthesize(t)[0] for t in texts + texts]
    c = a._decode_graphs
    assert isinstance(c, DecodeGraphCache) and len(c) <= 2 and c.evictions >= 1 and c.misses >= 3
    blocks = {g.ws.data_ptr(): g.ws.numel() for g in c._graphs.values()}
    # one shared workspace block, replaced only when a key needs a larger one (a graph captured on the old block keeps it until it
    # is evicted): never more blocks than live graphs, and the newest graph sits on the cache's current block
    assert len(blocks) <= len(c) and c._ws.data_ptr() in blocks and c.pinned_bytes() <= a.config.decode_graph_cache_bytes
    assert c.pinned_bytes() == sum(blocks.values()) + sum(g.io_bytes() for g in c._graphs.values())
    a.cleanup()
    b = _engine(tmp_path, max_batch_chunks=2, use_hip_graph=True, decode_graph_cache_entries=64)
    wb = [b.synthesize(t)[0] for t in texts + texts]
    assert b._decode_graphs.evictions == 0
    b.cleanup()
    for x, y in zip(wa, wb):
        assert np.array_equal(x, y)
