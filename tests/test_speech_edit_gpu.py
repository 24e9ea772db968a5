"""-m gpu: speech editing through the C ABI against the CPU oracle.  The oracle side is written here from the
oracle's pieces (mel, text_embed, rope_tables, transformer_step, vocoder, to_pcm) with its own numpy splice and frame mask; it
never calls the product planner.  Tolerances are those of tests/test_e2e_gpu.py."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
HOP = 256


def own_edit(S, edits):
    """edits [(a, b, g)]: source samples [a, b) (a on the hop grid) become g frames of gap -> (segments (src_off, dst_off, n), L, keep)."""
    segs, gaps = [], []
    src = dst = 0
    for a, b, g in edits:
        segs.append((src, dst, a - src))
        dst += a - src
        gaps.append((dst // HOP, dst // HOP + g))
        dst += g * HOP
        src = b
    segs.append((src, dst, S - src))
    L = dst + S - src
    keep = np.ones(L // HOP + 1, dtype=np.uint8)
    for f0, f1 in gaps:
        keep[f0:f1] = 0
    return segs, L, keep


def np_splice(src, segs, L):
    out = np.zeros(L, dtype=np.int16)
    for so, do, n in segs:
        out[do: do + n] = src[so: so + n]
    return out


def make_edits(spec, items, seed):
    """items: [(S, edits, text_len)] -> host and device inputs of one edit batch."""
    rng = np.random.default_rng(seed)
    g = torch.Generator().manual_seed(seed)
    srcs = [(rng.standard_normal(S) * 3000).astype(np.int16) for S, _e, _t in items]
    base = np.concatenate([[0], np.cumsum([s.size for s in srcs])]).astype(np.int64)
    rows, Ls, keeps, spliced, ids = [], [], [], [], []
    for b, ((S, edits, T), src) in enumerate(zip(items, srcs)):
        segs, L, keep = own_edit(S, edits)
        rows += [[b, int(base[b]) + so, do, n] for so, do, n in segs]
        Ls.append(L)
        keeps.append(keep)
        spliced.append(np_splice(src, segs, L))
        ids.append(torch.randint(0, spec.vocab_size, (T,), generator=g, dtype=torch.int32))
    B, N, T = len(items), max(k.size for k in keeps), max(t.numel() for t in ids)
    keep = np.zeros((B, N), dtype=np.uint8)
    ids_pad = torch.zeros((B, T), dtype=torch.int32)
    for b in range(B):
        keep[b, : keeps[b].size] = keeps[b]
        ids_pad[b, : ids[b].numel()] = ids[b]
    noise = torch.randn((B, N, spec.n_mel), generator=g)
    return dict(src=torch.from_numpy(np.concatenate(srcs)), rows=rows, L=Ls, keep=keep, spliced=spliced, ids=ids, ids_pad=ids_pad,
                text_len=torch.tensor([t.numel() for t in ids], dtype=torch.int32), noise=noise, N=N)


def dev_args(e):
    return (e["src"].to(DEV), e["rows"], e["L"], e["ids_pad"].to(DEV), e["text_len"].to(DEV), torch.from_numpy(e["keep"]).to(DEV))


def run_stages(eng, e, n_steps):
    """The edit stage by stage through the runtime (what edit_batch chains), keeping the conditioning and the waveform."""
    src, rows, L, ids, tl, keep = dev_args(e)
    mal = max(max(L), eng.spec.n_fft)
    audio = eng.edit_splice(src, rows, len(L), (mal + 3) // 4 * 4)
    frames = [v // HOP + 1 for v in L]
    i32 = lambda v: torch.tensor(v, dtype=torch.int32, device=DEV)
    pre = eng.preprocess_edit(audio, i32(L), ids, tl, i32(frames), e["N"], keep, L, max_audio_len=mal, seq_len_host=frames)
    x = e["noise"].to(DEV)
    eng.transformer_steps(x, pre, 0, n_steps)
    eng.edit_restore(x, pre, keep)
    pcm, _len, wave = eng.decode(x, pre, e["N"], want_wave=True)
    torch.cuda.synchronize()
    return pre, x.cpu(), pcm.cpu(), wave.cpu()


def run_oracle(orc, e, n_steps):
    outs = []
    M = orc.spec.n_mel
    for b, L in enumerate(e["L"]):
        n = L // HOP + 1
        keep = torch.from_numpy(e["keep"][b, :n].astype(bool))
        mel = orc.mel(torch.from_numpy(e["spliced"][b]))
        assert mel.shape == (n, M)
        cond = torch.where(keep[:, None], mel, torch.zeros_like(mel))
        cq, sq, ck, sk = orc.rope_tables(n)
        pre = {"rope_cos_q": cq, "rope_sin_q": sq, "rope_cos_k": ck, "rope_sin_k": sk,
               "cat_mel_text": torch.cat([cond, orc.text_embed(e["ids"][b], n, drop=False)], dim=-1),
               "cat_mel_text_drop": torch.cat([torch.zeros_like(cond), orc.text_embed(e["ids"][b], n, drop=True)], dim=-1)}
        x = e["noise"][b, :n].clone()
        for st in range(n_steps):
            x = orc.transformer_step(x, pre, st)
        x = torch.where(keep[:, None], cond, x)
        wave = orc.vocoder(x)
        outs.append(dict(pre=pre, x=x, wave=wave, pcm=orc.to_pcm(wave)))
    return outs


# two ragged items: a middle span regenerated longer, and a deletion next to an insertion
TWO = [(256 * 40 + 77, [(256 * 12, 256 * 20, 11)], 30), (256 * 28, [(256 * 6, 256 * 9, 0), (256 * 15, 256 * 15, 5)], 21)]


def test_splice_kernel_equals_numpy_splice(hip_tiny, tiny_setup):
    spec, _, _ = tiny_setup
    eng = hip_tiny["f32"]
    S2 = 256 * 30 + 123
    items = [(256 * 40 + 77, [(256 * 12, 256 * 20, 0)], 5),                 # deletion
             (256 * 25, [(0, 0, 7), (256 * 10, 256 * 10, 3)], 5),            # insertions, one at 0
             (S2, [(256 * 22, 256 * 30, 9)], 5)]                              # edit to the end: the partial hop of 123 samples stays
    e = make_edits(spec, items, seed=1)
    assert e["rows"][-1][3] == 123
    ld = (max(e["L"]) + 3) // 4 * 4 + 64
    out = eng.edit_splice(e["src"].to(DEV), e["rows"], 3, ld).cpu().numpy()
    for b, L in enumerate(e["L"]):
        assert np.array_equal(out[b, :L], e["spliced"][b]), b
        assert not out[b, L:].any(), b                                        # zeros past L_b
    with pytest.raises(ValueError):                                           # refused on the host, nothing launched
        eng.edit_splice(e["src"].to(DEV), [[0, e["src"].numel() - 10, 0, 11]], 1, ld)
    with pytest.raises(ValueError):
        eng.edit_splice(e["src"].to(DEV), [[0, 0, 0, 100], [0, 500, 99, 10]], 1, ld)


def test_preprocess_edit_is_preprocess_with_masked_mel(hip_tiny, tiny_setup):
    spec, _, _ = tiny_setup
    M = spec.n_mel
    for dt in ("f32", "bf16"):
        eng = hip_tiny[dt]
        e = make_edits(spec, TWO + [(256 * 33 + 5, [(256 * 30, 256 * 33, 4)], 17)], seed=2)
        B, N, L = 3, e["N"], e["L"]
        mal = max(max(L), spec.n_fft)
        audio = torch.zeros((B, mal), dtype=torch.int16)
        for b in range(B):
            audio[b, : L[b]] = torch.from_numpy(e["spliced"][b])
        frames = [v // HOP + 1 for v in L]
        i32 = lambda v: torch.tensor(v, dtype=torch.int32, device=DEV)
        keep = torch.from_numpy(e["keep"]).to(DEV)
        args = (audio.to(DEV), i32(L), e["ids_pad"].to(DEV), e["text_len"].to(DEV), i32(frames), N)
        ref = eng.preprocess(*args, audio_len_host=L)
        got = eng.preprocess_edit(*args, keep, L)
        torch.cuda.synchronize()
        want = ref["cat_mel_text"].clone()
        want[..., :M] = torch.where(keep[..., None].bool(), want[..., :M], torch.zeros_like(want[..., :M]))
        assert torch.equal(got["cat_mel_text"], want), dt
        assert torch.equal(got["cat_mel_text_drop"], ref["cat_mel_text_drop"]), dt
        assert not got["ref_signal_len"].any() and torch.equal(ref["ref_signal_len"].cpu(), torch.tensor(frames, dtype=torch.int32))


def test_fp32_edit_matches_oracle(hip_tiny, tiny_setup):
    spec, _, orc = tiny_setup
    eng = hip_tiny["f32"]
    M = spec.n_mel
    e = make_edits(spec, TWO, seed=3)
    pre, x, pcm, wave = run_stages(eng, e, 7)
    ref = run_oracle(orc, e, 7)
    for b, r in enumerate(ref):
        n = e["L"][b] // HOP + 1
        cat = pre["cat_mel_text"][b, :n].cpu()
        rc = r["pre"]["cat_mel_text"]
        assert float((cat[:, :M] - rc[:, :M]).abs().max()) < 2e-3
        assert float((cat[:, M:] - rc[:, M:]).abs().max()) < 2e-3 * float(rc[:, M:].abs().max())
        catd = pre["cat_mel_text_drop"][b, :n].cpu()
        assert float((catd - r["pre"]["cat_mel_text_drop"]).abs().max()) < 2e-3 * float(r["pre"]["cat_mel_text_drop"].abs().max())
        err_x = float((x[b, :n] - r["x"]).abs().max()) / float(r["x"].abs().max())
        assert err_x < 1e-3, err_x
        assert float((wave[b, : n * HOP] - r["wave"]).abs().max()) < 2e-4
        assert int((pcm[b, : n * HOP].int() - r["pcm"].int()).abs().max()) <= 2
    # edit_batch chains the same stages: the same state and PCM
    xb, pcmb, lenb = eng.edit_batch(*dev_args(e), e["noise"].to(DEV), n_steps=7)
    torch.cuda.synchronize()
    assert torch.equal(xb.cpu(), x) and torch.equal(pcmb.cpu(), pcm) and lenb.cpu().tolist() == e["L"]


def test_bf16_edit_close_to_oracle(hip_tiny, tiny_setup):
    spec, _, orc = tiny_setup
    e = make_edits(spec, TWO, seed=4)
    _pre, x, _pcm, wave = run_stages(hip_tiny["bf16"], e, 7)
    for b, r in enumerate(run_oracle(orc, e, 7)):
        n = e["L"][b] // HOP + 1
        d = x[b, :n] - r["x"]
        rmse = float(d.pow(2).mean().sqrt() / r["x"].pow(2).mean().sqrt())
        assert rmse < 2e-2, rmse
        wr = float((wave[b, : n * HOP] - r["wave"]).pow(2).mean().sqrt() / r["wave"].pow(2).mean().sqrt())
        assert wr < 0.1, wr


def test_restore_is_exact(hip_tiny, tiny_setup):
    spec, _, orc = tiny_setup
    M = spec.n_mel
    eng = hip_tiny["f32"]
    e = make_edits(spec, TWO, seed=5)
    pre, x, _pcm, _wave = run_stages(eng, e, 7)
    for b, L in enumerate(e["L"]):
        n = L // HOP + 1
        k = torch.from_numpy(e["keep"][b, :n].astype(bool))
        assert 0 < int(k.sum()) < n
        assert torch.equal(x[b, :n][k], pre["cat_mel_text"][b, :n, :M].cpu()[k])
    # no parts: every frame is kept, so the noise cannot reach the output -- and the PCM is the vocoder of the device's own mel
    e0 = make_edits(spec, [(256 * 30 + 41, [], 19)], seed=6)
    _x1, pcm1, len1 = eng.edit_batch(*dev_args(e0), e0["noise"].to(DEV))
    _x2, pcm2, _len2 = eng.edit_batch(*dev_args(e0), torch.randn(e0["noise"].shape, generator=torch.Generator().manual_seed(99)).to(DEV))
    torch.cuda.synchronize()
    assert torch.equal(pcm1, pcm2) and int(len1[0]) == 256 * 30 + 41
    pre0, _x, _p, _w = run_stages(eng, e0, 7)
    n = e0["N"]
    want = orc.to_pcm(orc.vocoder(pre0["cat_mel_text"][0, :n, :M].cpu()))
    assert int((pcm1[0, : n * HOP].cpu().int() - want.int()).abs().max()) <= 2


def _batch_vs_alone(eng, e, spec):
    _x, pcm, pcm_len = eng.edit_batch(*dev_args(e), e["noise"].to(DEV))
    torch.cuda.synchronize()
    for b, L in enumerate(e["L"]):
        n = L // HOP + 1
        one = dict(e, rows=[[0] + r[1:] for r in e["rows"] if r[0] == b], L=[L], keep=e["keep"][b: b + 1, :n].copy(),
                   ids_pad=e["ids"][b][None].contiguous(), text_len=e["text_len"][b: b + 1], noise=e["noise"][b: b + 1, :n].contiguous(), N=n)
        _x1, pcm1, len1 = eng.edit_batch(*dev_args(one), one["noise"].to(DEV))
        torch.cuda.synchronize()
        assert int(len1[0]) == int(pcm_len[b]) == L
        assert torch.equal(pcm1[0, :L], pcm[b, :L]), b
    return pcm


def test_edit_batch_equals_each_edit_alone(hip_tiny, tiny_setup):
    spec, _, _ = tiny_setup
    items = TWO + [(256 * 50 + 200, [(256 * 5, 256 * 12, 9), (256 * 40, 256 * 50, 2)], 44)]
    _batch_vs_alone(hip_tiny["f32"], make_edits(spec, items, seed=7), spec)
    from vietvoice_tts_amd.model_spec import ModelSpec, make_synthetic_weights
    from vietvoice_tts_amd.runtime import HipSynth
    small = ModelSpec.small()
    eng = HipSynth(small, make_synthetic_weights(small, seed=77), acoustic_dtype="bf16", nfe_step=6)
    e = make_edits(small, items, seed=8)
    pcms = []
    for lanes in (1, 2):
        eng.set_option("lanes", lanes)
        pcms.append(_batch_vs_alone(eng, e, small))
    assert torch.equal(pcms[0], pcms[1])
    eng.close()


def _engine(tmp, **kw):
    from vietvoice_tts_amd.core import ModelConfig, TTSEngine
    cfg = ModelConfig(model_cache_dir=str(tmp), synthetic_model=True, model_spec="tiny", nfe_step=5, acoustic_dtype="fp32",
                      max_chunk_duration=8.0, **kw)
    return TTSEngine(cfg)


def test_engine_edit_speech(tmp_path):
    from vietvoice_tts_amd.core import AudioProcessor
    from vietvoice_tts_amd.pack import MAX_POS
    from vietvoice_tts_amd.speech_edit import plan_edit
    e = _engine(tmp_path)
    sr = e.config.sample_rate
    clip, _secs = e.synthesize("Xin chào các bạn, hôm nay trời đẹp quá.")
    dur = clip.size / sr
    parts, fix, text = [(0.3 * dur, 0.5 * dur)], [0.3 * dur], "Xin chào các anh, hôm nay trời đẹp quá."
    out, secs = e.edit_speech(clip, text, parts, fix_duration=fix, seed=11, output_path=str(tmp_path / "edit.wav"))
    again, _ = e.edit_speech(clip, text, parts, fix_duration=fix, seed=11)
    plan = plan_edit(clip.size, parts, fix, sr, e.config.hop_length, e.model_session_manager.spec.n_fft, MAX_POS)
    assert out.dtype == np.int16 and out.ndim == 1 and out.size == plan.spliced_len and secs > 0
    assert np.array_equal(out, again)
    # the same inputs straight through HipSynth.edit_batch
    m = e.model_session_manager
    entry = e.voice_bank.get(AudioProcessor.to_wav_bytes(clip, sr))
    assert entry.n_samples == clip.size
    ids = e.text_processor.text_to_indices([list(e.text_processor.clean_text(text))])
    noise = torch.randn((plan.n_frames, m.spec.n_mel), generator=torch.Generator().manual_seed(11))
    _x, pcm, _len = m.engine.edit_batch(entry.pcm_dev, plan.rows(), [plan.spliced_len], torch.from_numpy(ids).to(DEV),
                                        torch.tensor([ids.shape[1]], dtype=torch.int32, device=DEV),
                                        torch.from_numpy(plan.keep[None]).to(DEV), noise[None].to(DEV))
    assert np.array_equal(pcm[0, : plan.spliced_len].cpu().numpy(), out)
    frames, width, rate = AudioProcessor.decode(str(tmp_path / "edit.wav"))
    assert rate == sr and width == 2 and np.array_equal(frames.reshape(-1), out)
    with pytest.raises(ValueError, match="overlap"):
        e.edit_speech(clip, text, [(0.1 * dur, 0.4 * dur), (0.3 * dur, 0.6 * dur)])
    with pytest.raises(ValueError, match="empty"):
        e.edit_speech(clip, "   ", parts)
    with pytest.raises(ValueError, match="max_chunk_duration"):
        e.edit_speech(clip, text, [(0.1 * dur, 0.1 * dur)], fix_duration=[8.5])
    e.cleanup()


@pytest.mark.parametrize("n_rows", [257, 600])
def test_splice_with_two_and_three_passes_of_descriptor_rows(hip_tiny, n_rows):
    """More rows than the 256 the splice kernel stages in LDS per pass: the rows of tools/edit_host_check.py (one starts at output sample 0,
    one ends at ld_out - 1, one reads src[n_src - 1], the items' rows shuffled over the passes), against numpy."""
    from tests.host_check_util import tool
    eng = hip_tiny["f32"]
    for B, ld_out in ((1, 1000), (3, 1000), (3, 4)):
        src, rows, want = tool("edit").splice_case(n_rows, B, ld_out, seed=n_rows + B)
        out = eng.edit_splice(torch.from_numpy(src).to(DEV), rows, B, ld_out).cpu().numpy()
        assert np.array_equal(out, want), (n_rows, B, ld_out)


def test_restore_past_the_grid(hip_tiny, tiny_setup):
    """B = 8, N = 4096, n_mel = 100: 819200 float4s against a grid of 2048 x 256 threads, so the kernel's loop takes a second trip."""
    spec, _, _ = tiny_setup
    eng = hip_tiny["f32"]
    B, N, M, cd = 8, 4096, spec.n_mel, spec.cond_dim
    assert M == 100 and B * N * (M // 4) > 2048 * 256
    g = torch.Generator().manual_seed(12)
    x = torch.randn((B, N, M), generator=g)
    cat = torch.randn((B, N, cd), generator=g)
    keep = (torch.rand((B, N + 3), generator=g) < 0.5).to(torch.uint8)
    keep[:, 0], keep[:, N - 1] = 1, 1
    seq_len = torch.tensor([0, N, N - 1, 1, N, 2049, N, 4095], dtype=torch.int32)
    got = eng.edit_restore(x.to(DEV), {"cat_mel_text": cat.to(DEV), "seq_len": seq_len.to(DEV)}, keep.to(DEV)).cpu()
    m = (torch.arange(N)[None, :] < seq_len[:, None]) & (keep[:, :N] != 0)
    want = torch.where(m[..., None], cat[..., :M], x)
    assert torch.equal(got, want)
