"""-m gpu: N6, the Vocos decoder on gfx950 against the float64 torch reference of test_vocos_cpu.py.  Tolerances are those of
test_e2e_gpu.py: waveform 2e-4 abs (full scale 1.0), PCM within +-2 LSB.  PARITY UNPINNED against the real decode graph."""
import ctypes as C
from dataclasses import replace

import numpy as np
import pytest
import torch

from tests.test_vocos_cpu import istft_reference, reference_pcm, vocos_reference
from vietvoice_tts_amd.model_spec import ModelSpec, make_synthetic_weights

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
WAVE_TOL, PCM_TOL = 2e-4, 2


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _check(eng, rc):
    assert rc == 0, eng.lib.vv_last_error(eng.ctx).decode()


def _full_decoder_spec():
    """The full-size Vocos decoder (512 / 1536 / 8, k 7) behind the tiny acoustic model: the decoder is what is under test."""
    f = ModelSpec.full_vocos()
    return replace(ModelSpec.tiny_vocos(), vocos_dim=f.vocos_dim, vocos_intermediate=f.vocos_intermediate, vocos_layers=f.vocos_layers)


_ENGINES = {}


def _engine(spec, dtype="fp32"):
    from vietvoice_tts_amd.runtime import HipSynth
    key = (spec, dtype)
    if key not in _ENGINES:
        w = make_synthetic_weights(spec, 9527)
        _ENGINES[key] = (HipSynth(spec, w, device=DEV, acoustic_dtype=dtype, nfe_step=4), w)
    return _ENGINES[key]


def _state(spec, gen, ref, seed=0):
    """x [B][N][n_mel] N(0, 1), ref_signal_len, seq_len = ref + gen."""
    g = torch.Generator().manual_seed(seed)
    seq = [r + t for r, t in zip(ref, gen)]
    N = max(seq) + 3
    x = torch.randn(len(gen), N, spec.n_mel, generator=g)
    i32 = lambda v: torch.tensor(v, dtype=torch.int32, device=DEV)
    return x, {"ref_signal_len": i32(ref), "seq_len": i32(seq)}, max(gen)


def _decode(eng, x, pre, t_max):
    pcm, n, wave = eng.decode(x.to(DEV).contiguous(), pre, t_max, want_wave=True)
    torch.cuda.synchronize()
    return pcm.cpu(), n.cpu(), wave.cpu()


def test_istft_head_matches_torch_istft():
    spec = ModelSpec.tiny_vocos()
    eng, _w = _engine(spec)
    T = [1, 2, 7, 13, 30]
    B, T_max, ld = len(T), max(T), 1152
    g = torch.Generator().manual_seed(5)
    head = torch.zeros(B, T_max, ld)
    head[:, :, :513] = -2.0 + torch.randn(B, T_max, 513, generator=g)
    loud = torch.rand(B, T_max, 513, generator=g) < 0.01
    head[:, :, :513][loud] = 5.0 + torch.rand(int(loud.sum()), generator=g)         # log-magnitudes above log 100 = 4.6: clipped
    head[:, :, 513:1026] = (torch.rand(B, T_max, 513, generator=g) * 2 - 1) * 50.0    # phases up to +-50 rad
    hd = head.to(DEV)
    frames = torch.tensor(T, dtype=torch.int32, device=DEV)
    L = T_max * spec.hop_length
    pcm = torch.full((B, L), 123, dtype=torch.int16, device=DEV)
    wave = torch.full((B, L), 7.0, device=DEV)
    n = torch.zeros(B, dtype=torch.int32, device=DEV)
    _check(eng, eng.lib.vv_istft_head(eng.ctx, B, T_max, hd.data_ptr(), ld, frames.data_ptr(), pcm.data_ptr(), L, n.data_ptr(),
                                      wave.data_ptr(), _stream()))
    torch.cuda.synchronize()
    pcm, n, wave = pcm.cpu(), n.cpu(), wave.cpu()
    for b, t in enumerate(T):
        want = istft_reference(spec, head[b, :t, :1026])
        k = spec.hop_length * (t - 1)
        assert int(n[b]) == k == want.numel()
        if k:
            assert float((wave[b, :k].double() - want).abs().max()) < WAVE_TOL
            assert int((pcm[b, :k].int() - reference_pcm(want).int()).abs().max()) <= PCM_TOL
        assert not pcm[b, k:].any() and not wave[b, k:].any()                      # the rest of the row is zeros


def test_embed_im2col_gemm_matches_conv1d():
    from vietvoice_tts_amd import pack
    import torch.nn.functional as F
    spec = ModelSpec.tiny_vocos()
    eng, w = _engine(spec)
    gen, ref = [9, 1, 17], [4, 0, 11]
    x, pre, T_max = _state(spec, gen, ref, seed=3)
    B, KE = len(gen), pack.vocos_embed_k(spec)
    cols = torch.full((B * T_max, KE), float("nan"), device=DEV)
    _check(eng, eng.lib.vv_vocos_im2col(eng.ctx, x.to(DEV).data_ptr(), B, x.shape[1], pre["ref_signal_len"].data_ptr(), pre["seq_len"].data_ptr(),
                                        T_max, cols.data_ptr(), KE, _stream()))
    We = dict((n, fn(w)) for n, _d, _s, fn in pack.entries(spec, torch.float32) if n == "voc.embed.weight")["voc.embed.weight"].to(DEV)
    from tests import gpu_util as gu
    h = gu.gemm(eng, cols, We, bias=w["voc.embed.bias"].to(DEV), tile=128).cpu().reshape(B, T_max, -1)
    for b in range(B):
        m = x[b, ref[b]: ref[b] + gen[b]].double()
        want = F.conv1d(m.T[None], w["voc.embed.weight"].double(), w["voc.embed.bias"].double(), padding=3)[0].T
        assert float((h[b, : gen[b]].double() - want).abs().max()) < 1e-4 * float(want.abs().max())
        ln = lambda t: F.layer_norm(t, (spec.vocos_dim,), w["voc.norm.weight"].double(), w["voc.norm.bias"].double(), 1e-6)
        assert float((ln(h[b, : gen[b]].double()) - ln(want)).abs().max()) < 1e-3


@pytest.mark.parametrize("which", ["tiny", "small", "full"])
def test_decode_matches_the_float64_reference(which):
    spec = {"tiny": ModelSpec.tiny_vocos(), "small": ModelSpec.small_vocos(), "full": _full_decoder_spec()}[which]
    eng, w = _engine(spec)
    gen, ref = [40, 2, 23, 1], [5, 0, 17, 3]
    x, pre, T_max = _state(spec, gen, ref, seed=1)
    pcm, n, wave = _decode(eng, x, pre, T_max)
    for b in range(len(gen)):
        want = vocos_reference(spec, w, x[b, ref[b]: ref[b] + gen[b]]) if gen[b] > 1 else torch.zeros(0, dtype=torch.float64)
        k = spec.hop_length * max(gen[b] - 1, 0)
        assert int(n[b]) == k == want.numel()
        if k:
            assert 0.05 < float(want.abs().max()) < 1.0
            assert float((wave[b, :k].double() - want).abs().max()) < WAVE_TOL
            assert int((pcm[b, :k].int() - reference_pcm(want).int()).abs().max()) <= PCM_TOL
        assert not pcm[b, k:].any()


def test_batch_equals_each_item_alone():
    spec = ModelSpec.small_vocos()
    eng, _w = _engine(spec)
    gen, ref = [31, 6, 18], [2, 9, 0]
    x, pre, T_max = _state(spec, gen, ref, seed=2)
    pcm, n, wave = _decode(eng, x, pre, T_max)
    for b in range(3):
        i32 = lambda v: torch.tensor([v], dtype=torch.int32, device=DEV)
        p1, n1, w1 = _decode(eng, x[b: b + 1], {"ref_signal_len": i32(ref[b]), "seq_len": i32(ref[b] + gen[b])}, gen[b])
        k = int(n1[0])
        assert k == int(n[b]) and torch.equal(p1[0, :k], pcm[b, :k]) and torch.equal(w1[0, :k], wave[b, :k])


def test_decode_into_and_captured_graph_equal_eager():
    from vietvoice_tts_amd.runtime import GraphedDecode
    spec = ModelSpec.tiny_vocos()
    eng, _w = _engine(spec)
    gen, ref = [12, 25], [3, 1]
    x, pre, T_max = _state(spec, gen, ref, seed=4)
    pcm, n, _wave = _decode(eng, x, pre, T_max)
    B, N = x.shape[0], x.shape[1]
    nb = C.c_uint64()
    _check(eng, eng.lib.vv_decode_ws_bytes(eng.ctx, B, T_max, C.byref(nb)))
    ws = torch.empty(int(nb.value), dtype=torch.uint8, device=DEV)
    p2 = torch.zeros_like(pcm, device=DEV)
    n2 = torch.zeros(B, dtype=torch.int32, device=DEV)
    xd = x.to(DEV).contiguous()
    _check(eng, eng.lib.vv_decode_into(eng.ctx, B, N, xd.data_ptr(), pre["ref_signal_len"].data_ptr(), pre["seq_len"].data_ptr(), T_max,
                                       p2.data_ptr(), p2.shape[1], n2.data_ptr(), None, ws.data_ptr(), ws.numel(), _stream()))
    torch.cuda.synchronize()
    assert torch.equal(p2.cpu(), pcm) and torch.equal(n2.cpu(), n)
    gd = GraphedDecode(eng, B, N, T_max)
    p3, n3 = gd(xd, pre["ref_signal_len"], pre["seq_len"])
    torch.cuda.synchronize()
    assert torch.equal(p3.cpu(), pcm) and torch.equal(n3.cpu(), n)


def test_bf16_and_fp32_contexts_decode_the_same_bits():
    spec = ModelSpec.tiny_vocos()
    gen, ref = [20, 7], [0, 4]
    x, pre, T_max = _state(spec, gen, ref, seed=6)
    a = _decode(_engine(spec, "fp32")[0], x, pre, T_max)
    b = _decode(_engine(spec, "bf16")[0], x, pre, T_max)
    for u, v in zip(a, b):
        assert torch.equal(u, v)


def test_set_vocos_refused_after_finalize_and_for_bad_cfg():
    from vietvoice_tts_amd.runtime import vocos_cfg_from_spec
    spec = ModelSpec.tiny_vocos()
    eng, _w = _engine(spec)
    assert eng.lib.vv_set_vocos(eng.ctx, C.byref(vocos_cfg_from_spec(spec))) == -22
    from vietvoice_tts_amd.runtime import cfg_from_spec
    ctx = C.c_void_p()
    assert eng.lib.vv_create(C.byref(ctx), 0, C.byref(cfg_from_spec(spec)), 0) == 0
    try:
        for dim, inter in ((130, 384), (128, 200), (1152, 384)):
            v = vocos_cfg_from_spec(spec)
            v.dim, v.intermediate = dim, inter
            assert eng.lib.vv_set_vocos(ctx, C.byref(v)) == -22
        v = vocos_cfg_from_spec(spec)
        v.win_length = 800
        assert eng.lib.vv_set_vocos(ctx, C.byref(v)) == -22
        assert eng.lib.vv_set_vocos(ctx, C.byref(vocos_cfg_from_spec(spec))) == 0
    finally:
        eng.lib.vv_destroy(ctx)


TEXT = "Xin chào các bạn, hôm nay trời đẹp quá. Chúng ta cùng nhau đi dạo quanh hồ nhé, rồi về nhà uống trà."


def _tts(tmp):
    from vietvoice_tts_amd.core import ModelConfig, TTSEngine
    cfg = ModelConfig(model_cache_dir=str(tmp), synthetic_model=True, model_spec="tiny-vocos", nfe_step=5, acoustic_dtype="fp32",
                      max_chunk_duration=8.0)
    return TTSEngine(cfg)


def test_engine_synthesize_matches_oracle_acoustics_plus_reference_vocos(tmp_path):
    from oracle.vv_oracle import Oracle
    e = _tts(tmp_path)
    m, cfg = e.model_session_manager, e.config
    assert m.spec.vocoder == "vocos"
    ref, txt = m.select_sample()
    inputs = e._prepare_inputs(ref, txt, TEXT)
    got, _ = e.synthesize(TEXT)
    w = make_synthetic_weights(m.spec, cfg.random_seed)
    orc = Oracle(m.spec, w, nfe_step=cfg.nfe_step)
    gen = torch.Generator().manual_seed(cfg.random_seed)
    waves = []
    for audio, ids, dur, _ts in inputs:
        n = int(dur[0])
        noise = torch.randn((n, m.spec.n_mel), generator=gen, dtype=torch.float32)
        pre = orc.preprocess(torch.from_numpy(np.asarray(audio).reshape(-1).astype(np.int16)), torch.from_numpy(np.asarray(ids)[0].astype(np.int32)),
                             n, noise)
        x = pre["noise"]
        for st in range(cfg.nfe_step - 1):
            x = orc.transformer_step(x, pre, st)
        r = int(pre["ref_signal_len"])
        waves.append(reference_pcm(vocos_reference(m.spec, w, x[r:n])).numpy().reshape(1, 1, -1))
    want = e.audio_processor.concatenate_with_crossfade_improved(waves, cfg.cross_fade_duration, cfg.sample_rate)
    assert got.shape == want.shape and got.size > 0
    assert int(np.abs(got.astype(np.int32) - want.astype(np.int32)).max()) <= PCM_TOL
    e.cleanup()
    e2 = _tts(tmp_path)
    whole, _ = e2.synthesize(TEXT)
    e2.cleanup()
    e3 = _tts(tmp_path)
    streamed = np.concatenate(list(e3.synthesize_stream(TEXT, chunks_per_step=1)))
    e3.cleanup()
    assert streamed.shape == whole.shape
    assert int(np.abs(streamed.astype(np.int32) - whole.astype(np.int32)).max()) <= PCM_TOL


def test_engine_edit_speech_returns_the_vocos_length(tmp_path):
    from vietvoice_tts_amd.model_pack import synthetic_voice
    from vietvoice_tts_amd.pack import MAX_POS
    from vietvoice_tts_amd.speech_edit import plan_edit
    e = _tts(tmp_path)
    spec, cfg = e.model_session_manager.spec, e.config
    clip = synthetic_voice(77, 2.3)
    parts = [(0.6, 1.1)]
    plan = plan_edit(clip.size, parts, [0.8], cfg.sample_rate, cfg.hop_length, spec.n_fft, MAX_POS)
    wave, _ = e.edit_speech(clip, "xin chào các bạn, đây là một câu đã sửa.", parts, fix_duration=[0.8], seed=3)
    e.cleanup()
    want = min(plan.spliced_len, cfg.hop_length * (plan.n_frames - 1))
    assert want <= plan.spliced_len and wave.dtype == np.int16 and wave.size == want and np.abs(wave.astype(np.int32)).max() > 0
