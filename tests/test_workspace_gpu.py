"""-m gpu: the stage drivers' workspace plans and profiling accounts.

1. vv_transformer_ws_bytes, vv_decode_ws_bytes and the launches / flops / bytes that vv_prof_collect reports for a fixed call
   sequence equal the figures recorded from the build before the drivers were restructured (tests/golden/driver_golden.json, written by
   tests/golden/make_driver_golden.py from ``driver_records`` below): a caller that sized a block with the earlier library still
   fits, and the rooflines of ``bench.py --full`` keep their inputs.
2. A caller-owned block of EXACTLY the bytes asked for is enough and nothing is written outside it: 4 KiB guard bands of 0xA5 on both
   sides stay intact and the result equals the context arena's bit for bit.  The transformer stage runs under rk4 (the slope
   buffers are the last ones taken, and written) and under Euler with "rope_rows" 1 (then the row-gathered rope tables are the last
   ones written); with the default options the tail of the block is never touched and an overrun would go unseen.

Engines of this module's own: it changes plans and options (the shared hip_tiny engines are never re-planned)."""
import ctypes as C
import json
import os

import pytest
import torch

from tests.test_e2e_gpu import make_batch

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "driver_golden.json")
HOP = 256
LENS = {"one": ([80], 80), "ragged": ([77, 30, 51], 80), "short": ([5, 1], 8)}      # per-item lengths and the padded N
# reference clips and generated frames whose seq_len = audio // hop + 1 + gen are the lengths above
BATCH = {"one": ([HOP * 39], [33], [40]), "ragged": ([HOP * 36, HOP * 20, HOP * 30], [41, 11, 30], [40, 9, 20])}
GUARD = 4096


def make_engines():
    from vietvoice_tts_amd.model_spec import ModelSpec, make_synthetic_weights
    from vietvoice_tts_amd.runtime import HipSynth
    tiny, voc = ModelSpec.tiny(), ModelSpec.tiny_vocos()
    w, wv = make_synthetic_weights(tiny, 9527), make_synthetic_weights(voc, 9527)
    return {"f32": HipSynth(tiny, w, device=DEV, acoustic_dtype="fp32", nfe_step=8),
            "bf16": HipSynth(tiny, w, device=DEV, acoustic_dtype="bf16", nfe_step=8),
            "vocos": HipSynth(voc, wv, device=DEV, acoustic_dtype="fp32", nfe_step=8)}


@pytest.fixture(scope="module")
def own():
    engs = make_engines()
    yield engs
    for e in engs.values():
        e.close()


def _steps_need(eng, lens, N):
    nb = C.c_uint64()
    eng._check(eng.lib.vv_transformer_ws_bytes(eng.ctx, len(lens), N, (C.c_int32 * len(lens))(*lens), C.byref(nb)))
    return int(nb.value)


def _decode_need(eng, B, t_gen_max):
    nb = C.c_uint64()
    eng._check(eng.lib.vv_decode_ws_bytes(eng.ctx, B, t_gen_max, C.byref(nb)))
    return int(nb.value)


def _inputs(eng, which):
    """Device inputs of one of the BATCH cases, preprocessed at N = 80 with the lengths on the host too."""
    la, lt, gf = BATCH[which]
    lens, N = LENS[which]
    b = make_batch(eng.spec, la, lt, gf, seed=17)
    assert [int(v) for v in b["seq_len"]] == lens
    d = {k: (v.to(DEV) if torch.is_tensor(v) else v) for k, v in b.items()}
    pre = eng.preprocess(d["audio"], d["audio_len"], d["ids"], d["text_len"], d["seq_len"], N, seq_len_host=lens)
    noise = torch.randn(len(lens), N, eng.spec.n_mel, generator=torch.Generator().manual_seed(23)).to(DEV)
    return pre, noise, lens, N, max(gf)


def driver_records(engs):
    """Everything the golden file pins, through entry points the library has had since the ODE plans: byte counts per option and
    plan, and the profiling accounts (no times) of preprocess + 2 Euler steps + decode on the ragged batch."""
    ws, dec, prof = {}, {}, {}
    try:
        for dt in ("f32", "bf16"):
            eng = engs[dt]
            for plan in ("euler", "rk4"):
                eng.set_nfe(8, plan)
                for lanes in (1, 2):
                    eng.set_option("lanes", lanes)
                    for skt in ((0, 2) if dt == "bf16" else (0,)):
                        eng.set_option("split_k_tail", skt)
                        for name, (lens, N) in LENS.items():
                            ws[f"{dt} {plan} lanes={lanes} split_k_tail={skt} {name}"] = _steps_need(eng, lens, N)
        for which in ("f32", "vocos"):
            for B in (1, 3):
                for t in (1, 40):
                    dec[f"{'vocos' if which == 'vocos' else 'hifigan'} B={B} t_gen_max={t}"] = _decode_need(engs[which], B, t)
    finally:
        for dt in ("f32", "bf16"):
            engs[dt].set_option("lanes", 0)
            engs[dt].set_option("split_k_tail", 0)
            engs[dt].set_nfe(8, "euler")
    for which in ("f32", "bf16", "vocos"):
        eng = engs[which]
        eng.set_nfe(8, "euler")
        la, lt, gf = BATCH["ragged"]
        b = make_batch(eng.spec, la, lt, gf, seed=17)
        d = {k: (v.to(DEV) if torch.is_tensor(v) else v) for k, v in b.items()}
        lens = [int(v) for v in b["seq_len"]]
        eng.prof_enable(True)
        try:
            eng.prof_collect()
            pre = eng.preprocess(d["audio"], d["audio_len"], d["ids"], d["text_len"], d["seq_len"], d["N"], seq_len_host=lens)
            x = d["noise"].clone()
            eng.transformer_steps(x, pre, 0, 2)
            eng.decode(x, pre, b["t_gen_max"])
            got = eng.prof_collect()
        finally:
            eng.prof_enable(False)
        prof[which] = {cls: {k: v[k] for k in ("launches", "flops", "bytes")} for cls, v in got.items()}
    return {"transformer_ws_bytes": ws, "decode_ws_bytes": dec, "prof": prof}


# ------------------------------------------------------------------------------------------------ 1. the recorded figures
def test_byte_counts_and_profiling_accounts_equal_the_recorded_ones(own):
    with open(GOLDEN) as f:
        want = json.load(f)
    got = driver_records(own)
    for kind in ("transformer_ws_bytes", "decode_ws_bytes"):
        assert got[kind].keys() == want[kind].keys()
        for k, v in want[kind].items():
            print(f"{kind} {k}: {got[kind][k]} (recorded {v})")
        assert got[kind] == want[kind], kind
    assert got["prof"].keys() == want["prof"].keys()
    for which, classes in want["prof"].items():
        assert got["prof"][which].keys() == classes.keys()
        for cls, w in classes.items():
            g = got["prof"][which][cls]
            print(f"prof {which} {cls}: {g} (recorded {w})")
            assert g["launches"] == w["launches"], (which, cls)
            for k in ("flops", "bytes"):          # the same expressions over the same launches: equal up to the last bit of a sum
                assert abs(g[k] - w[k]) <= 1e-12 * max(abs(g[k]), abs(w[k])), (which, cls, k)


# ------------------------------------------------------------------------------------------------ 2. exact-size caller blocks
def _guarded(need):
    buf = torch.full((GUARD + need + GUARD,), 0xA5, dtype=torch.uint8, device=DEV)
    assert (buf.data_ptr() + GUARD) % 256 == 0
    return buf, buf[GUARD: GUARD + need]


def _guards_intact(buf, need):
    return bool((buf[:GUARD] == 0xA5).all()) and bool((buf[GUARD + need:] == 0xA5).all())


@pytest.mark.parametrize("setting", ["rk4", "euler_rope_rows"])
@pytest.mark.parametrize("which,lanes", [("ragged", 2), ("one", 2), ("ragged", 1)])
@pytest.mark.parametrize("dt", ["f32", "bf16"])
def test_steps_fit_an_exact_block_and_stay_inside_it(own, dt, which, lanes, setting):
    eng = own[dt]
    try:
        eng.set_nfe(8, "rk4" if setting == "rk4" else "euler")
        eng.set_option("rope_rows", 0 if setting == "rk4" else 1)
        eng.set_option("lanes", lanes)
        pre, noise, lens, N, _ = _inputs(eng, which)
        host = (C.c_int32 * len(lens))(*lens)
        need = _steps_need(eng, lens, N)
        buf, ws = _guarded(need)
        x_arena, x_block = noise.clone(), noise.clone()
        eng.transformer_steps_ex(x_arena, pre, 0, 2, host, None)
        eng.transformer_steps_ex(x_block, pre, 0, 2, host, None, ws=ws)
        torch.cuda.synchronize()
        assert not torch.equal(x_block, noise) and bool(torch.isfinite(x_block).all())
        assert torch.equal(x_block, x_arena)
        assert _guards_intact(buf, need)
        assert bool((ws != 0xA5).any())                     # the block was the workspace of the call
        with pytest.raises(RuntimeError, match="workspace block too small"):
            eng.transformer_steps_ex(noise.clone(), pre, 0, 2, host, None, ws=buf[GUARD: GUARD + need - 256])
    finally:
        eng.set_option("lanes", 0)
        eng.set_option("rope_rows", 0)
        eng.set_nfe(8, "euler")


@pytest.mark.parametrize("which", ["f32", "bf16", "vocos"])
def test_decode_fits_an_exact_block_and_stays_inside_it(own, which):
    """HiFi-GAN behind the fp32 and the bf16 context (f32-MFMA and 3-way-split conv kernels) and the tiny Vocos decoder, B = 3."""
    eng = own[which]
    g = torch.Generator().manual_seed(29)
    ref, gen = [5, 0, 17], [40, 2, 23]
    B, N, T = 3, 60, max(gen)
    x = torch.randn(B, N, eng.spec.n_mel, generator=g).to(DEV)
    i32 = lambda v: torch.tensor(v, dtype=torch.int32, device=DEV)
    pre = {"ref_signal_len": i32(ref), "seq_len": i32([r + t for r, t in zip(ref, gen)])}
    pcm, n = eng.decode(x, pre, T)
    need = _decode_need(eng, B, T)
    buf, ws = _guarded(need)
    pcm2, n2 = torch.zeros_like(pcm), torch.zeros_like(n)
    st = torch.cuda.current_stream().cuda_stream
    eng._check(eng.lib.vv_decode_into(eng.ctx, B, N, x.data_ptr(), pre["ref_signal_len"].data_ptr(), pre["seq_len"].data_ptr(), T,
                                      pcm2.data_ptr(), pcm2.shape[1], n2.data_ptr(), None, ws.data_ptr(), need, st))
    torch.cuda.synchronize()
    assert bool(pcm.any()) and torch.equal(pcm2, pcm) and torch.equal(n2, n)
    assert _guards_intact(buf, need)
    assert bool((ws != 0xA5).any())
    assert eng.lib.vv_decode_into(eng.ctx, B, N, x.data_ptr(), pre["ref_signal_len"].data_ptr(), pre["seq_len"].data_ptr(), T,
                                  pcm2.data_ptr(), pcm2.shape[1], n2.data_ptr(), None, ws.data_ptr(), need - 256, st) == -22
    assert "workspace block too small" in eng.lib.vv_last_error(eng.ctx).decode()
