"""-m gpu: the kernels between the GEMMs -- ln_mod_kernel (all four <To, Td> forms), groupnorm_kernel, mel_kernel, text_embed_kernel,
dwconv_kernel, grn_stats_kernel / grn_apply_kernel and build_cat_kernel -- against float64 references of the operands as given, element
by element, at the smallest shapes where each form can go wrong.

References, A_e, yardsticks and bounds: tests/gpu_util.py (ln_ref, gn_ref, mel_ref, dw_ref, grn_ref, te_ref), each bound
max(c 2^-24, 4 x yardstick) with c counted from the kernel's roundings; tests/test_norm_ref_cpu.py checks those claims without a device.
Metric: err = max_e (|got_e - ref_e| - allow_e) / A_e; a bf16 output is allowed its store rounding 2^-8 |ref_e|, Mish 12 x 2^-24 |z_e|,
the mel logf's own 3 x 2^-24 |log|.  text_embed and build_cat are compared bit for bit.

Every launch goes through a gpu_util helper: outputs sit between guard rows / bands and (with a leading dimension) padding columns of
7.0, inputs have NaN in their padding columns, behind their last row and behind every vector and table, a delta's own split-K tail rows
hold NaN, input rows a length masks hold NaN; the guards are checked after the launch; each case runs contiguous and padded, and twice,
and all outputs must be the same bits.  One NORM_PARITY line per case; profiles/norm_parity/notes.md records them."""
import ctypes as C

import pytest
import torch

pytestmark = pytest.mark.gpu

from tests import gpu_util as gu  # noqa: E402
from vietvoice_tts_amd import runtime as rt  # noqa: E402

LN, GN, DW, GRN, TE = gu.ln_cases(), gu.gn_cases(), gu.dw_cases(), gu.grn_cases(), gu.te_cases()


def _ids(cases):
    return [c.name for c in cases]


def _same_bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(a.contiguous().view(torch.uint8), b.contiguous().view(torch.uint8))


def _four(launch):
    """contiguous, padded, and each once more -> the contiguous output; all four must be the same bits."""
    outs = [launch(padded=p) for p in (False, True, False, True)]
    first = outs[0] if isinstance(outs[0], tuple) else (outs[0],)
    for k, o in enumerate(outs[1:]):
        o = o if isinstance(o, tuple) else (o,)
        for a, b in zip(first, o):
            assert _same_bits(a, b), ("the padded launch differs from the contiguous one", "the repeat differs from the first launch", "the padded repeat differs")[k]
    return outs[0]


def _parity(case, got, r, old_ref, ref=None, A=None, allow="r", bound=None, yard=None, tag=""):
    ref, A = (r.ref if ref is None else ref), (r.A if A is None else A)
    err, where = gu.parity_err(got, ref, A, r.allow if allow == "r" else allow)
    print("\n" + gu.norm_line(case, err, r, gu.old_metric(got, old_ref), where, bound, yard) + tag)
    b = r.bound if bound is None else bound
    assert err <= b, f"{case.name}{tag}: err {err:.3e} > bound {b:.3e} at {where}: got {float(got[where]):.9g}, ref {float(ref[where]):.9g}"


# ------------------------------------------------------------------------------------ LayerNorm
@pytest.mark.parametrize("case", LN, ids=_ids(LN))
def test_layernorm_float64_parity(hip_tiny, case):
    """y per element inside the derived bound; the residual stream written back is EXACT -- (x + d1) + d2 in fp32, a split-K tail's parts
    summed in part order and rounded once to the delta's dtype -- or untouched (keep_x, no delta)."""
    eng = hip_tiny["f32"]
    o = case.ops()
    r = case.refs(o)
    y, x_after = _four(lambda padded: gu.ln_launch(eng, case, o, padded=padded))
    want_x = r.xs if (case.n_delta and not case.keep_x) else o.x
    assert torch.equal(x_after, want_x), f"{case.name}: the stream differs from the exact fp32 sums by up to {float((x_after - want_x).abs().max()):.3e}"
    assert y.dtype == case.out_dtype
    _parity(case, y, r, r.f32)


def _no_tails(a):
    a.delta_tail_parts = a.delta2_tail_parts = a.tail_row0 = 0
    a.delta_tail = a.delta2_tail = None


# name -> (what to break in the arguments of a valid launch, the message of the check that must refuse it)
LN_REFUSALS = {
    "D_mod_4": (lambda a: setattr(a, "D", a.D - 2), "ln: D must be a multiple of 4 within [4, 1024]"),
    "D_above_1024": (lambda a: [setattr(a, k, 1028) for k in ("D", "ldx", "ldy", "ld_delta")], "ln: D must be a multiple of 4 within [4, 1024]"),
    "D_zero": (lambda a: setattr(a, "D", 0), "ln: D must be a multiple of 4 within [4, 1024]"),
    "D_negative": (lambda a: setattr(a, "D", -4), "ln: D must be a multiple of 4 within [4, 1024]"),
    "ld_delta_short": (lambda a: setattr(a, "ld_delta", a.D - 4), "ln: bad delta leading dimension"),
    "ld_delta_mod_4": (lambda a: setattr(a, "ld_delta", a.ld_delta + 2), "ln: bad delta leading dimension"),
    "ldx_short": (lambda a: setattr(a, "ldx", a.D - 4), "ln: ldx and ldy must be at least D"),
    "ldy_short": (lambda a: setattr(a, "ldy", a.D - 4), "ln: ldx and ldy must be at least D"),
    "ldx_mod_4": (lambda a: setattr(a, "ldx", a.ldx + 2), "ln: D must be a multiple of 4 within [4, 1024]"),
    # no tails left: only the check of delta2 itself can refuse this one
    "delta2_without_delta": (lambda a: [_no_tails(a), setattr(a, "delta", None)], "ln: delta2 without delta"),
    "tail_without_delta": (lambda a: [setattr(a, "delta", None), setattr(a, "delta2", None)], "ln: a delta tail without its delta"),
    "tail_without_buffer": (lambda a: [setattr(a, "delta_tail", None), setattr(a, "delta2_tail_parts", 0), setattr(a, "delta2_tail", None)], "ln: bad split-K tail"),
    "tail2_without_buffer": (lambda a: [setattr(a, "delta2_tail_parts", 3), setattr(a, "delta2_tail", None)], "ln: bad split-K tail"),
    "tail_row0_at_R": (lambda a: setattr(a, "tail_row0", a.R), "ln: bad split-K tail"),
    "tail_nine_parts": (lambda a: setattr(a, "delta_tail_parts", 9), "ln: bad split-K tail"),
    "tail_misaligned": (lambda a: setattr(a, "delta_tail", a.delta_tail + 4), "ln: split-K tail buffers must be 16-byte aligned"),
    "R_zero": (lambda a: setattr(a, "R", 0), "ln: empty"),
}


@pytest.mark.parametrize("what", sorted(LN_REFUSALS))
@pytest.mark.parametrize("padded", [False, True])
def test_layernorm_refusals_write_nothing(hip_tiny, what, padded):
    """include/vvtts.h (vv_ln_args): each violated precondition returns -22 before anything is launched, with the message of its own
    check; y keeps its fill and x its values.  The base launch is valid (the first assertion)."""
    eng = hip_tiny["f32"]
    case = gu.LnCase("ln/refusal/" + what, n_delta=2, tail_row0=2, tail_parts=(2, 2), delta_bf16=True, seed=900)
    o = case.ops()
    if what == "D_mod_4":
        gu.ln_launch(eng, case, o, padded=padded, mutate=_no_tails)        # delta + delta2 without tails is a valid launch
    mutate, message = LN_REFUSALS[what]
    gu.ln_launch(eng, case, o, padded=padded, expect_error=True, mutate=mutate)
    assert eng.lib.vv_last_error(eng.ctx).decode().startswith(message), eng.lib.vv_last_error(eng.ctx).decode()


# ------------------------------------------------------------------------------------ GroupNorm
@pytest.mark.parametrize("case", GN, ids=_ids(GN))
def test_groupnorm_float64_parity(hip_tiny, case):
    """Every slab shape, both access paths, the affine present or not, Mish, a large mean, and an outlier as a slab's FIRST element (what
    the one-pass variance shifted by that element lost five digits on) with the same outlier as its last element as the control."""
    eng = hip_tiny["f32"]
    o = case.ops()
    r = case.refs(o)
    y = _four(lambda padded: gu.gn_launch(eng, case, o, padded=padded))
    _parity(case, y, r, r.f32)


# ------------------------------------------------------------------------------------ mel
def test_mel_float64_parity(hip_tiny, tiny_setup):
    """All mel cases in one test (they share the tables): the shortest clip the reflection is defined for, lengths at and beside a
    multiple of the hop, one item much shorter than the other (its frames behind it exact zeros), 32767 behind every audio_len; noise,
    silence (every bin the same float, logf(1e-5f)), a full-scale square wave with -32768, impulses at the first and last sample."""
    spec, _, orc = tiny_setup
    eng = hip_tiny["f32"]
    # the device's logf is not correctly rounded (gpu_util.MEL_LOG_ALLOW: 3 x 2^-24 of the result): "logf(1e-5f)" is one of the few floats
    # that close to the true logarithm, and which one is the device library's choice.  Every silent bin must hold the SAME one.
    true_log = float(torch.log(torch.tensor(1e-5, dtype=torch.float32).double()))
    misses = []
    for case in gu.mel_cases(spec):
        o = case.ops()
        r = gu.mel_ref(case, spec, orc, o)
        got = _four(lambda padded: gu.mel_launch(eng, case, o, spec, padded=padded))
        for b, L in enumerate(case.lens):
            assert bool((got[b, L // spec.hop_length + 1:] == 0.0).all()), f"{case.name}: frames behind item {b} are not exact zeros"
        if case.signal == "zero":
            silent = got[0, :case.lens[0] // spec.hop_length + 1]
            print(f"\nNORM_MEL_FLOOR silent bins hold {float(silent[0, 0]):.9g}; log(1e-5f) is {true_log:.12g}: "
                  f"{abs(float(silent[0, 0]) - true_log) / 2.0 ** -20:.2f} ulp apart")
            assert bool((silent.view(torch.int32) == silent[0, 0].view(torch.int32)).all()), f"{case.name}: the silent bins differ among themselves"
            assert abs(float(silent[0, 0]) - true_log) <= gu.MEL_LOG_ALLOW * abs(true_log), f"{case.name}: a silent bin is not logf(1e-5f)"
        try:
            _parity(case, got, r, r.f32)
        except AssertionError as e:
            misses.append(str(e))
    assert not misses, misses


def test_mel_short_clips_float64_parity(hip_tiny, tiny_setup):
    """Clips the fp32 oracle cannot frame: no samples (one frame of the row's first sample), one sample, n_fft / 2 and n_fft / 2 + 1,
    against the count alone (gpu_util.mel_ref_counted); tools/mel_host_check.py runs the same lengths at a small transform."""
    spec = tiny_setup[0]
    eng = hip_tiny["f32"]
    for case in gu.mel_short_cases(spec):
        o = case.ops()
        r = gu.mel_ref_counted(case, spec, o)
        got = _four(lambda padded: gu.mel_launch(eng, case, o, spec, padded=padded))
        for b, L in enumerate(case.lens):
            assert bool((got[b, L // spec.hop_length + 1:] == 0.0).all()), f"{case.name}: frames behind item {b} are not exact zeros"
        _parity(case, got, r, r.f32)


def _mel_guarded(eng, audio, audio_len, F_max, guard_rows=3):
    """vv_mel on audio [B][ld] that sits inside a larger allocation, guard rows of 32767 in front and behind -> (rc, mel [B][F_max][n_mel])."""
    B, ld = audio.shape
    whole = torch.full((guard_rows + B + guard_rows, ld), 32767, dtype=torch.int16)
    whole[guard_rows:guard_rows + B] = audio
    whole = whole.to(gu.DEV)
    lens = torch.tensor(audio_len, dtype=torch.int32, device=gu.DEV)
    mbuf, mel = gu._guarded((B, F_max, eng.spec.n_mel), gu.CONV_GUARD, gu.CONV_FILL)
    mel.fill_(gu.CONV_FILL)
    rc = eng.lib.vv_mel(eng.ctx, whole[guard_rows].data_ptr(), ld, lens.data_ptr(), mel.data_ptr(), B, F_max, gu.stream())
    torch.cuda.synchronize()
    gu._bands_intact(mbuf, gu.CONV_GUARD, gu.CONV_FILL, "mel")
    return rc, mel.cpu()


@pytest.mark.parametrize("which", [0, 1], ids=["first_item", "last_item"])
def test_mel_device_length_beyond_the_row_is_clamped(hip_tiny, tiny_setup, which):
    """A device audio_len of ld_audio + 5 (a stale tensor): the kernel clamps it to the row, so the result is that of the clip clamped to
    ld_audio and the frames past it are zeros -- wrong audio for that call, never a read outside the row.  The rows sit between guard rows
    of 32767 inside one allocation: nothing outside the test's own memory is read whatever the kernel does."""
    spec, _, orc = tiny_setup
    eng = hip_tiny["f32"]
    h = spec.hop_length
    lens = (6 * h + 1, 4 * h) if which == 0 else (4 * h, 6 * h + 1)
    case = gu.MelCase(f"mel/over_long_{which}", lens, seed=40 + which)
    o = case.ops()
    r = gu.mel_ref(case, spec, orc, o)                                 # the longer clip fills its row: clamped to ld_audio it is the row
    ld = max(lens)
    F_ref = ld // h + 1
    given = [n + 5 if n == ld else n for n in lens]
    rc, got = _mel_guarded(eng, o.audio, given, F_ref + 2)
    gu.check(eng, rc)
    assert bool((got[:, F_ref:] == 0.0).all()), "frames past the clamped clip are not exact zeros"
    for b, L in enumerate(lens):
        assert bool((got[b, L // h + 1:] == 0.0).all()), f"frames behind item {b} are not exact zeros"
    _parity(case, got[:, :F_ref].contiguous(), r, r.f32)
    rc, same = _mel_guarded(eng, o.audio, list(lens), F_ref + 2)       # the honest length: the same bits
    gu.check(eng, rc)
    assert _same_bits(got, same)


MEL_REFUSALS = {
    "audio_null": (dict(audio=None), "mel: audio, audio_len, mel and the four tables are required"),
    "audio_len_null": (dict(audio_len=None), "mel: audio, audio_len, mel and the four tables are required"),
    "mel_null": (dict(mel=None), "mel: audio, audio_len, mel and the four tables are required"),
    "ld_audio_zero": (dict(ld=0), "mel: ld_audio, hop and n_mel must be at least 1"),
    "ld_audio_negative": (dict(ld=-8), "mel: ld_audio, hop and n_mel must be at least 1"),
    "B_zero": (dict(B=0), "mel: empty"),
    "F_max_zero": (dict(F_max=0), "mel: empty"),
    "B_beyond_grid_y": (dict(B=65536), "mel: at most 65535 clips per launch"),
}


@pytest.mark.parametrize("what", sorted(MEL_REFUSALS))
def test_mel_refusals_write_nothing(hip_tiny, what):
    """vvk_mel refuses null buffers, ld_audio < 1 and a batch beyond grid.y with -22 and its own message before anything is launched (hop,
    n_mel and n_fft come from the bound model and are checked by the same lines); the base launch is valid."""
    eng = hip_tiny["f32"]
    spec = eng.spec
    B, ld = 2, spec.n_fft
    F_max = ld // spec.hop_length + 1
    audio = torch.full((B, ld), 1000, dtype=torch.int16, device=gu.DEV)
    lens = torch.tensor([ld, ld // 2 + 1], dtype=torch.int32, device=gu.DEV)
    mel = torch.full((B, F_max, spec.n_mel), gu.CONV_FILL, device=gu.DEV)
    call = lambda **k: eng.lib.vv_mel(eng.ctx, k.get("audio", audio.data_ptr()), k.get("ld", ld), k.get("audio_len", lens.data_ptr()),
                                      k.get("mel", mel.data_ptr()), k.get("B", B), k.get("F_max", F_max), gu.stream())
    bad, message = MEL_REFUSALS[what]
    _refused(eng, call(**bad), mel)
    assert eng.lib.vv_last_error(eng.ctx).decode().startswith(message), eng.lib.vv_last_error(eng.ctx).decode()
    gu.check(eng, call())
    torch.cuda.synchronize()
    assert not bool((mel == gu.CONV_FILL).any())


# ------------------------------------------------------------------------------------ the text stack
@pytest.mark.parametrize("case", TE, ids=_ids(TE))
def test_text_embed_bit_exact(hip_tiny, case):
    eng = hip_tiny["f32"]
    o = case.ops()
    got = _four(lambda padded: gu.te_launch(eng, case, o, padded=padded))
    want = gu.te_ref(case, o)
    assert _same_bits(got, want), (case.name, (got != want).nonzero()[:4].tolist())
    print(f"\nNORM_PARITY case={case.name} kernel={case.kernel} bit_exact=1 elements={got.numel()}")


@pytest.mark.parametrize("case", DW, ids=_ids(DW))
def test_dwconv_float64_parity(hip_tiny, case):
    """Every output row, the rows at and beyond len included (the kernel writes them from the taps that still reach valid input)."""
    eng = hip_tiny["f32"]
    o = case.ops()
    r = case.refs(o)
    got = _four(lambda padded: gu.dw_launch(eng, case, o, padded=padded))
    _parity(case, got, r, r.f32)


@pytest.mark.parametrize("case", GRN, ids=_ids(GRN))
def test_grn_float64_parity(hip_tiny, case):
    """In place, fp32 and bf16; the statistics over the valid tokens, the apply over all N rows; sumsq against float64 too."""
    eng = hip_tiny["f32"]
    o = case.ops()
    r = case.refs(o)
    y, ss = _four(lambda padded: gu.grn_launch(eng, case, o, padded=padded))
    assert y.dtype == case.dtype
    _parity(case, ss, r, r.ss32, ref=r.ss, A=r.ss_A, allow=None, bound=r.ss_bound, yard=r.ss_yard, tag=" (sumsq)")
    _parity(case, y, r, r.f32)
    for s, L in enumerate(o.lens):
        if L == 0:
            assert bool((ss[s] == 0.0).all())


def _refused(eng, rc, *outs):
    assert rc == -22, (rc, eng.lib.vv_last_error(eng.ctx).decode())
    torch.cuda.synchronize()
    for t in outs:
        assert bool((t == gu.CONV_FILL).all()), "a refused launch wrote its output"


def test_text_entries_refuse_bad_arguments(hip_tiny):
    """include/vvtts.h: alignment, % 4 and C % 64 preconditions of vv_text_embed / vv_dwconv / vv_grn are refused with -22, nothing written."""
    eng, L, st = hip_tiny["f32"], hip_tiny["f32"].lib, gu.stream()
    f = lambda *shape: torch.full(shape, gu.CONV_FILL, device=gu.DEV)
    B, N, Dt, V = 2, 5, 8, 5
    ids, tl = torch.zeros(B, 4, dtype=torch.int32, device=gu.DEV), torch.ones(B, dtype=torch.int32, device=gu.DEV)
    emb, pos, out = f(V + 1, Dt), f(N + 1, Dt), f(2 * B, N, Dt)
    te = lambda **k: L.vv_text_embed(eng.ctx, k.get("ids", ids.data_ptr()), 4, tl.data_ptr(), k.get("emb", emb.data_ptr()), k.get("pos", pos.data_ptr()),
                                     k.get("V", V), k.get("out", out.data_ptr()), k.get("B", B), k.get("N", N), k.get("Dt", Dt), st)
    for bad in (dict(Dt=6), dict(Dt=0), dict(emb=emb.data_ptr() + 4), dict(pos=pos.data_ptr() + 8), dict(out=out.data_ptr() + 4), dict(V=0), dict(B=0),
                dict(N=0), dict(ids=None), dict(ids=ids.data_ptr() + 2)):
        _refused(eng, te(**bad), out)
    Cc, KW = 8, 3
    x, y, w, bias = f(2 * B, N, Cc), f(2 * B, N, Cc), f(Cc + 1, KW), f(Cc + 4)
    sl = torch.full((B,), N, dtype=torch.int32, device=gu.DEV)
    dw = lambda **k: L.vv_dwconv(eng.ctx, k.get("x", x.data_ptr()), k.get("y", y.data_ptr()), w.data_ptr(), k.get("bias", bias.data_ptr()),
                                 k.get("sl", sl.data_ptr()), k.get("B", B), 2 * B, N, k.get("C", Cc), k.get("KW", KW), st)
    for bad in (dict(C=6), dict(C=0), dict(KW=0), dict(KW=4), dict(x=x.data_ptr() + 4), dict(y=y.data_ptr() + 8), dict(bias=bias.data_ptr() + 4), dict(B=0),
                dict(y=x.data_ptr()), dict(x=None)):
        _refused(eng, dw(**bad), y, x)
    Cg = 64
    gx, ss, ga, be = f(2 * B, N, Cg), f(2 * B, Cg), f(Cg), f(Cg + 4)
    grn = lambda **k: L.vv_grn(eng.ctx, k.get("dt", rt.VV_F32), k.get("x", gx.data_ptr()), k.get("ss", ss.data_ptr()), ga.data_ptr(),
                               k.get("be", be.data_ptr()), k.get("sl", sl.data_ptr()), k.get("B", B), 2 * B, N, k.get("C", Cg), st)
    for bad in (dict(C=32), dict(C=96), dict(C=8256), dict(dt=2), dict(x=gx.data_ptr() + 4), dict(dt=rt.VV_BF16, x=gx.data_ptr() + 2), dict(be=be.data_ptr() + 4),
                dict(B=0), dict(ss=None)):
        _refused(eng, grn(**bad), gx, ss)


# ------------------------------------------------------------------------------------ build_cat, through vv_preprocess
def test_build_cat_is_a_bit_exact_gather(hip_tiny, tiny_setup):
    """cat_mel_text = [mel (t < ref_len) | text(b)], the drop tensor = [0 | text(B + b)]: the mel columns are vv_mel's output bit for bit
    and exact zeros behind ref_len, the drop tensor's are exact zeros, and both text halves are the bits the unit entries produce when
    the test chains the text stack itself (vv_text_embed, then per block vv_dwconv, vv_layernorm, vv_gemm + GELU, vv_grn, vv_gemm into
    the residual) on the fp32 engine."""
    from vietvoice_tts_amd.pack import text_pos_table
    spec, w, _ = tiny_setup
    eng = hip_tiny["f32"]
    dev, st = gu.DEV, gu.stream()
    B, N, T = 2, 24, 10
    hop, M, Dt = spec.hop_length, spec.n_mel, spec.text_dim
    g = torch.Generator().manual_seed(4711)
    lens = [6 * hop + 10, spec.n_fft // 2 + 1]
    S = max(lens) + 5
    audio = (torch.randn(B, S, generator=g) * 5000).clamp(-30000, 30000).to(torch.int16).to(dev)
    audio_len = torch.tensor(lens, dtype=torch.int32, device=dev)
    ids = torch.randint(0, spec.vocab_size, (B, T), generator=g).to(torch.int32).to(dev)
    text_len = torch.tensor([T, 4], dtype=torch.int32, device=dev)
    seq_len = torch.tensor([N, 20], dtype=torch.int32, device=dev)
    pre = eng.preprocess(audio, audio_len, ids, text_len, seq_len, N)
    torch.cuda.synchronize()
    cat, drop, ref_len = pre["cat_mel_text"].cpu(), pre["cat_mel_text_drop"].cpu(), pre["ref_signal_len"].cpu().tolist()
    assert ref_len == [L // hop + 1 for L in lens] and cat.shape == (B, N, M + Dt)
    # the mel columns
    F_max = S // hop + 1
    mel = torch.zeros(B, F_max, M, device=dev)
    gu.check(eng, eng.lib.vv_mel(eng.ctx, audio.data_ptr(), S, audio_len.data_ptr(), mel.data_ptr(), B, F_max, st))
    torch.cuda.synchronize()
    mel = mel.cpu()
    for b in range(B):
        assert _same_bits(cat[b, :ref_len[b], :M].contiguous(), mel[b, :ref_len[b]].contiguous()), f"item {b}: the mel columns are not vv_mel's bits"
        assert bool((cat[b, ref_len[b]:, :M] == 0.0).all()), f"item {b}: the mel columns behind ref_len are not exact zeros"
    assert bool((drop[:, :, :M] == 0.0).all()), "the drop tensor's mel columns are not exact zeros"
    # the text halves, chained through the unit entries
    d = lambda name: w[name].float().contiguous().to(dev)
    R2, C2, k = 2 * B * N, Dt * spec.text_ff_mult, spec.text_conv_k
    emb, pos = d("text.embed.weight"), text_pos_table(spec)[:N].contiguous().to(dev)
    tx, ty, th = (torch.zeros(R2, Dt, device=dev) for _ in range(3))
    sumsq = torch.zeros(2 * B, C2, device=dev)
    gu.check(eng, eng.lib.vv_text_embed(eng.ctx, ids.data_ptr(), T, text_len.data_ptr(), emb.data_ptr(), pos.data_ptr(), spec.vocab_size + 1,
                                        tx.data_ptr(), B, N, Dt, st))
    for i in range(spec.text_layers):
        p = f"text.blocks.{i}"
        cw, cb = d(p + ".dwconv.weight").reshape(Dt, k).contiguous(), d(p + ".dwconv.bias")
        gu.check(eng, eng.lib.vv_dwconv(eng.ctx, tx.data_ptr(), ty.data_ptr(), cw.data_ptr(), cb.data_ptr(), seq_len.data_ptr(), B, 2 * B, N, Dt, k, st))
        nw, nb = d(p + ".norm.weight"), d(p + ".norm.bias")
        a = rt.vv_ln_args()
        a.out_dtype, a.x, a.ldx, a.y, a.ldy, a.R, a.D = rt.VV_F32, ty.data_ptr(), Dt, th.data_ptr(), Dt, R2, Dt
        a.w, a.b, a.add_one, a.eps = nw.data_ptr(), nb.data_ptr(), 0, 1e-6
        gu.check(eng, eng.lib.vv_layernorm(eng.ctx, C.byref(a), st))
        tm = gu.gemm(eng, th, d(p + ".pwconv1.weight"), bias=d(p + ".pwconv1.bias"), mode=gu.MODE_STORE, act=gu.ACT_GELU_ERF)
        gg, gb = d(p + ".grn.gamma"), d(p + ".grn.beta")
        gu.check(eng, eng.lib.vv_grn(eng.ctx, rt.VV_F32, tm.data_ptr(), sumsq.data_ptr(), gg.data_ptr(), gb.data_ptr(), seq_len.data_ptr(), B, 2 * B, N, C2, st))
        gu.gemm(eng, tm, d(p + ".pwconv2.weight"), bias=d(p + ".pwconv2.bias"), mode=gu.MODE_GATE_RES, C_io=tx)
    torch.cuda.synchronize()
    text = tx.cpu().view(2 * B, N, Dt)
    for b in range(B):
        assert _same_bits(cat[b, :, M:].contiguous(), text[b].contiguous()), f"item {b}: the text columns are not the chained text stack's bits"
        assert _same_bits(drop[b, :, M:].contiguous(), text[B + b].contiguous()), f"item {b}: the drop tensor's text columns are not the chained stack's bits"
