"""-m gpu: the implicit-GEMM convolution kernels (conv_mfma_kernel, conv_x3_kernel, up2_stream_x3_kernel, mrf_pair_kernel, posconv_bf16 /
posconv_f32) against float64 references of the operands as given, element by element, at the seams of their launch geometry.

Reference (tests/gpu_util.py conv_ref / mrf_ref / posconv_ref), for every output column:
    out = (conv(lrelu(x zero-filled outside [0, len))) + bias [+ resid as given]) * scale [+ previous out]
fully determined, so the WHOLE output is compared.  Metric: err = max_e |got_e - ref_e| / A_e, A_e = the same expression with every operand
replaced by its absolute value.  Bound: max(8 x 2^-24, 4 x yardstick), yardstick = the CPU library in fp32 on the same operands in the same
metric; the x3 forms add 2^-23 (their dropped piece products); a bf16 output adds its store rounding, 2^-8 |ref_e| (gpu_util.BF16_STORE).  Every case also keeps
the old whole-tensor tolerance.  One CONV_PARITY line per (case, form, variant); profiles/conv_parity/notes.md records them.

Every launch goes through a wrapper that puts a guard band in front of and behind `out` and eight channels of NaN behind the weight slab and
checks the band afterwards; every address a test relies on lies inside a tensor it allocated.  The cases and the x3 instantiation each one
claims to reach are listed in gpu_util.conv_cases(); tests/test_conv_ref_cpu.py checks the claims against the dispatch rule."""
import pytest
import torch

pytestmark = pytest.mark.gpu

from tests import gpu_util as gu  # noqa: E402

CASES = gu.conv_cases()
POS = gu.posconv_cases()
F32, BF16 = torch.float32, torch.bfloat16
DT_NAME = {F32: "f32", BF16: "bf16"}


def _ids(cases):
    return [c.name for c in cases]


def _bits_equal(a, b):
    return a.shape == b.shape and torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


def _with_x(o, x, **more):
    s = gu._Ops()
    s.__dict__.update(o.__dict__)
    s.x = x
    s.__dict__.update(more)
    return s


def _launch(eng, case, form, variant, o=None, lens="case", in_offset=None, in_tail=0):
    """One launch of a case in one form and variant -> the output [B][cout][T_out] on the CPU (guard bands checked by the wrapper)."""
    o = case.ops() if o is None else o
    lens = case.lens if lens == "case" else lens
    c2 = variant == "conv2"
    kw = dict(lens=lens, guard=gu.CONV_GUARD, in_offset=case.in_offset if in_offset is None else in_offset, in_tail=in_tail,
              scale=1.0 / 3.0 if c2 else 1.0, accumulate=1 if c2 else 0, out0=o.prev if c2 else None)
    if case.kind == "mrf":
        return gu.mrf_resblock(eng, o.x, o.wp, o.bias, o.wp2, o.bias2, case.KW, case.dil, **kw).cpu()
    T_in = o.x.shape[2]
    return gu.conv1d(eng, o.x, o.wp, o.bias, case.cout, T_in * case.up if case.up else T_in, case.KW, case.dil, case.up,
                     resid=o.resid if c2 else None, pre_slope=0.1, x3=gu.CONV_FORMS[form], **kw).cpu()


def _two_launches(eng, case, variant, o=None, lens="case"):
    """The unfused twin of vv_mrf_resblock: vv_conv1d(conv1) then vv_conv1d(conv2, resid = y), both on the f32 MFMA kernel."""
    o = case.ops() if o is None else o
    lens = case.lens if lens == "case" else lens
    c2 = variant == "conv2"
    C_, T = case.cout, o.x.shape[2]
    t1 = gu.conv1d(eng, o.x, o.wp, o.bias, C_, T, case.KW, case.dil, 0, pre_slope=0.1, lens=lens, guard=gu.CONV_GUARD, in_offset=case.in_offset)
    return gu.conv1d(eng, t1.cpu(), o.wp2, o.bias2, C_, T, case.KW, 1, 0, resid=o.x, pre_slope=0.1, scale=1.0 / 3.0 if c2 else 1.0,
                     accumulate=1 if c2 else 0, out0=o.prev if c2 else None, lens=lens, guard=gu.CONV_GUARD).cpu()


@pytest.mark.parametrize("case", CASES, ids=_ids(CASES))
def test_conv_float64_parity(hip_tiny, case):
    """Every case of the grid, every form it lists, plain and (where listed) in the decode's conv2 form: per element against float64 inside
    the derived bound, inside the old whole-tensor tolerance, guard bands intact; the fused mrf launch equals its two-launch twin and the
    streaming up-sampler equals the generic kernel, bit for bit."""
    eng = hip_tiny["f32"]
    misses = []
    for variant in case.variants:
        ref, A, yard = case.refs(variant)
        outs = {}
        for form in case.forms_of(variant):
            got = outs[form] = _launch(eng, case, form, variant)
            assert got.shape == ref.shape
            err, where = gu.parity_err(got, ref, A)
            bound = gu.conv_bound(yard, x3=form not in ("f32", "mrf"))
            old = gu.rel_err(got, ref)
            print(f"\nCONV_PARITY case={case.name} section={case.section} form={form} variant={variant} err={err:.3e} yardstick={yard:.3e} "
                  f"bound={bound:.3e} ratio={err / bound:.2f} old_rel_err={old:.2e} worst_item_row_col={where}")
            if not err <= bound:
                misses.append((form, variant, f"err {err:.3e} > bound {bound:.3e} at (item, row, column) {where}"))
            if not old < gu.TOL_F32:
                misses.append((form, variant, f"whole-tensor rel_err {old:.3e} >= {gu.TOL_F32}"))
        if case.kind == "mrf" and not _bits_equal(outs["mrf"], _two_launches(eng, case, variant)):
            misses.append(("mrf", variant, "the fused launch differs from conv1 + conv2 in two launches"))
        if "stream" in outs and "generic" in outs and not _bits_equal(outs["stream"], outs["generic"]):
            misses.append(("stream", variant, "the streaming up-sampler differs from the generic x3 kernel"))
    assert not misses, misses


LEN_CASES = [c for c in CASES if c.lens is not None]


@pytest.mark.parametrize("case", LEN_CASES, ids=_ids(LEN_CASES))
def test_conv_input_past_len_is_never_used(hip_tiny, case):
    """Input columns past an item's valid length hold NaN in one run and 1e30 in another: the whole output is bit-identical to the run that
    holds zeros there (a value that was read and multiplied, even by zero weights, would show)."""
    eng = hip_tiny["f32"]
    o = case.ops()
    past = torch.arange(case.T)[None, :] >= torch.tensor([max(0, min(L, case.T)) for L in case.lens])[:, None]
    fills = {v: _with_x(o, torch.where(past[:, None, :], torch.tensor(v), o.x)) for v in (0.0, gu.NAN, 1.0e30)}
    for variant in case.variants:
        for form in case.forms_of(variant):
            zero = _launch(eng, case, form, variant, o=fills[0.0])
            assert bool(torch.isfinite(zero).all()), (case.name, form, variant)
            for v in (gu.NAN, 1.0e30):
                got = _launch(eng, case, form, variant, o=fills[v])
                if case.kind == "mrf":      # y is also the residual, added AS GIVEN: columns past len carry the poison by definition
                    got = torch.where(past[:, None, :], zero, got)
                assert _bits_equal(got, zero), (case.name, form, variant, f"{v} past len changed the output")


WIN_CASES = [c for c in CASES if c.section == "windows"]


@pytest.mark.parametrize("case", WIN_CASES, ids=_ids(WIN_CASES))
def test_conv_x3_every_window_equals_the_item_alone(hip_tiny, case):
    """The 1-D window walk of conv_x3_kernel (win = (jj / n_rt) * 8 + xcd, b = win / n_tt): every item of the batch is bit-identical to the
    same item launched alone, in both x3 forms -- a window decoded to the wrong item, time tile or row tile cannot pass."""
    eng = hip_tiny["f32"]
    for form in case.forms:
        batch = _launch(eng, case, form, "plain")
        for i in range(case.B):
            alone = _launch(eng, case, form, "plain", o=case.item(i))
            assert _bits_equal(batch[i:i + 1], alone), (case.name, form, f"item {i} differs from the item alone")


NB_CASES = [c for c in CASES if c.section == "neighbours"]


@pytest.mark.parametrize("case", NB_CASES, ids=_ids(NB_CASES))
def test_conv_item_does_not_see_its_neighbours(hip_tiny, case):
    """Item 1 of a batch whose other items hold NaN everywhere is bit-identical to item 1 alone: the pad channels of the last chunk (in
    memory the next item's first channels) are never multiplied in.  Then as the LAST item, its input a view into a larger allocation
    whose head and tail hold NaN."""
    eng = hip_tiny["f32"]
    o = case.ops()
    nan = torch.full_like(o.x[:1], gu.NAN)
    middle = _with_x(o, torch.cat([nan, o.x[1:2], nan], 0))
    last = _with_x(o, torch.cat([nan, o.x[1:2]], 0), resid=o.resid[:2], prev=o.prev[:2])
    for form in case.forms:
        alone = _launch(eng, case, form, "plain", o=case.item(1))
        assert bool(torch.isfinite(alone).all())
        assert _bits_equal(_launch(eng, case, form, "plain", o=middle)[1:2], alone), (case.name, form, "NaN neighbours reached item 1")
        assert _bits_equal(_launch(eng, case, form, "plain", o=last, in_offset=4, in_tail=64)[1:2], alone), (case.name, form, "NaN behind the last item reached it")


def test_mrf_resblock_refuses_wider_stages(hip_tiny):
    eng = hip_tiny["f32"]
    g = torch.Generator().manual_seed(3)
    y, w, b = torch.randn(1, 128, 40, generator=g), gu.pack_conv(torch.randn(128, 128, 3, generator=g)), torch.zeros(128)
    rc, msg = gu.mrf_resblock(eng, y, w, b, w, b, 3, 1, expect_error=True)
    assert rc == -22 and b"mrf_resblock" in msg


# ------------------------------------------------------------------------------------ posconv
PGRID = [(c, dt, odt) for c in POS for dt, odt in ((F32, F32), (BF16, BF16), (BF16, F32))]


def _pos_launch(eng, case, dt, odt, layout, poison=True, **kw):
    """-> (whole out buffer on the CPU, starts, rows).  Padded layout: input rows past a sequence's length hold NaN."""
    o = case.ops(dt)
    if layout == "packed":
        x, resid, starts, rows = case.packed(dt)
    else:
        x, resid, starts, rows = o.x.clone(), o.resid, None, case.n_seq * case.seq_n
        if poison:
            for r0, n, L in gu.posconv_rows(case.n_seq, case.seq_n, case.lens):
                x[r0 + L:r0 + n] = gu.NAN
    pads = dict(pad_in=case.pad, pad_out=case.pad, pad_resid=case.pad)
    pads.update(kw)
    out = gu.posconv(eng, x, o.w, o.bias, n_seq=case.n_seq, seq_n=case.seq_n, groups=case.groups, resid=resid, lens=case.lens, starts=starts,
                     out_dtype=odt, sentinel_rows=4, **pads)
    return out.cpu(), starts, rows


def _pos_check(case, dt, odt, layout, out, starts, rows, tag, misses):
    refs, As, yard = case.refs(dt, layout)
    D, fill = case.D, gu.CONV_FILL
    assert bool((out[:, D:].float() == fill).all()), (tag, "padding columns of out were written")
    assert bool((out[rows:].float() == fill).all()), (tag, "sentinel rows were written")
    owned = torch.zeros(out.shape[0], dtype=torch.bool)
    worst, where, old_worst, dev9, model9 = 0.0, None, 0.0, 0.0, 0.0
    for s, ((r0, ref), (_, A)) in enumerate(zip(refs, As)):
        n = ref.shape[0]
        owned[r0:r0 + n] = True
        if n == 0:
            continue
        got = out[r0:r0 + n, :D]
        err, w = gu.parity_err(got, ref, A, allow=gu.BF16_STORE * ref.abs() if odt == BF16 else None)
        if err >= worst:
            worst, where = err, (s,) + w
        if odt == BF16:         # under a 2^-9 |ref_e| store term: the device, and float64 rounded to bf16 (nothing but the store)
            dev9 = max(dev9, gu.parity_err(got, ref, A, allow=gu.BF16_STORE_HALF * ref.abs())[0])
            model9 = max(model9, gu.parity_err(gu.bf16r(ref), ref, A, allow=gu.BF16_STORE_HALF * ref.abs())[0])
        old_worst = max(old_worst, gu.rel_err(got, ref))
    bad = ((out.float() != fill).any(dim=1) & ~owned)[:rows].nonzero().flatten().tolist()
    assert not bad, (tag, "rows owned by no sequence were written", bad[:8])
    bound = gu.conv_bound(yard)
    print(f"\nCONV_PARITY case=posconv_{case.name} section=posconv form={DT_NAME[dt]}->{DT_NAME[odt]} variant={layout} err={worst:.3e} "
          f"yardstick={yard:.3e} bound={bound:.3e} ratio={worst / bound:.2f} old_rel_err={old_worst:.2e} worst_seq_row_col={where}"
          + (f" err_with_2^-9_store={dev9:.3e} store_only_model_with_2^-9_store={model9:.3e}" if odt == BF16 else ""))
    if not worst <= bound:
        misses.append((tag, f"err {worst:.3e} > bound {bound:.3e} at (sequence, row, column) {where}"))
    if not old_worst < (5e-3 if dt == BF16 else gu.TOL_F32):
        misses.append((tag, f"whole-sequence rel_err {old_worst:.3e}"))


@pytest.mark.parametrize("case,dt,odt", PGRID, ids=[f"{c.name}-{DT_NAME[dt]}-{DT_NAME[odt]}" for c, dt, odt in PGRID])
def test_posconv_float64_parity(hip_tiny, case, dt, odt):
    """Both kernels, padded and packed layouts, n_seq = 2 B with lengths indexed seq % B, padded leading dimensions: every row the kernel
    writes (padded: every row < seq_n; packed: rows [0, len)) against float64 on the operands as given; padding columns, sentinel rows
    and packed rows nobody owns keep their fill; a packed sequence is bit-identical to the same sequence in the padded layout."""
    eng = hip_tiny["f32"]
    misses, outs = [], {}
    for layout in ("padded", "packed") if case.lens else ("padded",):     # packed rows need a length array
        out, starts, rows = _pos_launch(eng, case, dt, odt, layout)
        outs[layout] = (out, starts)
        _pos_check(case, dt, odt, layout, out, starts, rows, (case.name, DT_NAME[dt], DT_NAME[odt], layout), misses)
    assert not misses, misses
    if "packed" not in outs:
        return
    (pad_out, _), (pk_out, starts) = outs["padded"], outs["packed"]
    for s, (r0, _, L) in enumerate(gu.posconv_rows(case.n_seq, case.seq_n, case.lens)):
        a, b = pad_out[r0:r0 + L, :case.D].float(), pk_out[starts[s]:starts[s] + L, :case.D].float()
        assert _bits_equal(a, b), (case.name, f"sequence {s}: packed rows differ from the padded layout")


def test_posconv_f32_kernel_takes_any_leading_dimension(hip_tiny):
    """The f32 kernel's epilogue is scalar: ld_out / ld_resid need no multiple (the refusals below are the bf16 kernel's only)."""
    eng = hip_tiny["f32"]
    case = next(c for c in POS if c.name == "seq_n65")
    misses = []
    out, starts, rows = _pos_launch(eng, case, F32, F32, "padded", pad_out=1, pad_resid=3)
    _pos_check(case, F32, F32, "padded", out, starts, rows, ("odd_ld",), misses)
    assert not misses, misses


def test_posconv_refuses_bad_arguments(hip_tiny):
    """vvk_posconv returns -22 with a message, and launches nothing, for: seq_len with B <= 0 (a modulo by zero on the device), a residual
    narrower than the channels, and leading dimensions / pointers that break the 4-channel vector accesses of the bf16 kernel's epilogue."""
    eng = hip_tiny["f32"]
    case = next(c for c in POS if c.name == "seq_n17")

    def refused(dt, odt, tweak, what):
        o = case.ops(dt)
        resid = o.resid if o.resid is not None else torch.zeros_like(o.x)
        rc, msg = gu.posconv(eng, o.x, o.w, o.bias, n_seq=case.n_seq, seq_n=case.seq_n, groups=case.groups, resid=resid, lens=case.lens,
                             out_dtype=odt, pad_in=8, pad_out=8, pad_resid=8, sentinel_rows=4, tweak=tweak, expect_error=True)
        assert rc == -22 and msg.startswith(b"posconv"), (what, rc, msg)

    def setter(**fields):
        def tweak(a):
            for k, v in fields.items():
                setattr(a, k, v)
        return tweak

    def shift(field, nbytes):
        def tweak(a):
            setattr(a, field, getattr(a, field) + nbytes)
        return tweak

    for dt, odt in ((F32, F32), (BF16, BF16), (BF16, F32)):
        refused(dt, odt, setter(B=0), "seq_len with B = 0")
        refused(dt, odt, setter(B=-1), "seq_len with B < 0")
        refused(dt, odt, setter(ld_resid=case.D - 4), "ld_resid < groups * 64")
    for odt in (BF16, F32):
        refused(BF16, odt, setter(ld_out=case.D + 2), "ld_out % 4")
        refused(BF16, odt, setter(ld_resid=case.D + 2), "ld_resid % 4")
        refused(BF16, odt, shift("resid", 4), "resid not 8-byte aligned")
        refused(BF16, odt, shift("bias", 4), "bias not 16-byte aligned")
    refused(BF16, BF16, shift("out", 4), "bf16 out not 8-byte aligned")
    refused(BF16, F32, shift("out", 8), "f32 out not 16-byte aligned")
