"""CPU checks of the conv parity harness (tests/gpu_util.py): the float64 references against the library's float64 convolutions, the
polyphase packing against the plain transposed conv, the error scale and the yardstick, and the claims the case list makes about the
x3 instantiation and the window walk each case reaches."""
import pytest
import torch
import torch.nn.functional as F

from tests import gpu_util as gu

CASES = gu.conv_cases()
POS = gu.posconv_cases()
SAMPLE = CASES[::5] + [c for c in CASES if c.kind == "tconv" and c.T <= 70]
X3_FORMS = ("x3", "x3w", "stream", "generic")


def x3_dispatch(KW, transposed, up, cin, rows_total, rows_pad, resid, accumulate, wg_rows):
    """launch_x3 / up2_stream_fits of vv_vocoder_x3.hip restated -> (instantiation, rows per workgroup)."""
    if (transposed and up == 2 and KW == 2 and not resid and not accumulate and cin in (64, 128) and rows_total % 64 == 0
            and 64 <= rows_total <= 128 and wg_rows != -1):
        return (gu.STREAM4 if cin == 64 else gu.STREAM8), 64
    if rows_total <= 32:
        return (gu.T_NARROW if transposed else gu.NARROW), 32
    wide = wg_rows == 128 and rows_pad % 128 == 0
    if not wide and (KW <= 7 or transposed):
        return (gu.T_R64 if transposed else gu.R64), 64
    if rows_total <= 64 or not wide:
        assert KW == 11 and not transposed          # the only way here with rows_pad = rows_total rounded up to 64
        return gu.K11, 64
    return (gu.T_WIDE if transposed else gu.WIDE), 128


def _reached(case, form, variant):
    c2 = variant == "conv2"
    return x3_dispatch(case.KW, bool(case.up), case.up, case.cin, case.rows_total, case.rows_pad, c2, c2, {"x3": 0, "x3w": 128, "stream": 0, "generic": -1}[form])


def test_every_claimed_instantiation_is_the_one_the_dispatch_rule_gives():
    reached, fallback = set(), False
    for c in CASES:
        assert c.kind == "mrf" or set(c.reach) == set(c.forms) - {"f32"}, c.name
        for v in c.variants:
            for f in c.forms_of(v):
                if f in X3_FORMS:
                    inst, vr = _reached(c, f, v)
                    assert inst == c.reach[f], (c.name, f, v, inst, c.reach[f])
                    reached.add(inst)
                    fallback |= f == "x3w" and c.rows_pad == 192 and vr == 64 and c.fallback
    assert set(gu.X3_REQUIRED) <= reached, set(gu.X3_REQUIRED) - reached
    assert fallback, "no case has rows_pad = 192 with wg_rows = 128"
    # the f32 kernel's two row widths, conv and transposed, and every mrf_pair_kernel instantiation (three kernels x two widths)
    assert {(bool(c.up), c.rows_total <= 32) for c in CASES if "f32" in c.forms} == {(False, False), (False, True), (True, False), (True, True)}
    assert {(c.KW, c.cin) for c in CASES if c.kind == "mrf"} == {(k, w) for k in (3, 7, 11) for w in (32, 64)}


def test_window_and_row_tile_counts_are_the_claimed_ones():
    seen = {"x3": set(), "x3w": set()}
    for c in CASES:
        for f, (n_win, n_rt) in c.claims.items():
            _, vr = _reached(c, f, "plain")
            assert gu._x3_walk(c.B, c.T + 1 if c.up else c.T, c.rows_total, vr) == (n_win, n_rt), (c.name, f)
            seen[f].add((n_win, n_rt))
    for f in seen:
        assert {w for w, _ in seen[f]} >= {1, 7, 8, 9, 12, 17}
        for w in (1, 7, 8, 9, 12, 17):
            assert {r for ww, r in seen[f] if ww == w} >= {1, 2, 4}, (f, w)


def test_case_list_covers_the_sections():
    conv = {(c.KW, c.dil) for c in CASES if c.kind == "conv" and c.section == "taps"}
    mrf = {(c.KW, c.dil, c.cin) for c in CASES if c.kind == "mrf" and c.section == "taps"}
    assert conv == {(k, d) for k in (3, 7, 11) for d in (1, 2, 3, 4, 5)}
    assert mrf == {(k, d, w) for k, d in conv for w in (32, 64)}
    assert {c.T for c in CASES if c.section == "seams" and c.kind == "conv"} == {1, 2, 3, 255, 256, 257, 513}
    assert {(c.up, c.T) for c in CASES if c.section == "seams" and c.kind == "tconv"} == {(u, t) for u in (2, 8) for t in (1, 255, 256, 257)}
    for k, vt2 in gu.MRF_VT2.items():
        assert vt2 == 128 - ((k - 1 + 3) & ~3)
        assert {c.T for c in CASES if c.section == "seams" and c.kind == "mrf" and c.KW == k} == {1, vt2 - 1, vt2, vt2 + 1, 2 * vt2 + 1}
    for c in CASES:
        if c.section == "lengths":
            seam = gu.MRF_VT2[c.KW] if c.kind == "mrf" else 256
            assert c.lens == [-3, 0, 1, seam - 1, seam, seam + 1, c.T] and c.variants == ("plain", "conv2") and c.T % 4 == 0, c.name
    assert {c.kind for c in CASES if c.section == "lengths"} == {"conv", "tconv", "mrf"}
    assert {c.up for c in CASES if c.section == "lengths" and c.kind == "tconv"} == {2, 8}
    assert {c.cin for c in CASES if c.section == "channels"} == {1, 7, 8, 9, 15, 16, 17, 100, 512}
    assert {c.cout for c in CASES if c.section == "rows" and c.kind == "conv"} == {24, 32, 33, 64, 65, 128, 192, 256}
    assert {(c.cin, c.cout, c.up) for c in CASES if c.section == "rows" and c.kind == "tconv"} == {(32, 16, 8), (64, 32, 8), (16, 8, 2), (64, 32, 2), (128, 64, 2)}
    assert all(c.in_offset == 1 and c.T % 4 == 0 or c.T % 4 for c in CASES if c.section == "alignment")
    assert {c.cin for c in CASES if c.section == "neighbours" and c.kind == "conv"} >= {20, 100}
    assert {c.seq_n for c in POS} >= {1, 15, 16, 17, 63, 64, 65, 255, 256, 257, 513}
    assert {c.groups for c in POS} >= {1, 2, 16} and next(c for c in POS if c.groups == 16).seq_n == 257
    assert all(c.n_seq == 2 * len(c.lens) for c in POS if c.lens) and any(c.resid for c in POS) and not all(c.resid for c in POS)


@pytest.mark.parametrize("case", SAMPLE, ids=[c.name for c in SAMPLE])
def test_float64_reference_agrees_with_the_library_in_float64(case):
    o = case.ops()
    for v in case.variants:
        ref, A, yard = case.refs(v)
        kw = case.ref_kw(v)
        z = lambda t: F.leaky_relu(gu._zero_outside(t.double(), case.lens), float(torch.tensor(0.1, dtype=torch.float32)))   # the kernel's fp32 slope
        if case.kind == "mrf":
            t1 = F.conv1d(z(o.x), o.w.double(), o.bias.double(), dilation=case.dil, padding=case.dil * (case.KW - 1) // 2)
            lib = F.conv1d(z(t1), o.w2.double(), o.bias2.double(), padding=(case.KW - 1) // 2) + o.x.double()
        elif case.up:
            lib = F.conv_transpose1d(z(o.x), o.w.double(), o.bias.double(), stride=case.up, padding=case.up // 2)
        else:
            lib = F.conv1d(z(o.x), o.w.double(), o.bias.double(), dilation=case.dil, padding=case.dil * (case.KW - 1) // 2)
        if case.kind != "mrf" and kw["resid"] is not None:
            lib = lib + kw["resid"].double()
        lib = lib * torch.tensor(kw["scale"], dtype=torch.float32).double()
        if kw["prev"] is not None:
            lib = lib + kw["prev"].double()
        assert lib.shape == ref.shape
        assert float(((lib - ref).abs() / A).max()) < 1e-13
        assert float(A.min()) > 0.0 and bool((A >= ref.abs() * (1 - 1e-12)).all())
        # the yardstick is a real figure (or the floor applies), and it never lets the bound near the old whole-tensor tolerance
        bound = gu.conv_bound(yard)
        assert yard > 0.0 or bound == 8 * gu.EPS24
        assert bound <= 64 * gu.EPS24, (case.name, v, yard)


@pytest.mark.parametrize("cin,cout,up,T", [(16, 8, 2, 9), (20, 16, 8, 5), (8, 4, 2, 1)])
def test_polyphase_packing_is_the_plain_transposed_conv(cin, cout, up, T):
    """out[co][q up + p - up / 2] = sum_ci sum_j in[ci][q - j] W[ci][j][co up + p], q in [0, T], on the packed slab."""
    g = torch.Generator().manual_seed(cin + up)
    x, w = torch.randn(2, cin, T, generator=g).double(), torch.randn(cin, cout, 2 * up, generator=g).double()
    wp = gu.conv_transpose_pack(w, up).double()
    assert wp.shape == ((cin + 7) // 8 * 8, 2, (cout * up + 63) // 64 * 64) and not bool(wp[cin:].any()) and not bool(wp[:, :, cout * up:].any())
    xp = F.pad(x, (1, 1))                                   # xp[..., q + 1] = in[q], zero at q = -1 and q = T
    out = torch.zeros(2, cout, T * up, dtype=torch.float64)
    for q in range(T + 1):
        for row in range(cout * up):
            co, p = divmod(row, up)
            t = q * up + p - up // 2
            if 0 <= t < T * up:
                out[:, co, t] = sum(torch.einsum("bc,c->b", xp[:, :, q + 1 - j], wp[:cin, j, row]) for j in range(2))
    assert torch.allclose(out, F.conv_transpose1d(x, w, None, stride=up, padding=up // 2), rtol=0, atol=1e-12)
    assert torch.allclose(gu._conv_transpose_taps(x, w, up), out, rtol=0, atol=1e-12)


POS_SMALL = [c for c in POS if c.seq_n <= 65]


@pytest.mark.parametrize("case", POS_SMALL, ids=[c.name for c in POS_SMALL])
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_posconv_reference_agrees_with_the_library_in_float64(case, dtype):
    o = case.ops(dtype)
    for layout in ("padded", "packed"):
        refs, As, yard = case.refs(dtype, layout)
        x, resid, starts = o.x, o.resid, None
        if layout == "packed":
            x, resid, starts, total = case.packed(dtype)
            assert total == starts[-1] + max(0, min(case.lens[(case.n_seq - 1) % len(case.lens)], case.seq_n)) + 2
        rows = gu.posconv_rows(case.n_seq, case.seq_n, case.lens, starts)
        assert len(rows) == case.n_seq == len(refs)
        for (r0, n, L), (r0r, ref), (_, A) in zip(rows, refs, As):
            assert r0 == r0r and ref.shape[0] == n
            if n == 0:
                continue
            xs = x[r0:r0 + n].double().clone()
            xs[L:] = 0
            lib = F.mish(F.conv1d(xs.t().unsqueeze(0), o.w.double(), o.bias.double(), padding=15, groups=case.groups)).squeeze(0).t()
            if resid is not None:
                lib = lib + resid[r0:r0 + n].double()
            assert float(((lib - ref).abs() / A).max()) < 1e-13
            assert float(A.min()) > 0.0
        assert 0.0 < yard and gu.conv_bound(yard) <= 64 * gu.EPS24
