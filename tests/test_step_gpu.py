"""-m gpu: the kernels between the transformer's prediction and the PCM -- pack_cat / pack_cat_guided, cfg_euler, ode_stage (all four
instantiations), apg_reduce / apg_coef, row_tables / guided_tables, the length kernels, rope_compact / rope_rows, mel_slice, vocos_im2col,
vocos_spectrum, vocos_ola and conv_post (all four instantiations) -- launched alone through their unit entries and compared with float64
references of the operands as given, element by element, at the smallest shapes that reach each edge.

Cases, references, scales, counts and launch helpers: tests/step_util.py; tests/test_step_ref_cpu.py checks without a device that the
cases reach what they claim and that every bound rejects the mutation table.  Gathers, tables and PCM are compared bit for bit.  Every
launch runs twice on fresh buffers and must return the same bits; outputs sit between bands of 7.0, operands between NaN guard rows.
One STEP_PARITY line per case; profiles/step_parity/notes.md records them."""
import ctypes as C

import pytest
import torch

pytestmark = pytest.mark.gpu

from tests import gpu_util as gu  # noqa: E402
from tests import step_util as su  # noqa: E402
from tests.gpu_util import DEV, EPS24, parity_err  # noqa: E402
from vietvoice_tts_amd import runtime as rt  # noqa: E402

STAGE = su.stage_cases()
SMALL_STAGE = [c for c in STAGE if c.Rc <= 86]


def _ids(cases):
    return [c.name for c in cases]


def _line(name, what, err, bound, where, yard=None):
    y = "" if yard is None else f" yardstick {yard / EPS24:.2f}"
    print(f"\nSTEP_PARITY {name} {what}: err {err / EPS24:.2f} x 2^-24, bound {bound / EPS24:.2f}{y}, err / bound {err / bound:.2f} at {where}")


def _hold(name, what, got, ref, A, bound, allow=None, yard=None):
    err, where = parity_err(got, ref, A, allow)
    _line(name, what, err, bound, where, yard)
    assert err <= bound, f"{name} {what}: err {err:.3e} > bound {bound:.3e} at {where}: got {float(got[where]):.9g}, ref {float(ref[where]):.9g}"


# ------------------------------------------------------------------------------------------------ ode_stage / cfg_euler
def _stage_check(case, o, res):
    ref = su.stage_eval(case, o)
    b = su.stage_bounds(case)
    got_x = res["x"][o.xr] if (case.euler or case.last) else res["x_out"]
    _hold(case.name, "state", got_x, ref["acc"], ref["mag"], b["acc"])
    if not case.euler:
        _hold(case.name, "slope", res["k"], ref["k"], ref["K"], b["k"])
        has_u = torch.ones(case.Rc, dtype=torch.bool) if o.u_row is None else o.u_row >= 0
        pc = o.pred[:case.Rc, :case.n_mel]
        assert torch.equal(res["k"][~has_u], pc[~has_u]), "a row without an unconditional prediction: k == pc exactly"
        if case.g == 0.0 and not case.per_item and not case.apg:
            assert torch.equal(res["k"], pc), "g == 0: k == pc exactly"
    # rows no row_src entry names keep their bits (NaN); before the last stage x is not written at all
    if case.euler or case.last:
        mask = torch.ones(o.x.shape[0], dtype=torch.bool)
        mask[o.xr] = False
        assert su.same_bits(res["x"][mask], o.x[mask]), "a row of x outside row_src was written"
    else:
        assert su.same_bits(res["x"], o.x), "x was written before the last stage"


@pytest.mark.parametrize("case", SMALL_STAGE, ids=_ids(SMALL_STAGE))
def test_stage_and_euler_float64_parity(hip_tiny, case):
    """Every stage of every method x the four instantiations of ode_stage_kernel, and cfg_euler_kernel with and without row_src, over
    n_mel 4 / 100 / 128, ldp == n_mel / + 4 / 128, 1 / 3 / 86 rows, scalar and per-item strength, every u_row pattern."""
    eng = hip_tiny["f32"]
    o = case.ops()
    res = su.twice(lambda: su.stage_launch(eng, case, o))
    _stage_check(case, o, res)
    if case.guided and case.u_map == "identity":                        # u_row[r] = Rc + r is the plain kernel in bits
        plain = su.stage_launch(eng, case, o, u_row=None)
        for k in res:
            assert res[k] is None or su.same_bits(res[k], plain[k]), f"{k}: the identity map differs from the plain kernel"


@pytest.mark.parametrize("case", [c for c in SMALL_STAGE if c.apg and c.Rc == 86], ids=lambda c: c.name)
def test_apg_stage_with_zero_projection_is_the_guided_kernel(hip_tiny, case):
    """C_b == 0 on every item: the launch has the bits of the plain / guided kernel run with the per-item strengths A_b."""
    eng = hip_tiny["f32"]
    o = case.ops()
    o.apg_coef[:, 1] = 0.0
    a = su.stage_launch(eng, case, o)
    o.g_item = o.apg_coef[:, 0].clone()
    b = su.stage_launch(eng, case, o, apg=None)
    for k in a:
        assert a[k] is None or su.same_bits(a[k], b[k]), k


@pytest.mark.parametrize("case", [c for c in STAGE if c.Rc > 86], ids=lambda c: c.name)
def test_stage_wrap_equals_its_slices(hip_tiny, case):
    """21000 rows x 25 float4s = 525000 work items against the 524288 one trip of the capped grid covers: inside the bound, and bit for
    bit the same rows launched in slices of 86."""
    eng = hip_tiny["f32"]
    assert su.wraps(case.total, su.grid_for)
    o = case.ops()
    res = su.twice(lambda: su.stage_launch(eng, case, o))
    _stage_check(case, o, res)
    xdev, k, xo = su.framed(o.x), [], []
    for r0 in range(0, case.Rc, 86):
        r1 = min(r0 + 86, case.Rc)
        part = su.stage_launch(eng, case, o, rows=(r0, r1), xdev=xdev)
        if not case.euler:
            k.append(part["k"])
            xo.append(part["x_out"])
    assert su.same_bits(xdev[1].cpu(), res["x"])
    if not case.euler:
        assert su.same_bits(torch.cat(k), res["k"]) and su.same_bits(torch.cat(xo), res["x_out"])


# ------------------------------------------------------------------------------------------------ apg_reduce / apg_coef
APG = su.apg_cases()


@pytest.mark.parametrize("case", APG, ids=_ids(APG))
def test_apg_partials_and_coefficients(hip_tiny, case):
    """Partials in float64 against extended-precision sums with A = sum |terms| and the length of the fixed tree as the count; tiles past an
    item's length are not written; coefficients within one fp32 rounding of the float64 value."""
    eng = hip_tiny["f32"]
    o = case.ops()
    res = su.twice(lambda: su.apg_launch(eng, case, o))
    ref = su.apg_ref(case, o)
    written = torch.isfinite(ref["part"])
    assert bool((res["part"][~written] == su.FILL).all()), "a tile past the item's length was written"
    e = ((res["part"] - ref["part"]).abs() / ref["scale"])[written]
    lim = (ref["chain"][:, :, None] * su.EPS53).expand_as(ref["part"])[written]
    print(f"\nSTEP_PARITY {case.name} partials: worst err / bound {float((e / lim).max()):.3f} (chains of {int(ref['chain'].max())} float64 additions)")
    assert bool((e <= lim).all())
    cb = EPS24 * ref["coef"].abs() + ref["slack"]
    ce = (res["coef"].double() - ref["coef"]).abs()
    print(f"STEP_PARITY {case.name} coef: worst err / (2^-24 |coef|) {float((ce / (EPS24 * ref['coef'].abs()).clamp_min(1e-300)).max()):.3f}")
    assert bool((ce <= cb).all()), (res["coef"], ref["coef"])
    for b in range(case.B):
        if case.guided is not None and not case.guided[b]:
            assert res["coef"][b].tolist() == [0.0, 0.0]


# ------------------------------------------------------------------------------------------------ pack
PACK = su.pack_cases()


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
@pytest.mark.parametrize("case", PACK, ids=_ids(PACK))
def test_pack_is_the_gather(hip_tiny, case, dtype):
    """Bit-equal to the gather written in torch (bf16: its round-to-nearest-even); only_x leaves every other column's 7.0; the padding
    columns are exact zeros; rows outside the window keep their 7.0; NaN sits in every source row nobody names."""
    eng = hip_tiny["f32"]
    o = case.ops()
    for only_x in (False, True):
        res = su.twice(lambda: su.pack_launch(eng, case, o, only_x, dtype))
        want = su.pack_ref(case, o, only_x, dtype)[0]
        assert su.same_bits(res["out"], want), (case.name, only_x, int((res["out"].float() != want.float()).sum()))
    print(f"\nSTEP_PARITY {case.name} {dtype}: exact, {su.pack_total(case)} float4s" + (" (wraps)" if su.wraps(su.pack_total(case), su.grid_for) else ""))


# ------------------------------------------------------------------------------------------------ tables and lengths
def test_row_tables_and_guided_tables_are_the_contract(hip_tiny):
    """Every entry of every table equals the restated contract (checked against a row walk without a device), lies inside its range, and
    the sentinels around the tables are untouched -- whatever the device lengths: zero, negative, above N, summing past Rc or short of it."""
    eng = hip_tiny["f32"]
    plain, guided = su.table_cases()
    for case in plain:
        got = su.twice(lambda: su.tables_launch(eng, case))
        want = su.tables_restated(case)
        for k, v in want.items():
            assert got[k].tolist() == v, (case.name, k)
        su.table_ranges(case, {k: v.tolist() for k, v in got.items()})
    for case in guided:
        got = su.twice(lambda: su.tables_launch(eng, case))
        want = su.guided_restated(case)
        for k, v in want.items():
            assert got[k].tolist() == v, (case.name, k, got[k].tolist(), v)
        su.table_ranges(case, {k: v.tolist() for k, v in got.items()})
    print(f"\nSTEP_PARITY tables: {len(plain)} row_tables and {len(guided)} guided_tables cases exact")


@pytest.mark.parametrize("case", su.len_cases(), ids=lambda c: c.name)
def test_length_kernels_are_exact(hip_tiny, case):
    """ref_len, decode_len and vocos_lens at B = 1 / 10 / 64 / 65 with lengths at, below and above every clamp: negative, above N, a
    reference longer than the sequence, a slice longer than T_max."""
    eng = hip_tiny["f32"]
    o = case.ops()
    got = su.len_launch(eng, case, o)
    want = su.len_ref(case, o)
    assert got == want, {k: (got[k], want[k]) for k in want if got[k] != want[k]}


@pytest.mark.parametrize("n", su.ROPE_SIZES)
@pytest.mark.parametrize("rows", su.ROPE_SIZES)
def test_rope_gathers_are_exact(hip_tiny, n, rows):
    eng = hip_tiny["f32"]
    pos = su.rope_positions(n, rows)
    got, want = su.rope_launch(eng, n, pos)
    for k in want:
        assert su.same_bits(got[k], want[k]), (k, n, rows)


# ------------------------------------------------------------------------------------------------ mel_slice / im2col
SLICE = su.slice_cases()


@pytest.mark.parametrize("case", SLICE, ids=_ids(SLICE))
def test_mel_slice_and_im2col_are_exact(hip_tiny, case):
    """Generated lengths 0 / 1 / T and more, ref_len 0 and past seq_len, seq_len past N, and negative ref_len: a clamped item that starts
    at its row 0, with the NaN guard rows in front of x unread."""
    eng = hip_tiny["f32"]
    o = case.ops()
    want = su.slice_ref(case, o)
    mel = su.twice(lambda: su.slice_launch(eng, case, o, "mel"))["out"]
    assert su.same_bits(mel, want["mel"]), case.name
    for k in (case.k, 1):
        c2 = su.dataclasses.replace(case, k=k)
        cols = su.twice(lambda: su.slice_launch(eng, c2, o, "cols"))["out"]
        assert su.same_bits(cols, su.slice_ref(c2, o)["cols"]), (case.name, k)


def test_im2col_wrap(hip_tiny):
    """B = 2, T_max = 6000, ld_out 704: 2.1 M float4s against the 8192 workgroups of grid_1d."""
    eng = hip_tiny["f32"]
    T = 6000
    case = su.SliceCase("slice/im2col_wrap", 100, T, T + 40, (T + 30, 2500), (30, -7), k=7, ld_extra=4)
    assert su.wraps(case.B * T * ((7 * 100 + 4) // 4), su.grid_1d)
    o = case.ops()
    cols = su.twice(lambda: su.slice_launch(eng, case, o, "cols"))["out"]
    assert su.same_bits(cols, su.slice_ref_fast(case, o))


# ------------------------------------------------------------------------------------------------ vocos_spectrum
SPEC = su.spec_cases()


@pytest.mark.parametrize("case", SPEC, ids=_ids(SPEC))
def test_spectrum_float64_parity(hip_tiny, case):
    """mag cos p / mag sin p from the fp32 head values, A_e = mag: log-magnitudes on both sides of the clip, -100 and +90; phases 0,
    +-pi, +-50 ... +-1e8.  Column n/2 holds mag cos p and no sine is stored for it or for column 0 (the element behind the plane and
    every row's column 0 are compared too).  Bound: 4 x the CPU library's fp32 error over a floor of 3 x 2^-24."""
    eng = hip_tiny["f32"]
    o = case.ops()
    ref, A = su.spec_eval(case, o)
    yard = parity_err(su.spec_eval(case, o, torch.float32)[0], ref, A, su.F32_MIN_NORMAL)[0]
    got = su.twice(lambda: su.spec_launch(eng, case, o))["out"]
    assert bool(torch.isfinite(got).all()) and float(got[:-1].abs().max()) <= 100.0
    _hold(case.name, "out", got, ref, A, su.bound_of(su.SPECTRUM_FLOOR_C, yard), su.F32_MIN_NORMAL, yard)


# ------------------------------------------------------------------------------------------------ vocos_ola
OLA = su.ola_cases()


@pytest.mark.parametrize("case", OLA, ids=_ids(OLA))
def test_ola_float64_parity_and_exact_pcm(hip_tiny, case):
    eng = hip_tiny["f32"]
    o = case.ops()
    ref, A, plen = su.ola_eval(case, o)
    res = su.twice(lambda: su.ola_launch(eng, case, o))
    assert res["pcm_len"].tolist() == plen
    alone = su.ola_launch(eng, case, o, items=list(range(case.B)))
    for k in res:
        assert res[k] is None or su.same_bits(res[k], alone[k]), f"{k}: an item alone differs from the item in the batch"
    L = case.T_max * case.hop
    for b, n in enumerate(plen):
        assert not res["pcm"][b, n:L].any(), "samples at and beyond hop (T_b - 1) are exact zeros"
    if case.wave:
        for b, n in enumerate(plen):
            assert not res["wave"][b, n:L].any()
        yard = parity_err(su.ola_eval(case, o, torch.float32)[0], ref, A)[0]
        _hold(case.name, "wave", res["wave"], ref, A, su.bound_of(case.c, yard), yard=yard)
        assert torch.equal(res["pcm"], su.pcm_of(res["wave"])), "pcm != trunc(clamp(fl32(wave x 32767))) of the waveform the launch returned"
    else:
        want = su.pcm_of(ref.float())
        assert int((res["pcm"].int() - want.int()).abs().max()) <= 1


# ------------------------------------------------------------------------------------------------ conv_post
POST = su.post_cases()


@pytest.mark.parametrize("case", POST, ids=_ids(POST))
def test_conv_post_float64_parity_and_exact_pcm(hip_tiny, case):
    """tanh(conv(lrelu(zero-filled x)) + bias) per element for each instantiation, valid lengths on both sides of the wave seam (248) and
    the workgroup seam (992) in every residue mod 4 -- so that element 0 of a 16-byte load that straddles the valid length is the row's last
    valid sample -- and 0, 1, 3, 4, 5, T, negative and past T; the PCM is the truncation of the waveform the launch returned."""
    eng = hip_tiny["f32"]
    o = case.ops()
    ref, A = su.post_eval(case, o)
    yard = parity_err(su.post_eval(case, o, torch.float32)[0], ref, A)[0]
    res = su.twice(lambda: su.post_launch(eng, case, o))
    _hold(f"{case.name} <VEC={int(case.form[0])}, CB={case.form[1]}>", "wave", res["wave"], ref, A, su.bound_of(su.POST_C, yard), yard=yard)
    assert torch.equal(res["pcm"], su.pcm_of(res["wave"])), "pcm != trunc(clamp(fl32(wave x 32767))) of the waveform the launch returned"


# ------------------------------------------------------------------------------------------------ refusals
def _refusals(eng):
    """name -> (call, message): one violated precondition each, on otherwise valid arguments.  Outputs hold 7.0 / a sentinel before."""
    L, ctx, st = eng.lib, eng.ctx, su.stream()
    f = lambda *s, v=su.FILL: torch.full(s, v, device=DEV)
    i = lambda *s: torch.full(s, 1, dtype=torch.int32, device=DEV)
    x, pred, out, cat = f(16, 8), f(16, 16), f(16, 16), f(16, 8)
    outb = torch.full((16, 16), su.FILL, dtype=torch.bfloat16, device=DEV)
    tab, pcm = i(64), torch.full((4, 64), 1234, dtype=torch.int16, device=DEV)
    P = lambda t, off=0: t.data_ptr() + off
    bufs = dict(x=x, pred=pred, out=out, cat=cat, outb=outb, tab=tab, pcm=pcm)
    R = {}

    def eul(**k):
        a = dict(x=P(x), pred=P(pred), ldp=16, BN=8, M=8)
        a.update(k)
        return lambda: L.vv_cfg_euler(ctx, a["x"], a["pred"], a["ldp"], a["BN"], a["M"], 2.0, 0.1, st)
    w4, rng, nul, al = "cfg_euler: widths must be multiples of 4", "cfg_euler: BN >= 1, n_mel >= 4, ldp >= n_mel", "cfg_euler: x and pred are required", \
        "cfg_euler: x and pred must be 16-byte aligned"
    R.update({"euler/n_mel_mod_4": (eul(M=6), w4), "euler/ldp_mod_4": (eul(ldp=18), w4), "euler/BN_zero": (eul(BN=0), rng),
              "euler/BN_negative": (eul(BN=-3), rng), "euler/n_mel_zero": (eul(M=0), rng), "euler/ldp_below_n_mel": (eul(ldp=4), rng),
              "euler/x_null": (eul(x=None), nul), "euler/pred_null": (eul(pred=None), nul), "euler/x_misaligned": (eul(x=P(x, 4)), al),
              "euler/pred_misaligned": (eul(pred=P(pred, 8)), al)})
    R["euler_rows/BN_zero"] = (lambda: L.vv_cfg_euler_rows(ctx, P(x), P(pred), 16, 0, 8, 2.0, 0.1, P(tab), st), rng)
    R["euler_rows/x_misaligned"] = (lambda: L.vv_cfg_euler_rows(ctx, P(x, 4), P(pred), 16, 8, 8, 2.0, 0.1, P(tab), st), al)
    R["euler_rows/row_src_misaligned"] = (lambda: L.vv_cfg_euler_rows(ctx, P(x), P(pred), 16, 8, 8, 2.0, 0.1, P(tab, 2), st),
                                          "vv_cfg_euler_rows: every array must be 4-byte aligned")

    def pk(guided=False, **k):
        a = dict(dt=rt.VV_F32, x=P(x), cat=P(cat), drop=P(cat), out=P(out), ldo=16, BN=4, M=8, CD=8, only_x=0, rs=P(tab), us=P(tab), uc=P(tab), row0=0, n=4)
        a.update(k)
        if guided:
            return lambda: L.vv_pack_cat_guided(ctx, a["dt"], a["x"], a["cat"], a["drop"], a["out"], a["ldo"], a["BN"], a["row0"], a["n"], a["M"], a["CD"],
                                                a["only_x"], 0, a["rs"], a["us"], a["uc"], st)
        return lambda: L.vv_pack_cat(ctx, a["dt"], a["x"], a["cat"], a["drop"], a["out"], a["ldo"], a["BN"], a["M"], a["CD"], a["only_x"], a["rs"], st)
    for g, name in ((False, "pack_cat"), (True, "pack_cat_guided")):
        req, ali = f"{name}: x, out and (unless only_x) cat and cat_drop are required", f"{name}: x, cat and cat_drop must be 16-byte aligned"
        R.update({f"{name}/ldo_short": (pk(g, ldo=12), f"{name}: bad widths"), f"{name}/n_mel_mod_4": (pk(g, M=6, CD=10), f"{name}: bad widths"),
                  f"{name}/ldo_mod_4": (pk(g, ldo=18), f"{name}: bad widths"), f"{name}/x_null": (pk(g, x=None), req),
                  f"{name}/out_null": (pk(g, out=None), req), f"{name}/cat_null": (pk(g, cat=None), req), f"{name}/cat_drop_null": (pk(g, drop=None), req),
                  f"{name}/x_misaligned": (pk(g, x=P(x, 4)), ali), f"{name}/cat_misaligned": (pk(g, cat=P(cat, 8)), ali),
                  f"{name}/cat_drop_misaligned": (pk(g, drop=P(cat, 4)), ali), f"{name}/out_f32_misaligned": (pk(g, out=P(out, 8)), ali),
                  f"{name}/out_bf16_misaligned": (pk(g, dt=rt.VV_BF16, out=P(outb, 4)), ali),
                  f"{name}/dtype": (pk(g, dt=7), f"vv_{name}: dtype must be VV_DTYPE_F32 or VV_DTYPE_BF16"),
                  f"{name}/n_mel_zero": (pk(g, M=0), f"{name}: " + ("n_mel >= 4" if g else "BN >= 1, n_mel >= 4")),
                  f"{name}/table_misaligned": (pk(g, rs=P(tab, 2)), f"vv_{name}: every array must be 4-byte aligned")})
    R["pack_cat/BN_zero"] = (pk(BN=0), "pack_cat: BN >= 1, n_mel >= 4")
    tabs = "pack_cat_guided: rows and their three tables"
    R.update({"pack_cat_guided/Rc_zero": (pk(True, BN=0), tabs), "pack_cat_guided/row0_negative": (pk(True, row0=-1), tabs),
              "pack_cat_guided/n_rows_zero": (pk(True, n=0), tabs), "pack_cat_guided/u_src_null": (pk(True, us=None), tabs),
              "pack_cat_guided/u_crow_null": (pk(True, uc=None), tabs), "pack_cat_guided/row_src_null": (pk(True, rs=None), tabs)})

    xin, w = f(2, 8, 64, v=0.5), f(8, 7, v=0.1)

    def post(**k):
        a = dict(x=P(xin), w=P(w), pcm=P(pcm), ld=64, B=2, C=8, T=64, KW=7, slope=0.01)
        a.update(k)
        return lambda: L.vv_conv_post(ctx, a["x"], a["w"], 0.0, a["pcm"], a["ld"], P(out), a["B"], a["C"], a["T"], a["KW"], a["slope"], None, st)
    shp, req = "conv_post: B >= 1, T >= 1 and ld_pcm >= T", "conv_post: in, w and pcm are required"
    R.update({"conv_post/B_zero": (post(B=0), shp), "conv_post/T_zero": (post(T=0), shp), "conv_post/T_negative": (post(T=-4), shp),
              "conv_post/ld_pcm_short": (post(ld=63), shp), "conv_post/in_null": (post(x=None), req), "conv_post/w_null": (post(w=None), req),
              "conv_post/pcm_null": (post(pcm=None), req), "conv_post/KW_5": (post(KW=5), "conv_post: k=7 and C<=64 expected"),
              "conv_post/C_65": (post(C=65), "conv_post: k=7 and C<=64 expected"), "conv_post/C_zero": (post(C=0), "conv_post: k=7 and C<=64 expected"),
              "conv_post/slope_zero": (post(slope=0.0), "conv_post: pre_slope must be in (0, 1]")})

    def ms(**k):
        a = dict(x=P(x), B=2, N=8, M=8, rl=P(tab), sl=P(tab), out=P(out), T=4)
        a.update(k)
        return lambda: L.vv_mel_slice(ctx, a["x"], a["B"], a["N"], a["M"], a["rl"], a["sl"], a["out"], a["T"], st)
    dims, req = "mel_slice: B, N and n_mel must be at least 1", "mel_slice: x, ref_len, seq_len and out are required"
    R.update({"mel_slice/T_zero": (ms(T=0), "mel_slice: empty"), "mel_slice/B_zero": (ms(B=0), dims), "mel_slice/N_zero": (ms(N=0), dims),
              "mel_slice/n_mel_zero": (ms(M=0), dims), "mel_slice/x_null": (ms(x=None), req), "mel_slice/ref_len_null": (ms(rl=None), req),
              "mel_slice/seq_len_null": (ms(sl=None), req), "mel_slice/out_null": (ms(out=None), req),
              "mel_slice/seq_len_misaligned": (ms(sl=P(tab, 2)), "vv_mel_slice: every array must be 4-byte aligned")})

    lens_msg = "decode_len: B, n_levels, N, T_max >= 1"
    R.update({"decode_len/B_zero": (lambda: L.vv_decode_len(ctx, P(tab), P(tab), P(tab, 64), 0, 2, P(tab), 8, 4, st), lens_msg),
              "decode_len/N_zero": (lambda: L.vv_decode_len(ctx, P(tab), P(tab), P(tab, 64), 2, 2, P(tab), 0, 4, st), lens_msg),
              "decode_len/mult_null": (lambda: L.vv_decode_len(ctx, P(tab), P(tab), P(tab, 64), 2, 2, None, 8, 4, st), lens_msg),
              "decode_len/lens_null": (lambda: L.vv_decode_len(ctx, P(tab), P(tab), None, 2, 2, P(tab), 8, 4, st), lens_msg),
              "ref_len/hop_zero": (lambda: L.vv_ref_len(ctx, P(tab), P(tab, 64), 2, 0, st), "ref_len: B >= 1, hop >= 1"),
              "ref_len/out_null": (lambda: L.vv_ref_len(ctx, P(tab), None, 2, 256, st), "ref_len: B >= 1, hop >= 1"),
              "vocos_lens/T_max_zero": (lambda: L.vv_vocos_lens(ctx, P(tab), P(tab), P(tab, 64), 2, 8, 0, st), "vocos_lens: bad arguments"),
              "row_tables/B_zero": (lambda: L.vv_row_tables(ctx, P(tab), 0, 8, 4, P(tab, 64), P(tab, 96), P(tab, 128), P(tab, 160), st), "row_tables: empty"),
              "row_tables/table_null": (lambda: L.vv_row_tables(ctx, P(tab), 2, 8, 4, P(tab, 64), None, P(tab, 128), P(tab, 160), st),
                                        "vv_row_tables: seq_len and the four tables are required")})
    fl = (C.c_uint8 * 4)(1, 0, 1, 1)
    gt = lambda B=2, Rc=4, Ru=2, flags=fl: (lambda: L.vv_guided_tables(ctx, P(tab), None if flags is None else C.cast(flags, C.c_void_p), B, 8, Rc, Ru,
                                                                         *[P(tab, 32 + 16 * j) for j in range(7)], st))
    gm = "guided_tables: 1..1024 items, 0 <= Ru <= Rc"
    R.update({"guided_tables/Ru_above_Rc": (gt(Ru=5), gm), "guided_tables/B_1025": (gt(B=1025), gm), "guided_tables/flags_null": (gt(flags=None), gm),
              "guided_tables/Ru_negative": (gt(Ru=-1), gm)})

    sp = lambda ld=18, R_=2, n=16, head=P(pred): (lambda: L.vv_vocos_spectrum(ctx, head, ld, R_, n, P(out), st))
    sm = "vocos_spectrum: bad arguments"
    R.update({"spectrum/R_zero": (sp(R_=0), sm), "spectrum/n_odd": (sp(n=15), sm), "spectrum/ld_head_short": (sp(ld=17), sm), "spectrum/head_null": (sp(head=None), sm)})

    def ola(**k):
        a = dict(fr=P(pred), ld_f=16, B=2, T=4, lens=P(tab), win=P(cat), n=16, hop=4, pcm=P(pcm), ld=64, wave=P(out), ldw=16)
        a.update(k)
        return lambda: L.vv_vocos_ola(ctx, a["fr"], a["ld_f"], a["B"], a["T"], a["lens"], a["win"], a["n"], a["hop"], a["pcm"], a["ld"], None, a["wave"],
                                      a["ldw"], st)
    om = "vocos_ola: bad arguments"
    R.update({"ola/n_fft_mod_hop": (ola(hop=5), om), "ola/ld_f_short": (ola(ld_f=12), om), "ola/ld_pcm_short": (ola(ld=15), om),
              "ola/ld_wave_short": (ola(ldw=15), om), "ola/hop_zero": (ola(hop=0), om), "ola/lens_null": (ola(lens=None), om), "ola/window_null": (ola(win=None), om),
              "ola/pcm_null": (ola(pcm=None), om), "ola/n_fft_odd": (ola(n=15, hop=5), "vv_vocos_ola: n_fft must be even and at least 2"),
              "ola/pcm_misaligned": (ola(pcm=P(pcm, 1)), "vv_vocos_ola: pcm must be 2-byte aligned")})

    def im(**k):
        a = dict(x=P(x), M=8, k=3, out=P(out), ld=24)
        a.update(k)
        return lambda: L.vv_vocos_im2col_ex(ctx, a["x"], 1, 4, a["M"], P(tab), P(tab), 2, a["k"], a["out"], a["ld"], st)
    im_m = "vocos_im2col: bad arguments"
    R.update({"im2col/k_even": (im(k=2), im_m), "im2col/n_mel_mod_4": (im(M=6), im_m), "im2col/ld_out_short": (im(ld=20), im_m),
              "im2col/x_misaligned": (im(x=P(x, 4)), "vocos_im2col: operands must be 16-byte aligned"),
              "im2col/out_misaligned": (im(out=P(out, 8)), "vocos_im2col: operands must be 16-byte aligned")})
    return R, bufs


def test_refusals_return_22_with_their_message_and_write_nothing(hip_tiny):
    """Every argument set the launchers' checks name -- the alignment ones of cfg_euler and pack_cat among them -- returns -22 with the
    message of its own check before anything is launched: the outputs keep their fill, and the context runs a valid launch afterwards."""
    eng = hip_tiny["f32"]
    R, bufs = _refusals(eng)
    before = {k: v.clone() for k, v in bufs.items()}
    for name in sorted(R):
        call, message = R[name]
        rc = call()
        got = eng.lib.vv_last_error(eng.ctx).decode()
        assert rc == -22, (name, rc, got)
        assert got.startswith(message), (name, got)
    torch.cuda.synchronize()
    for k, v in bufs.items():
        assert su.same_bits(v.cpu(), before[k].cpu()), f"{k} was written by a refused call"
    assert len(R) >= 90
    case = SMALL_STAGE[0]
    _stage_check(case, case.ops(), su.stage_launch(eng, case, case.ops()))        # the context is usable afterwards
    print(f"\nSTEP_PARITY refusals: {len(R)} argument sets refused with -22 and their own message")


# ------------------------------------------------------------------------------------------------ through the Vocos context
def _vocos_engine():
    from tests.test_vocos_gpu import _engine                           # the suite's cached tiny Vocos engine
    from vietvoice_tts_amd.model_spec import ModelSpec
    spec = ModelSpec.tiny_vocos()
    return _engine(spec)[0], spec


def test_vocos_im2col_entry_clamps_a_negative_ref_len():
    """The exported vv_vocos_im2col with ref_len < 0 (and > seq_len, and seq_len > N): the item starts at its row 0, nothing in front of x
    is read -- x sits between NaN guard rows, so a row read in front of it would show in the operand."""
    from vietvoice_tts_amd import pack
    eng, spec = _vocos_engine()
    T = 9
    KE = pack.vocos_embed_k(spec)
    case = su.SliceCase("slice/context_entry", spec.n_mel, T, T + 6, (8, 12, T + 9, 5, 3), (-2, -40, 1, 7, 0), k=spec.vocos_embed_k,
                        ld_extra=KE - spec.vocos_embed_k * spec.n_mel)
    o = case.ops()
    xw, dx = su.framed(o.x, su.SLICE_FRONT, su.SLICE_FRONT)
    sl, rl = su.table(torch.tensor(case.seq_len), 10 ** 6), su.table(torch.tensor(case.ref_len), 10 ** 6)
    whole, out, guard = su.out_rows(case.B * T, KE)
    gu.check(eng, eng.lib.vv_vocos_im2col(eng.ctx, su.ptr(dx), case.B, case.N, su.ptr(rl[1]), su.ptr(sl[1]), T, su.ptr(out), KE, su.stream()))
    torch.cuda.synchronize()
    gu._bands_intact(whole, guard, su.FILL, case.name)
    su.frame_intact(xw, dx, case.name)
    assert su.same_bits(out.cpu(), su.slice_ref(case, o)["cols"])


def _ola64(fr, n, hop):
    """[T][n] -> the overlap-add [n + hop (T - 1)] in the dtype of fr."""
    T = fr.shape[0]
    acc = torch.zeros(n + hop * (T - 1), dtype=fr.dtype)
    for t in range(T):
        acc[t * hop:t * hop + n] += fr[t]
    return acc


def test_istft_head_per_element_bound():
    """vv_istft_head (spectrum, the K = n_fft GEMM against const.istft_basis, overlap-add) with phases up to +-1e4 rad, per element: the
    spectrum's bound and the GEMM's (gemm_bound of its yardstick) act on A_f = sum_k mag_k |basis|, the overlap-add's count on top, all
    over the envelope; the PCM is the truncation of the waveform the launch returned."""
    from vietvoice_tts_amd import pack
    eng, spec = _vocos_engine()
    n, hop, nb = spec.n_fft, spec.hop_length, spec.n_fft // 2 + 1
    T = [1, 2, 5, 12]
    B, T_max, ld = len(T), max(T), 1152
    g = torch.Generator().manual_seed(77)
    head = torch.full((B * T_max, ld), su.NAN)
    head[:, :nb] = -2.0 + torch.randn(B * T_max, nb, generator=g)
    loud = torch.rand(B * T_max, nb, generator=g) < 0.01
    head[:, :nb][loud] = 5.0
    head[:, nb:2 * nb] = (torch.rand(B * T_max, nb, generator=g) * 2 - 1) * 1e4
    for b, t in enumerate(T):
        head[b * T_max + t:(b + 1) * T_max] = su.NAN                   # frames past an item's length are never read ...
    hd = torch.where(torch.isnan(head), torch.zeros(()), head)          # ... by the overlap-add; the spectrum and the GEMM run on every row
    hd[:, 2 * nb:] = su.NAN
    for b, t in enumerate(T):
        hd[b * T_max + t:(b + 1) * T_max, :2 * nb] = 1e30               # what they hold there must not reach a valid sample
    L = T_max * hop
    hw, dh = su.framed(hd)
    frames = su.table(torch.tensor(T), 10 ** 6)
    pw, pcm = gu._guarded((B, L), 64, 1234, init=torch.full((B, L), 1234, dtype=torch.int16), dtype=torch.int16)
    ww, wave, wg = su.out_rows(B, L)
    plen = torch.full((B,), su.SENTINEL, dtype=torch.int32, device=DEV)
    gu.check(eng, eng.lib.vv_istft_head(eng.ctx, B, T_max, su.ptr(dh), ld, su.ptr(frames[1]), su.ptr(pcm), L, su.ptr(plen), su.ptr(wave), su.stream()))
    torch.cuda.synchronize()
    gu._bands_intact(pw, 64, 1234, "istft_head: pcm")
    gu._bands_intact(ww, wg, su.FILL, "istft_head: wave")
    wave, pcm = wave.cpu(), pcm.cpu()
    assert torch.equal(pcm, su.pcm_of(wave))
    basis, win = pack.istft_basis(spec), torch.hann_window(spec.win_length, periodic=True, dtype=torch.float32)
    k_ola = n // hop
    for b, t in enumerate(T):
        assert int(plen[b]) == hop * (t - 1)
        assert not wave[b, hop * (t - 1):].any()
        if t < 2:
            continue
        case = su.SpecCase("istft", 1e4, R=t, n=n, ld_extra=ld - n - 2)
        o = type("Ops", (), {})()
        o.head = hd[b * T_max:b * T_max + t]
        s64, As = su.spec_eval(case, o)
        s32 = su.spec_eval(case, o, torch.float32)[0]
        y_spec = parity_err(s32, s64, As, su.F32_MIN_NORMAL)[0]
        s64, As, s32 = s64[:-1].view(t, n), As[:-1].view(t, n), s32[:-1].view(t, n)
        f64 = s64 @ basis.double().T
        AF = As @ basis.double().abs().T
        # (sample 0 of a frame is exactly zero: the periodic Hann window starts at 0, so that basis row is zero and so is its scale)
        y_gemm = parity_err(s64.float() @ basis.T, s64.float().double() @ basis.double().T,
                            (s64.float().double().abs() @ basis.double().abs().T).clamp_min(1e-300))[0]
        assert y_spec < 4 * EPS24 and y_gemm <= (n + 8) * EPS24, (y_spec / EPS24, y_gemm / EPS24)       # the ceilings of the two yardsticks
        env = _ola64((win.double() ** 2).expand(t, n), n, hop)[n // 2:n // 2 + hop * (t - 1)]
        ref = _ola64(f64, n, hop)[n // 2:n // 2 + hop * (t - 1)] / env
        A = _ola64(AF, n, hop)[n // 2:n // 2 + hop * (t - 1)] / env
        bound = su.bound_of(su.SPECTRUM_FLOOR_C, y_spec) + gu.gemm_bound(y_gemm) + (2 * k_ola + 1) * EPS24
        err, where = parity_err(wave[b, :hop * (t - 1)], ref, A)
        _line(f"istft_head/T{t} (yardsticks: spectrum {y_spec / EPS24:.2f}, GEMM {y_gemm / EPS24:.2f})", "wave", err, bound, where)
        assert err <= bound, (t, err, bound)
