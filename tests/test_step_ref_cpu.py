"""No device: the claims tests/test_step_gpu.py rests on (tests/step_util.py).

1. The case lists reach what they say: the wrap cases exceed the grid caps restated from grid_for / grid_1d, the conv_post lengths hit the
   wave seam (248) and the workgroup seam (992) in every residue mod 4, every instantiation and branch has a case.
2. The table restatements agree with a row-by-row construction, and every entry lies inside the buffer it indexes.
3. Every bound has a ceiling: the fp32 CPU evaluation (the yardstick) is below half its count (three quarters for the stage kernel's
   slope, whose bound is the derived count alone and whose worst case is 3 of its 4), so no count is tighter than fp32 arithmetic itself.
4. The mutation table: each plausible bug, applied to the float64 reference and stored in the output dtype, misses the bound (or the exact
   comparison) on every case it applies to; the cases it skips are listed with the reason.  For the kernels that had a test before, the
   number of cases on which the previous tolerance lets the mutation through is printed (profiles/step_parity/notes.md records it)."""
import collections

import numpy as np
import pytest
import torch

from tests import step_util as su
from tests.gpu_util import EPS24, parity_err

STAGE = su.stage_cases()
SMALL_STAGE = [c for c in STAGE if c.Rc <= 86]


def _report(group, table):
    print(f"\nSTEP_MUTATIONS {group}")
    for mut, (caught, skipped, old_pass) in table.items():
        why = "; ".join(f"{n} x {r}" for r, n in collections.Counter(skipped).items())
        print(f"  {mut}: rejected on {caught} cases, skipped {len(skipped)}" + (f" ({why})" if why else "") +
              ("" if old_pass is None else f"; the previous tolerance accepts it on {old_pass}"))


# ------------------------------------------------------------------------------------------------ 1. what the cases reach
def test_wrap_cases_exceed_the_grid_caps():
    assert su.grid_for(10 ** 9) == 2048 and su.grid_1d(10 ** 9) == 8192
    wraps = [c for c in STAGE if "wrap" in c.name]
    assert {c.inst for c in wraps} == {"plain", "euler_rows"}
    for c in wraps:
        assert c.total == 525000 > 2048 * 256 == 524288 and su.wraps(c.total, su.grid_for)
    for c in SMALL_STAGE:
        assert not su.wraps(c.total, su.grid_for)
    packs = {c.name: c for c in su.pack_cases()}
    for name in ("pack/wrap", "pack_guided/wrap"):
        assert su.wraps(su.pack_total(packs[name]), su.grid_for)
    spec = [c for c in su.spec_cases() if "wrap" in c.name][0]
    assert su.wraps(spec.R * (spec.n // 2 + 1), su.grid_1d) and spec.R == 4100
    B, T, ld = IM2COL_WRAP
    assert su.wraps(B * T * (ld // 4), su.grid_1d) and (B, T) == (2, 6000)


IM2COL_WRAP = (2, 6000, 7 * 100 + 4)


def test_stage_cases_cover_every_shape_form_and_pattern():
    small = [c for c in SMALL_STAGE if not c.euler]
    for inst in ("plain", "guided", "apg", "apg_guided"):
        mine = [c for c in small if c.inst == inst]
        assert {(c.method, c.stage) for c in mine} == set(su.method_stages())          # every coefficient pattern of every method
        assert {c.Rc for c in mine} == {1, 3, 86}
        assert {(c.n_mel, c.ldp) for c in mine} == set(su.STAGE_SHAPES)
        assert {c.per_item for c in mine} == {False, True}
    assert {c.g for c in small if not c.per_item and not c.apg} == set(su.STAGE_G)
    assert {(c.n_mel, c.ldp) for c in small} == set(su.STAGE_SHAPES) and {s[0] for s in su.STAGE_SHAPES} == {4, 100, 128}
    assert {c.u_map for c in small if c.inst == "guided"} == set(su.U_MAPS) == {c.u_map for c in small if c.inst == "apg_guided"}
    for c in small:                                                                       # zero coefficients travel as NULL buffers
        assert len(c.coef) == c.stage + 1
    assert any(c.coef[j] == 0 for c in small for j in range(c.stage))
    assert su.STAGE_LENS[3] == ((1, 1, 1), 5)                                            # items of length 1 whose rows are 0, 5, 10: r / seq_n != row_src[r] / seq_n
    for inst in ("euler", "euler_rows"):
        assert {(c.n_mel, c.ldp) for c in SMALL_STAGE if c.inst == inst} == set(su.STAGE_SHAPES)
    # APG reads x_e through row_src at stage 0 and packed later
    assert {bool(c.stage) for c in small if c.apg and c.rows} == {False, True}


def test_conv_post_cases_hit_both_seams_in_every_residue():
    assert su.POST_WAVE == 62 * 4 and su.POST_WG == 4 * su.POST_WAVE
    assert su.POST_WAVE in su.POST_SEAM_LENS and su.POST_WG in su.POST_SEAM_LENS
    for seam in (su.POST_WAVE, su.POST_WG):
        near = [v for v in su.POST_SEAM_LENS if abs(v - seam) <= 3]
        assert {v % 4 for v in near} == {0, 1, 2, 3} and min(near) < seam < max(near)
    cases = su.post_cases()
    forms = collections.defaultdict(list)
    for c in cases:
        forms[c.form].append(c)
    assert set(forms) == {(True, 8), (True, 4), (True, 1), (False, 1)}
    for f, cs in forms.items():
        lens = {v for c in cs for v in su.case_lens_raw(c)}
        assert set(su.POST_SEAM_LENS) <= lens and set(su.POST_SMALL_LENS) <= lens, f
    assert any(c.form == (False, 1) and c.T % 4 == 0 and c.shift == 1 for c in cases)    # the pointer moved by 4 bytes
    assert any((c.T + c.ld_extra) % 2 for c in cases)                                     # ld_pcm odd
    # the VEC form's element 0 is the last valid sample of a row: len % 4 in {1, 2, 3} on a 16-byte aligned row
    assert all({v % 4 for v in su.case_lens_raw(c) if 0 < v < c.T} == {0, 1, 2, 3} for c in cases if c.form[0] and c.T >= 1000)


def test_apg_cases_reach_the_tile_edges():
    T = su.APG_TILE
    lens = {n for c in su.apg_cases() for n in c.lens}
    assert {T - 1, T, T + 1, 1} <= lens
    names = {c.name for c in su.apg_cases()}
    assert {"apg/unguided_between", "apg/S2_zero", "apg/eta_one_and_caps"} <= names
    assert np.finfo(np.longdouble).eps <= 2.0 ** -60, "the extended-precision reference needs x87 long double"
    c = [c for c in su.apg_cases() if c.name == "apg/eta_one_and_caps"][0]
    o = c.ops()
    r = su.apg_ref(c, o)
    assert float(r["coef"][0, 1]) == 0.0 and float(r["coef"][1, 0]) < 0.9 * 2.0 and float(r["coef"][2, 0]) == 2.0   # eta 1; the cap binds; it does not
    z = [c for c in su.apg_cases() if c.name == "apg/S2_zero"][0]
    rz = su.apg_ref(z, z.ops())
    assert bool((rz["part"][:, 0, 1] == 0).all()) and bool((rz["coef"][:, 1] == 0).all())


# ------------------------------------------------------------------------------------------------ 2. the tables
def test_table_restatements_agree_with_the_row_walk():
    plain, guided = su.table_cases()
    assert {len(c.seq_len) for c in plain} >= {1, 3, 33, 65} <= {len(c.seq_len) for c in guided}
    for c in plain:
        t = su.tables_restated(c)
        assert t == su.tables_brute(c), c.name
        su.table_ranges(c, t)
        assert su.SENTINEL not in t["row_src"] and su.SENTINEL not in t["row_pos"], c.name      # every entry is written
    for c in guided:
        t = su.guided_restated(c)
        b = su.guided_brute(c)
        assert t == b, (c.name, {k: (t[k], b[k]) for k in t if t[k] != b[k]})
        su.table_ranges(c, t)
        nb = sum(1 for f in c.flags if f)
        B = len(c.seq_len)
        for k in ("row_pos", "u_src", "u_crow", "u_row"):
            assert su.SENTINEL not in t[k], (c.name, k)
        assert su.SENTINEL not in t["row_start"][:B + nb] and su.SENTINEL not in t["kv_len"][:B + nb] and su.SENTINEL not in t["rs_rel"][:nb]
    names = " ".join(c.name for c in guided)
    for tag in ("Ru0", "RuRc", "cut", "device_more", "device_fewer", "device_negative", "device_above_N", "zero_first", "zero_last", "zero_middle",
                "_last", "_notlast"):
        assert tag in names, tag


def test_table_mutations_are_rejected():
    plain, guided = su.table_cases()
    table = {}
    for mut in su.GUIDED_MUTATIONS:
        caught, skipped = 0, []
        pool = [(c, su.tables_restated) for c in plain] if mut == "prefix_unclamped" else []
        pool += [(c, su.guided_restated) for c in guided]
        for c, fn in pool:
            if fn(c, mut) == fn(c):
                skipped.append("the mutated rule gives the same tables for these lengths and flags")
            else:
                caught += 1
        table[mut] = (caught, skipped, None)
        assert caught >= 3, mut
    _report("tables (no unit test before: every case is new)", table)
    # where a mutation applies is a property of the case: lengths outside [0, N] or past Rc, a set flag next to a clear one, orphan rows
    for c in guided:
        out_of_range = any(v < 0 or v > c.N for v in c.seq_len)
        if out_of_range and "device_negative" in c.name:
            assert su.guided_restated(c, "prefix_unclamped") != su.guided_restated(c), c.name
        clamped = [min(max(v, 0), c.N) for v in c.seq_len]
        if sum(clamped) < c.Rc:
            assert su.guided_restated(c, "orphan_u_row_kept") != su.guided_restated(c), c.name


def test_length_rules():
    assert su.gen_slice(10, 4, 40) == (4, 6) and su.gen_slice(50, 4, 40) == (4, 36) and su.gen_slice(10, 12, 40) == (10, 0)
    assert su.gen_slice(10, -3, 40) == (0, 10) and su.gen_slice(-2, -3, 40) == (0, 0) and su.gen_slice(50, 45, 40, 12) == (40, 0)
    assert su.gen_slice(30, 4, 40, 12) == (4, 12)
    for c in su.len_cases():
        o = c.ops()
        r = su.len_ref(c, o)
        assert all(0 <= t <= c.T_max for t in r["vocos"]) and r["decode"][-1] == [t * c.mult[-1] for t in r["vocos"]]
        assert r["ref_len"][0] == 1 and (c.B == 1 or r["ref_len"][1] == 2)
    assert {c.B for c in su.len_cases()} >= {64, 65}


# ------------------------------------------------------------------------------------------------ 3. + 4. per kernel group
def _misses(got, ref, A, bound, allow=None):
    return parity_err(got, ref, A, allow)[0] > bound


@pytest.mark.parametrize("inst", ["plain", "guided", "apg", "apg_guided", "euler", "euler_rows"])
def test_stage_counts_have_a_ceiling_and_reject_the_mutations(inst):
    table = {m: [0, [], 0] for m in su.STAGE_MUTATIONS}
    worst = dict(k=0.0, acc=0.0)
    for case in [c for c in SMALL_STAGE if c.inst == inst]:
        o = case.ops()
        ref = su.stage_eval(case, o)
        yard = su.stage_yard(case, o, ref)
        b = su.stage_bounds(case)
        for key in ("k", "acc"):
            worst[key] = max(worst[key], yard[key] / b[key])
            # the stage bounds are the derived counts alone (no 4 x yardstick term, so their ceiling is the count itself); the fp32 CPU
            # evaluation, which rounds every product and sum on its own, must pass them: the worst-case count is 3 of the slope's 4
            assert yard[key] <= (0.75 if key == "k" else 0.5) * b[key], (case.name, key, yard[key] / EPS24)
        if case.g == 0.0 and not case.per_item and not case.apg:
            assert torch.equal(su.stage_eval(case, o, torch.float32)["k"], o.pred[:case.Rc, :case.n_mel])   # g == 0: k == pc exactly
        for mut in su.STAGE_MUTATIONS:
            why = su.stage_mut_applies(case, mut)
            if why:
                table[mut][1].append(why)
                continue
            m = su.stage_eval(case, o, mut=mut)
            miss_k = not case.euler and _misses(m["k"].float(), ref["k"], ref["K"], b["k"])
            miss_x = _misses(m["acc"].float(), ref["acc"], ref["mag"], b["acc"])
            assert miss_k or miss_x, (case.name, mut)
            table[mut][0] += 1
            if case.euler:                                                                 # test_cfg_euler: one whole-tensor rel_err < 1e-6
                old = float((m["acc"].float().double() - ref["acc"]).abs().max() / ref["acc"].abs().max())
                table[mut][2] += old < 1e-6
    print(f"\nSTEP_CEILING {inst}: the fp32 CPU evaluation reaches {worst['k']:.2f} (slope) and {worst['acc']:.2f} (state) of the bound")
    _report(f"stage / Euler, {inst}", {m: (v[0], v[1], v[2] if inst.startswith("euler") else None) for m, v in table.items()})
    applicable = {"plain": ("swap_sign", "item_of_r", "skip_coef"), "guided": ("swap_sign", "item_of_r", "skip_coef", "pu_from_Rc_r"),
                  "apg": ("swap_sign", "item_of_r", "skip_coef", "xe_from_r"), "apg_guided": su.STAGE_MUTATIONS,
                  "euler": ("swap_sign", "skip_coef"), "euler_rows": ("swap_sign", "skip_coef")}[inst]
    for mut in applicable:
        assert table[mut][0] >= 1, (inst, mut, "no case exercises this mutation")


def test_apg_mutations_are_rejected():
    table = {m: [0, []] for m in su.APG_MUTATIONS}
    for case in su.apg_cases():
        o = case.ops()
        ref = su.apg_ref(case, o)
        written = torch.isfinite(ref["part"])
        pb = ref["chain"][:, :, None] * su.EPS53
        cb = EPS24 * ref["coef"].abs() + ref["slack"]
        assert float((ref["slack"] / (EPS24 * ref["coef"].abs()).clamp_min(1e-300)).max()) < 1e-3      # the float64 share is far below the fp32 rounding
        for mut in su.APG_MUTATIONS:
            m = su.apg_ref(case, o, mut)
            bad_p = bool((((m["part"] - ref["part"]).abs() / ref["scale"])[written] > pb.expand_as(ref["part"])[written]).any())
            bad_c = bool(((m["coef"].float().double() - ref["coef"]).abs() > cb).any())
            if not (bad_p or bad_c):
                same = torch.equal(torch.nan_to_num(m["part"]), torch.nan_to_num(ref["part"])) and torch.equal(m["coef"], ref["coef"])
                assert same, (case.name, mut, "a mutation that changes the values must miss the bound")
                table[mut][1].append({"drop_tile_last_frame": "no guided row", "S1_over_S3": "C == 0 on every item (eta 1 or S2 == 0)",
                                      "cap_without_omt": "no cap binds, or t_e == 1"}[mut])
            else:
                table[mut][0] += 1
    _report("APG (coefficients were checked against a float64 rule before, partials never)", {m: (v[0], v[1], None) for m, v in table.items()})
    for mut in su.APG_MUTATIONS:
        assert table[mut][0] >= 2, mut


def test_pack_mutations_are_rejected():
    table = {m: [0, []] for m in su.PACK_MUTATIONS}
    for case in su.pack_cases():
        if "wrap" in case.name:
            continue
        o = case.ops()
        for only_x in (False, True):
            for dtype in (torch.float32, torch.bfloat16):
                ref, row0, n = su.pack_ref(case, o, only_x, dtype)
                assert bool(torch.isfinite(ref.float()).all()), case.name                 # no named source row holds NaN
                if not only_x and case.ldo > case.n_mel + case.cond_dim:
                    assert bool((ref[row0:row0 + n, case.n_mel + case.cond_dim:] == 0).all())
                for mut in su.PACK_MUTATIONS:
                    why = su.pack_mut_applies(case, mut, only_x, dtype)
                    if why:
                        table[mut][1].append(why)
                        continue
                    m = su.pack_ref(case, o, only_x, dtype, mut)[0]
                    assert not su.same_bits(m, ref), (case.name, only_x, dtype, mut)
                    table[mut][0] += 1
    _report("pack (no unit test before: every case is new)", {m: (v[0], v[1], None) for m, v in table.items()})
    for mut in su.PACK_MUTATIONS:
        assert table[mut][0] >= 4, mut


def test_slice_mutations_are_rejected():
    table = {m: [0, []] for m in su.SLICE_MUTATIONS}
    for case in su.slice_cases():
        o = case.ops()
        ref = su.slice_ref(case, o)
        assert bool(torch.isfinite(ref["mel"]).all()) and bool(torch.isfinite(ref["cols"]).all()), case.name
        assert torch.equal(ref["cols"], su.slice_ref_fast(case, o)), case.name
        gens = [su.gen_slice(s, r, case.N)[1] for s, r in zip(case.seq_len, case.ref_len)]
        assert {0, 1} <= set(gens) and any(g >= case.T for g in gens) and any(s > case.N for s in case.seq_len) and any(r < 0 for r in case.ref_len)
        for mut in su.SLICE_MUTATIONS:
            m = su.slice_ref(case, o, mut)
            same_mel = su.same_bits(m["mel"], ref["mel"])
            same_cols = su.same_bits(m["cols"], ref["cols"])
            if mut == "no_tap_offset":
                assert same_mel and not same_cols, case.name                              # mel_slice has no taps
            else:
                assert not same_mel and not same_cols, (case.name, mut)
            table[mut][0] += 1
    _report("mel_slice / im2col (checked only through a whole decode before)", {m: (v[0], v[1], None) for m, v in table.items()})


def test_spectrum_floor_ceiling_and_mutations():
    table = {m: [0, []] for m in su.SPEC_MUTATIONS}
    for case in su.spec_cases():
        if "wrap" in case.name:
            continue
        o = case.ops()
        ref, A = su.spec_eval(case, o)
        assert bool(torch.isfinite(ref).all()) and float(ref[:-1].abs().max()) <= 100.0           # +90 gives 100, not inf or NaN
        yard = parity_err(su.spec_eval(case, o, torch.float32)[0], ref, A, su.F32_MIN_NORMAL)[0]
        bound = su.bound_of(su.SPECTRUM_FLOOR_C, yard)
        print(f"\nSTEP_YARDSTICK {case.name}: yardstick {yard / EPS24:.2f} x 2^-24, bound {bound / EPS24:.2f} x 2^-24")
        assert yard <= 4.0 * EPS24, (case.name, yard / EPS24)            # the CPU library stays within 2 ulp of the float64 value at every phase
        for mut in su.SPEC_MUTATIONS:
            m = su.spec_eval(case, o, mut=mut)[0].float()
            if _misses(m, ref, A, bound, su.F32_MIN_NORMAL):
                table[mut][0] += 1
            else:
                assert mut == "fast_sine" and case.phase < 1e4, (case.name, mut)
                table[mut][1].append("below 1e4 rad a single-float 2 pi reduction is still inside the bound of some phases")
    _report("spectrum (reached only through vv_istft_head, phases to 50 rad, before)", {m: (v[0], v[1], None) for m, v in table.items()})
    assert table["fast_sine"][0] >= 3 and table["no_clip"][0] == table["sine_at_n"][0] == len(su.PHASES)


def test_ola_count_ceiling_and_mutations():
    table = {m: [0, [], 0] for m in su.OLA_MUTATIONS + ("round_nearest",)}
    for case in su.ola_cases():
        o = case.ops()
        ref, A, plen = su.ola_eval(case, o)
        assert bool(torch.isfinite(ref).all()), case.name                                 # no frame past an item's length is read
        y32 = su.ola_eval(case, o, torch.float32)[0]
        yard = parity_err(y32, ref, A)[0]
        bound = su.bound_of(case.c, yard)
        assert yard <= 0.5 * case.c * EPS24, (case.name, yard / EPS24)
        for mut in su.OLA_MUTATIONS:
            m = su.ola_eval(case, o, mut=mut)[0].float()
            assert _misses(m, ref, A, bound), (case.name, mut)
            table[mut][0] += 1
            d = (m.double() - ref).abs()
            table[mut][2] += bool(torch.isfinite(d).all()) and float(d.max()) < 2e-4       # test_istft_head_matches_torch_istft: 2e-4 absolute
        big = ref.float() * 3.0                                                           # spread over the int16 range
        assert not torch.equal(su.pcm_of(big), su.pcm_of(big, "round_nearest")), case.name
        table["round_nearest"][0] += 1
        table["round_nearest"][2] += int((su.pcm_of(big).int() - su.pcm_of(big, "round_nearest").int()).abs().max()) <= 2      # +-2 PCM steps
    _report("OLA and PCM", {m: tuple(v) for m, v in table.items()})


def test_conv_post_ceiling_and_mutations():
    table = {m: [0, [], 0] for m in su.POST_MUTATIONS + ("round_nearest",)}
    for case in su.post_cases():
        o = case.ops()
        ref, A = su.post_eval(case, o)
        y32 = su.post_eval(case, o, torch.float32)[0]
        yard = parity_err(y32, ref, A)[0]
        bound = su.bound_of(su.POST_C, yard)
        assert yard <= 0.5 * su.POST_C * EPS24, (case.name, yard / EPS24)
        for mut in su.POST_MUTATIONS:
            m = su.post_eval(case, o, mut=mut)[0].float()
            if mut == "mask_at_T" and all(v is None or v >= case.T for v in case.lens):
                table[mut][1].append("every length is T")
                continue
            if case.T < 4 and torch.equal(m, ref.float()):
                table[mut][1].append("a row of one sample: the mutated rule computes the same values")
                continue
            assert _misses(m, ref, A, bound), (case.name, mut)
            table[mut][0] += 1
            table[mut][2] += float((m.double() - ref).abs().max()) < 2e-6                  # test_conv_post_stream_kernel_forms: 2e-6 absolute
        assert not torch.equal(su.pcm_of(ref.float()), su.pcm_of(ref.float(), "round_nearest")) or case.T < 4
        if case.T >= 4:
            table["round_nearest"][0] += 1
            table["round_nearest"][2] += int((su.pcm_of(ref.float()).int() - su.pcm_of(ref.float(), "round_nearest").int()).abs().max()) <= 1
    _report("conv_post and PCM", {m: tuple(v) for m, v in table.items()})
    for mut in su.POST_MUTATIONS:
        assert table[mut][0] >= 9, mut


@pytest.mark.parametrize("case", [c for c in STAGE if c.Rc > 86], ids=lambda c: c.name)
def test_a_missing_second_trip_is_rejected_only_by_the_wrap_cases(case):
    """The grid-stride loop's second trip left out: the float4s past the 2048 x 256 the capped grid covers keep what the buffer held.  No
    launch of the suite before these cases was large enough to have such elements."""
    o = case.ops()
    ref = su.stage_eval(case, o)
    b = su.stage_bounds(case)
    covered = su.grid_for(case.total) * 256 * 4                          # elements one trip writes
    acc = ref["acc"].float().reshape(-1).clone()
    stale = o.x[o.xr].reshape(-1) if case.euler else torch.full_like(acc, su.FILL)
    acc[covered:] = stale[covered:]
    assert covered < acc.numel() and _misses(acc.view_as(ref["acc"]), ref["acc"], ref["mag"], b["acc"])
    for small in SMALL_STAGE:
        assert su.grid_for(small.total) * 256 >= small.total
