#!/usr/bin/env python3
"""The kernels of csrc/vv_elementwise.hip on the CPU under sanitizers, against the mirrors and under the bounds of the device tests.

Builds tools/elementwise_host_check.cpp (the kernel source on tools/hip_host_shim.h, exact-size heap buffers) twice, with
-fsanitize=address,undefined and with -fsanitize=thread.  Cases, references and bounds are those of tests/gpu_util.py (ln_*, gn_*, te_*,
dw_*, grn_*), tests/step_util.py (stage_*, apg_*, pack_*, table_cases, len_*, rope_*), tests/cfg_reuse_util.py, tests/block_cache_util.py,
tests/cfg_norm_util.py and tests/multistep_util.py; nothing is fitted here.  Exact kernels (pack, tables, lengths, rope, text_embed, build_cat, ode_diff_*,
cfg_drift_*, block_span, block_drift_*) are compared bit for bit; the others under the bound function of their device test (ln_bound, gn_bound, dw_bound, the
GRN counts, the stage counts, the APG chain bound).  rsqrtf and the Mish branch of act_apply run on the shim's stand-ins (1 / sqrtf;
exp2f and a division): those results speak for the indexing and the barriers of their paths, not for the device's functions.

Buffers: every operand is an exact block; a plane with a leading dimension starts with its first row at element 0 and ends with its
last row; outputs are filled with 0xAA and what no thread owns (padding columns, partials of tiles past an item's length, rows past Rc)
must still hold it; inputs hold NaN in their padding columns.

Grids, restated from the launchers of csrc/vv_elementwise.hip (which stay outside the guards):
  ln_mod              vvk_ln_mod: `grid = (a->R + 3) / 4`, 256 threads; tail_row0 = R and tp = 0 without a tail
  groupnorm           vvk_groupnorm: `dim3 grid(G, B)`, 256
  grn                 vvk_grn: `dim3 g1(C / 64, n_seq)`, `rpb = 16`, `dim3 g2((N + rpb - 1) / rpb, n_seq)`, LDS `C * sizeof(float)`
  apg / diff / drift / cfg_gram  `dim3(a->n_tiles, a->B)`, 256; the finishing kernels (cfg_norm_coef among them) `a->B` workgroups of 64
  tables              `row_tables_kernel<<<B, 256>>>`, `guided_tables_kernel<<<B, 256>>>`
  lengths             `(B + 63) / 64` workgroups of 64
  rope                `(n * 32 + 255) / 256` and `(rows * 16 + 255) / 256`: the device's (no grid-stride loop)
  block_drift         `dim3(a->n_tiles, a->n_seq)`, 256; the finishing kernel `a->n_seq` workgroups of 64
  the grid-stride kernels (pack, cfg_euler, ode_stage, text_embed, dwconv, build_cat, block_span): `grid_for(total)`, but at most 2 workgroups, so
  that the loop takes further trips (this replaces the device's 21000-row wrap cases)

The reduced list (tests/test_host_sanitizers_cpu.py) keeps every edge named in profiles/host_sanitizers/notes.md and drops repeats of
the same path.  Needs no GPU.

    python tools/elementwise_host_check.py [--cxx clang++] [--keep DIR] [--san asan|tsan|both] [--reduced]"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import host_check_common as H  # noqa: E402
import numpy as np  # noqa: E402

NAME = "elementwise"
NANF = np.float32("nan")


def find_cxx():
    return H.find_cxx()


def build(cxx, work, san="asan"):
    return H.build(NAME, cxx, work, san)


def _mods():
    if H.ROOT not in sys.path:
        sys.path.insert(0, H.ROOT)
    import torch
    from tests import gpu_util as gu
    from tests import step_util as su
    return torch, gu, su


# ---------------------------------------------------------------------------------------------------- buffers
def npy(t):
    """torch tensor -> numpy (bf16 as its 16-bit words)."""
    import torch
    t = t.detach().contiguous()
    return t.view(torch.int16).numpy().copy() if t.dtype == torch.bfloat16 else t.numpy().copy()


def tor(a, like=None):
    """numpy -> torch; like = torch.bfloat16: the 16-bit words are bf16."""
    import torch
    t = torch.from_numpy(np.ascontiguousarray(a).copy())
    return t.view(torch.bfloat16) if like == torch.bfloat16 else t


def plane(a, ld, fill=None):
    """[R][W] -> flat [(R - 1) ld + W]: row r at r ld, the last row ends the block; padding columns hold `fill` (None: 0xAA bytes)."""
    R, W = a.shape
    flat = H.filled(((R - 1) * ld + W,), a.dtype)
    if fill is not None:
        flat[:] = fill
    flat[_idx(R, W, ld)] = a
    return flat


def _idx(R, W, ld):
    return (np.arange(R)[:, None] * ld + np.arange(W)[None, :])


def rows_of(flat, R, W, ld):
    return flat[_idx(R, W, ld)]


def pad_of(flat, R, W, ld):
    m = np.ones(flat.shape, bool)
    m[_idx(R, W, ld).reshape(-1)] = False
    return flat[m]


def same_bytes(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def grid2(total):
    """grid_for of vv_elementwise.hip, at most 2 workgroups."""
    return max(1, min((total + 255) // 256, 2))


def holds(fn):
    """fn asserts; -> whether it passed (the message of a failure is printed)."""
    try:
        fn()
        return True
    except AssertionError as e:
        print(f"    {str(e)[:300]}", flush=True)
        return False


def cover(cases, key):
    """The cases that bring a value of some attribute no earlier case had: key(case) -> [(attribute, value)]."""
    seen, out = set(), []
    for c in cases:
        k = set(key(c))
        if k - seen:
            out.append(c)
            seen |= k
    return out


# ---------------------------------------------------------------------------------------------------- LayerNorm
def ln_list(reduced):
    torch, gu, su = _mods()
    cs = gu.ln_cases() + gu.ln_host_cases()
    if reduced:
        cs = cover(cs, lambda c: [("form", c.out_bf16, c.delta_bf16, c.D in (4, 252, 256, 260, 1024) and c.D), ("R", c.R), ("nd", c.n_delta, c.keep_x),
                                  ("wb", c.has_w, c.has_b), ("tail", c.tail_parts, c.tail_row0 >= c.R, c.tail_row0 % 4 != 0)])
    return [(c, pad) for c in cs for pad in (0, 4)]


def ln_add(bt, case, pad):
    torch, gu, su = _mods()
    o = case.ops()
    R, D = case.R, case.D
    ldx = ldy = ldd = D + pad
    tails = [p if (p > 1 and i < case.n_delta) else 0 for i, p in enumerate(case.tail_parts)]
    args = [plane(npy(o.x), ldx, NANF), ldx, H.filled(((R - 1) * ldy + D,), np.int16 if case.out_bf16 else np.float32), ldy, R, D,
            npy(o.w) if case.has_w else None, npy(o.b) if case.has_b else None, case.add_one, case.eps]
    dl, tl = [], []
    for i in range(2):
        if i < case.n_delta:
            d = o.d[i].clone()
            if tails[i]:
                d[case.tail_row0:] = float("nan")           # the GEMM leaves these rows unwritten: the kernel must not read them
            dn = npy(d)
            dl.append(plane(dn, ldd, dn.dtype.type(0x7FC0) if case.delta_bf16 else NANF))
            tr = R - case.tail_row0
            tl.append(plane(npy(o.t[i][:tails[i]].reshape(tails[i] * tr, D)), ldd, NANF) if tails[i] and tr > 0 else None)
        else:
            dl.append(None)
            tl.append(None)
    tail_row0 = case.tail_row0 if any(tails) else R
    args += [dl[0], ldd, dl[1], case.keep_x, tail_row0, tails[0], tl[0], tails[1], tl[1]]
    k = bt.add(f"ln_mod<{'bf16' if case.out_bf16 else 'f32'},{'bf16' if case.delta_bf16 else 'f32'}>", (R + 3) // 4, 256, args)
    return k, o, args


def ln_check(case, pad, o, args, out):
    torch, gu, su = _mods()
    R, D, ld = case.R, case.D, case.D + pad
    r = case.refs(o)
    y = tor(rows_of(out[2], R, D, ld), case.out_dtype)
    x_after = tor(rows_of(out[0], R, D, ld))
    want_x = r.xs if (case.n_delta and not case.keep_x) else o.x
    err, where = gu.parity_err(y, r.ref, r.A, r.allow)

    def chk():
        assert H.still_filled(pad_of(out[2], R, D, ld)), "a padding column of y was written"
        assert same_bytes(pad_of(out[0], R, D, ld), pad_of(args[0], R, D, ld)), "a padding column of x was written"
        assert torch.equal(x_after, want_x), "the stream differs from the exact fp32 sums"
        assert err <= r.bound, f"err {err:.3e} > bound {r.bound:.3e} at {where}"
    return holds(chk), err / r.bound


# ---------------------------------------------------------------------------------------------------- GroupNorm
def gn_list(reduced):
    torch, gu, su = _mods()
    cs = gu.gn_cases()
    if reduced:
        cs = cover(cs, lambda c: [("path", c.vec, c.offset, c.T % 4), ("n", c.n < 64, c.n < 256), ("cpg", c.C // c.G == 1), ("affine", c.has_gamma, c.has_beta),
                                  ("act", c.act)])
    return cs


def gn_add(bt, case):
    o = case.ops()
    x = npy(o.x).reshape(-1)
    args = [H.Off(x, 4 * case.offset), H.Off(H.filled(x.shape, np.float32), 4 * case.offset), npy(o.gamma) if case.has_gamma else None,
            npy(o.beta) if case.has_beta else None, case.C, case.T, case.G, case.eps, case.act]
    return bt.add("groupnorm", (case.G, case.B), 256, args), o


def gn_check(case, o, out):
    torch, gu, su = _mods()
    r = case.refs(o)
    err, where = gu.parity_err(tor(out[1]).view(o.x.shape), r.ref, r.A, r.allow)
    return holds(lambda: _assert(err <= r.bound, f"err {err:.3e} > bound {r.bound:.3e} at {where}")), err / r.bound


def _assert(cond, msg):
    assert cond, msg


# ---------------------------------------------------------------------------------------------------- the text stack
def te_list(reduced):
    torch, gu, su = _mods()
    cs = gu.te_cases()
    return cover(cs, lambda c: [("ld<N", c.ld_ids < c.N), ("len>ld", max(c.text_len) > c.ld_ids), ("B", c.B), ("Dt", c.Dt), ("far", c.far_ids)]) if reduced else cs


def te_add(bt, case):
    o = case.ops()
    total = 2 * case.B * case.N * case.Dt // 4
    args = [npy(o.ids), case.ld_ids, npy(o.text_len), npy(o.emb), npy(o.pos), H.filled((2 * case.B, case.N, case.Dt), np.float32), case.B, case.N, case.Dt,
            case.vocab_rows]
    return bt.add("text_embed", grid2(total), 256, args), o


def te_check(case, o, out):
    torch, gu, su = _mods()
    return same_bytes(out[5], npy(gu.te_ref(case, o))), 0.0


def dw_list(reduced):
    torch, gu, su = _mods()
    cs = gu.dw_cases()
    if reduced:
        cs = cover(cs, lambda c: [("KW", c.KW in (1, 7) and c.KW), ("C", c.C == 4), ("len0", c.lens is not None and 0 in c.lens),
                                  ("len1", c.lens is not None and 1 in c.lens), ("null", c.lens is None), ("N1", c.N == 1)])
    return cs


def dw_add(bt, case):
    o = case.ops()
    x = o.x.clone()
    for s, L in enumerate(o.lens):
        x[s, L:] = float("nan")                              # rows at and beyond len: the kernel must not read them
    total = case.n_seq * case.N * case.C // 4
    args = [npy(x), H.filled(tuple(o.x.shape), np.float32), npy(o.w), npy(o.bias), None if case.lens is None else np.array(case.lens, np.int32), case.B,
            case.n_seq, case.N, case.C, case.KW]
    return bt.add("dwconv", grid2(total), 256, args), o


def dw_check(case, o, out):
    torch, gu, su = _mods()
    r = case.refs(o)
    err, where = gu.parity_err(tor(out[1]), r.ref, r.A, r.allow)
    return holds(lambda: _assert(err <= r.bound, f"err {err:.3e} > bound {r.bound:.3e} at {where}")), err / r.bound


def grn_list(reduced):
    torch, gu, su = _mods()
    cs = gu.grn_cases()
    if reduced:
        cs = cover(cs, lambda c: [("C", c.bf16, c.C in (64, 128, 320) and c.C), ("N", c.N in (1, 4, 5, 17) and c.N),
                                  ("len", c.lens is None or tuple(sorted({0 if l == 0 else (1 if l < c.N else (2 if l == c.N else 3)) for l in c.lens})))])
    return cs


def grn_add(bt, case):
    """Two launches, as vvk_grn: the statistics, then the apply on their result."""
    o = case.ops()
    name = "bf16" if case.bf16 else "f32"
    lens = None if case.lens is None else np.array(case.lens, np.int32)
    k = bt.add(f"grn_stats<{name}>", (case.C // 64, case.n_seq), 256, [npy(o.x), H.filled((case.n_seq, case.C), np.float32), lens, case.B, case.N, case.C])
    return k, o


def grn_add_apply(bt, case, o, sumsq):
    name = "bf16" if case.bf16 else "f32"
    return bt.add(f"grn_apply<{name}>", ((case.N + 15) // 16, case.n_seq), 256, [npy(o.x), sumsq, npy(o.gamma), npy(o.beta), case.N, case.C, 16],
                  shmem=4 * case.C)


def grn_check(case, o, ss, y):
    torch, gu, su = _mods()
    r = case.refs(o)
    e1, w1 = gu.parity_err(tor(ss), r.ss, r.ss_A, None)
    e2, w2 = gu.parity_err(tor(y, case.dtype), r.ref, r.A, r.allow)

    def chk():
        assert e1 <= r.ss_bound, f"sumsq err {e1:.3e} > bound {r.ss_bound:.3e} at {w1}"
        assert e2 <= r.bound, f"err {e2:.3e} > bound {r.bound:.3e} at {w2}"
        for s, L in enumerate(o.lens):
            assert L != 0 or bool((tor(ss)[s] == 0.0).all())
    return holds(chk), max(e1 / r.ss_bound, e2 / r.bound)


# ---------------------------------------------------------------------------------------------------- build_cat
def bc_list(reduced):
    """(masked, n_mel, Dt, N, F_max, ref_len): F_max < N; ref_len of 0, F_max and F_max + 3; ld_keep = N + 3."""
    return [(m, n_mel, Dt, 9, 6, (0, 6, 9)) for m in (False, True) for n_mel, Dt in ((4, 4), (100, 8))]


def bc_add(bt, c):
    masked, M, Dt, N, F_max, ref_len = c
    B, rng = len(ref_len), np.random.default_rng(77 + M + masked)
    mel = rng.standard_normal((B, F_max, M)).astype(np.float32)
    text = rng.standard_normal((2 * B, N, Dt)).astype(np.float32)
    keep = rng.choice(np.array([0, 1, 255], np.uint8), (B, N + 3))
    keep[:, 0], keep[:, N:] = 1, 1
    keep = keep.reshape(-1)[:(B - 1) * (N + 3) + N].copy()                                    # the last row ends the block
    cd = M + Dt
    args = [mel, F_max, np.array(ref_len, np.int32), text, H.filled((B, N, cd), np.float32), H.filled((B, N, cd), np.float32), B, N, M, Dt,
            keep if masked else None, N + 3 if masked else 0]
    return bt.add(f"build_cat<{'masked' if masked else 'plain'}>", grid2(B * N * cd // 4), 256, args), (mel, text, keep)


def bc_check(c, ops, out):
    masked, M, Dt, N, F_max, ref_len = c
    mel, text, keep = ops
    B = len(ref_len)
    cat, drop = np.zeros((B, N, M + Dt), np.float32), np.zeros((B, N, M + Dt), np.float32)
    for b in range(B):
        for t in range(N):
            if t < ref_len[b] and t < F_max and (not masked or keep[b * (N + 3) + t]):
                cat[b, t, :M] = mel[b, t]
        cat[b, :, M:], drop[b, :, M:] = text[b], text[B + b]
    return same_bytes(out[4], cat) and same_bytes(out[5], drop), 0.0


# ---------------------------------------------------------------------------------------------------- ode_stage / cfg_euler
def stage_list(reduced):
    torch, gu, su = _mods()
    cs = [c for c in su.stage_cases() if c.Rc <= 86 and c.n_mel in (4, 100)]
    if reduced:
        cs = cover(cs, lambda c: [(c.inst, "M", c.n_mel, c.ldp - c.n_mel in (0, 4) and c.ldp - c.n_mel), (c.inst, "Rc", c.Rc), (c.inst, "rows", c.rows),
                                  (c.inst, "last", c.last), (c.inst, "u", c.u_map), (c.inst, "xe", c.stage > 0), (c.inst, "item", c.per_item)])
    return cs


def pred_plane(o, M, ldp):
    p = npy(o.pred[:, :M])
    return plane(p, ldp, NANF), p.shape[0]


def stage_add(bt, case, ring=False):
    """ring: k_out is the block of k_prev[0] (the ring slot of the oldest slope under a multistep plan); the thread build must stay silent,
    each element being read and written by one thread, and the result is the mirror's."""
    torch, gu, su = _mods()
    o = case.ops()
    Rc, M = case.Rc, case.n_mel
    pred, _ = pred_plane(o, M, case.ldp)
    rs = npy(o.row_src) if o.row_src is not None else None
    total = Rc * M // 4
    if case.euler:
        args = [npy(o.x), pred, case.ldp, Rc, M, case.g, case.h, rs if case.inst == "euler_rows" else None]
        return bt.add("cfg_euler", grid2(total), 256, args), o
    coef = [float(c) for c in case.coef]
    kp = [npy(o.k_prev[j]) if j < case.stage and coef[j] != 0 else None for j in range(3)]
    cc = [coef[j] if kp[j] is not None else 0.0 for j in range(3)]
    apg_coef = x_e = None
    xe_packed, omt = 0, 0.0
    if case.apg:
        apg_coef, xe_packed = npy(o.apg_coef).reshape(-1), int(o.xe_packed)
        x_e = H.Alias(0) if o.x_e is None else npy(o.x_e)
        omt = float(np.float32(1.0) - np.float32(o.t_e))
    args = [npy(o.x), pred, case.ldp, Rc, M, case.g, None if o.g_item is None else npy(o.g_item), case.N, rs, kp[0], kp[1], kp[2], cc[0], cc[1], cc[2],
            coef[case.stage], H.Alias(9) if ring else H.filled((Rc, M), np.float32), None if case.last else H.filled((Rc, M), np.float32),
            None if o.u_row is None else npy(o.u_row), apg_coef, x_e, xe_packed, omt]
    return bt.add(f"ode_stage<{case.inst}>", grid2(total), 256, args), o


def stage_check(case, o, out, ring=False):
    torch, gu, su = _mods()
    ref, b = su.stage_eval(case, o), su.stage_bounds(case)
    x = tor(out[0])
    got_x = x[o.xr] if (case.euler or case.last) else tor(out[17])
    e1, w1 = gu.parity_err(got_x, ref["acc"], ref["mag"])
    worst = e1 / b["acc"]

    def chk():
        nonlocal worst
        assert e1 <= b["acc"], f"state err {e1:.3e} > bound {b['acc']:.3e} at {w1}"
        if not case.euler:
            k = tor(out[9 if ring else 16])
            e2, w2 = gu.parity_err(k, ref["k"], ref["K"])
            worst = max(worst, e2 / b["k"])
            assert e2 <= b["k"], f"slope err {e2:.3e} > bound {b['k']:.3e} at {w2}"
            has_u = torch.ones(case.Rc, dtype=torch.bool) if o.u_row is None else o.u_row >= 0
            pc = o.pred[:case.Rc, :case.n_mel]
            assert torch.equal(k[~has_u], pc[~has_u]), "a row without an unconditional prediction: k == pc exactly"
        if case.euler or case.last:
            mask = torch.ones(o.x.shape[0], dtype=torch.bool)
            mask[o.xr] = False
            assert su.same_bits(x[mask], o.x[mask]), "a row of x outside row_src was written"
        else:
            assert su.same_bits(x, o.x), "x was written before the last stage"
    return holds(chk), worst


# ---------------------------------------------------------------------------------------------------- apg_reduce / apg_coef
def apg_list(reduced):
    torch, gu, su = _mods()
    cs = su.apg_cases()
    return [c for c in cs if "lens_0_31" in c.name or "unguided" in c.name or "packed" in c.name] if reduced else cs


def apg_add(bt, case):
    torch, gu, su = _mods()
    o = case.ops()
    B, nt, M = case.B, case.n_tiles, case.n_mel
    pred, _ = pred_plane(o, M, case.ldp)
    omt = 1.0 - float(np.float32(case.t_e))                            # vvk_apg_coef: `1.0 - (double)a->t_e`
    o.host = dict(pred=pred, u_row=None if o.u_row is None else npy(o.u_row), row_start=npy(o.row_start), len=np.array(case.lens_dev, np.int32), omt=omt)
    h = o.host
    args = [pred, case.ldp, case.Rc, M, h["u_row"], npy(o.x_e), npy(o.row_src) if case.rows else None, h["row_start"], h["len"], nt, omt,
            H.filled((B, nt, 3), np.float64)]
    return bt.add("apg_reduce", (nt, B), 256, args), o


def apg_add_coef(bt, case, o, part):
    h = o.host
    args = [part, case.n_tiles, case.Rc, case.n_mel, h["u_row"], h["row_start"], h["len"], h["omt"], 9.0, npy(o.g_item), npy(o.eta), npy(o.norm),
            H.filled((case.B, 2), np.float32)]
    return bt.add("apg_coef", case.B, 64, args)


def apg_check(case, o, part, coef):
    torch, gu, su = _mods()
    ref = su.apg_ref(case, o)
    written = torch.isfinite(ref["part"])
    got = tor(part)
    e = ((got - ref["part"]).abs() / ref["scale"])[written]
    lim = (ref["chain"][:, :, None] * su.EPS53).expand_as(ref["part"])[written]
    cb = gu.EPS24 * ref["coef"].abs() + ref["slack"]
    ce = (tor(coef).double() - ref["coef"]).abs()

    def chk():
        assert H.still_filled(part[~written.numpy()]), "a tile past the item's length was written"
        assert bool((e <= lim).all()), "a partial misses its chain bound"
        assert bool((ce <= cb).all()), (coef.tolist(), ref["coef"].tolist())
        for b in range(case.B):
            if case.lens[b] == 0 or (case.guided is not None and not case.guided[b]):
                assert coef[b].tolist() == [0.0, 0.0]
    return holds(chk), float((e / lim).max()) if e.numel() else 0.0


# ---------------------------------------------------------------------------------------------------- pack
def pack_list(reduced):
    torch, gu, su = _mods()
    cs = [c for c in su.pack_cases() if "wrap" not in c.name]          # 2 workgroups take the further trips instead
    return [(c, only_x, dt) for c in cs for only_x in (False, True) for dt in (torch.float32, torch.bfloat16)
            if not reduced or (only_x, dt) in ((False, torch.bfloat16), (True, torch.float32))]


def pack_add(bt, case, only_x, dtype):
    torch, gu, su = _mods()
    o = case.ops()
    M, CD, ldo, Rc = case.n_mel, case.cond_dim, case.ldo, case.Rc
    total = Rc + o.Ru if case.guided else 2 * Rc
    x = npy(o.xs if case.x_packed else o.xp)
    out = H.filled((total, ldo), np.int16 if dtype == torch.bfloat16 else np.float32)
    tag = "bf16" if dtype == torch.bfloat16 else "f32"
    cols4 = (M if only_x else ldo) // 4
    if case.guided:
        row0, n = case.window or (0, total)
        args = [x, npy(o.cat), npy(o.cat_drop), out, ldo, Rc, row0, n, M, CD, int(only_x), int(case.x_packed), npy(o.row_src), npy(o.u_src), npy(o.u_crow)]
        return bt.add(f"pack_cat_guided<{tag}>", grid2(n * cols4), 256, args), o
    rs = npy(o.row_src) if (case.rows and not case.x_packed) else None
    return bt.add(f"pack_cat<{tag}>", grid2(2 * Rc * cols4), 256, [x, npy(o.cat), npy(o.cat_drop), out, ldo, Rc, M, CD, int(only_x), rs]), o


def pack_check(case, only_x, dtype, o, out):
    torch, gu, su = _mods()
    want = su.pack_ref(case, o, only_x, dtype)[0]                      # 7.0 where the launch writes nothing
    untouched = (want.float() == su.FILL).numpy()
    got = out[3]
    return bool(H.still_filled(got[untouched]) and same_bytes(got[~untouched], npy(want)[~untouched])), 0.0


# ---------------------------------------------------------------------------------------------------- tables, lengths, rope
def table_list(reduced):
    torch, gu, su = _mods()
    plain, guided = su.table_cases()
    if reduced:
        keep = lambda c: any(t in c.name for t in ("B1", "B3", "B33", "device_more", "device_fewer"))
        plain, guided = [c for c in plain if keep(c)], [c for c in guided if keep(c) and ("_alt" in c.name or "B" in c.name.split("/")[1][:1])]
    return plain + guided


def flag_words(flags):
    w = np.zeros(32, np.uint32)
    for b, f in enumerate(flags):
        if f:
            w[b >> 5] |= np.uint32(1 << (b & 31))
    return w


def table_add(bt, case):
    B, N, Rc = len(case.seq_len), case.N, case.Rc
    i32 = lambda n: H.filled((n,), np.int32)
    sl = np.array(case.seq_len, np.int32)
    if case.flags is None:
        names = ("row_start", "row_src", "row_pos", "kv_len")
        return bt.add("row_tables", B, 256, [sl, B, N, Rc, i32(2 * B), i32(Rc), i32(2 * Rc), i32(2 * B)]), dict(zip(names, range(4, 8)))
    Ru = case.Ru
    names = ("row_start", "rs_rel", "kv_len", "row_pos", "u_src", "u_crow", "u_row")
    args = [sl, flag_words(case.flags), B, N, Rc, Ru, i32(2 * B), i32(B), i32(2 * B), i32(Rc + Ru), i32(Ru), i32(Ru), i32(Rc)]
    return bt.add("guided_tables", B, 256, args), dict(zip(names, range(6, 13)))


def table_check(case, where, out):
    torch, gu, su = _mods()
    want = su.tables_restated(case) if case.flags is None else su.guided_restated(case)
    fill = int(H.filled((1,), np.int32)[0])
    good = True
    for k, v in want.items():
        w = np.array([fill if e == su.SENTINEL else e for e in v], np.int32)
        good &= bool(np.array_equal(out[where[k]], w))
    return good, 0.0


def len_list(reduced):
    torch, gu, su = _mods()
    return [c for c in su.len_cases() if not reduced or c.B in (1, 64, 65)]


def len_add(bt, case):
    o = case.ops()
    B = case.B
    k1 = bt.add("ref_len", (B + 63) // 64, 64, [npy(o.audio_len), H.filled((B,), np.int32), B, case.hop])
    k2 = bt.add("decode_len", (B + 63) // 64, 64, [npy(o.seq_len), npy(o.ref_len), H.filled((len(case.mult) * B,), np.int32), B, len(case.mult),
                                                   np.array(case.mult, np.int32), case.N, case.T_max])
    return (k1, k2), o


def rope_list(reduced):
    torch, gu, su = _mods()
    return [(1, 1), (7, 9)] if reduced else [(n, r) for n in su.ROPE_SIZES for r in su.ROPE_SIZES]


def rope_add(bt, n, rows):
    torch, gu, su = _mods()
    g = su._gen(6000 + n + rows)
    cos, sin = torch.randn(n, 64, generator=g), torch.randn(n, 64, generator=g)
    want = torch.empty(n, 64)
    want[:, 0::2], want[:, 1::2] = cos[:, 0::2], sin[:, 0::2]
    pos = su.rope_positions(n, rows)
    k1 = bt.add("rope_compact", (n * 32 + 255) // 256, 256, [npy(cos), npy(sin), H.filled((n, 64), np.float32), n])
    k2 = bt.add("rope_rows", (rows * 16 + 255) // 256, 256, [npy(want), np.array(pos, np.int32), H.filled((rows, 64), np.float32), rows])
    return (k1, k2), (npy(want), npy(want[torch.tensor(pos)]))



# ---------------------------------------------------------------------------------------------------- the reuse form, the ring alias
def reuse_list(reduced):
    if H.ROOT not in sys.path:
        sys.path.insert(0, H.ROOT)
    from tests import cfg_reuse_util as ru
    return ru.reuse_stage_cases()


def reuse_add(bt, case):
    o = case.ops()
    Rc, M, i = o.Rc, case.n_mel, case.stage
    coef = [float(c) for c in o.coef]
    kp = [npy(o.k_prev[j]) if j < i and coef[j] != 0 else None for j in range(3)]
    cc = [coef[j] if kp[j] is not None else 0.0 for j in range(3)]
    L = flag_words([m & 1 for m in o.modes])
    S = flag_words([m & 2 for m in o.modes])
    args = [npy(o.x), plane(npy(o.pred[:, :M]), case.ldp, NANF), case.ldp, Rc, M, case.g, None, case.N, npy(o.row_src), kp[0], kp[1], kp[2], cc[0], cc[1], cc[2],
            coef[i], H.filled((Rc, M), np.float32), None if o.last else H.filled((Rc, M), np.float32), npy(o.u_row), None, None, 0, 0.0,
            npy(o.d_old), L, S]                                          # d_buf: exactly Rc x n_mel
    return bt.add("ode_stage<reuse>", grid2(Rc * M // 4), 256, args), o


def reuse_check(case, o, out):
    torch, gu, su = _mods()
    r = case.ref(o)
    eps = gu.EPS24
    rs = o.row_src.long()
    x = tor(out[0])
    got = (x[rs] if o.last else tor(out[17])).double()
    k = tor(out[16])
    e_acc = float(((got - r["acc"]).abs() / (8 * eps * r["mag"])).max())
    e_k = float(((k.double() - r["k"]).abs() / (4 * eps * r["K"]).clamp_min(1e-300)).max())

    def chk():
        assert e_acc <= 1.0, f"state: {e_acc:.3f} x its bound"
        assert e_k <= 1.0, f"slope: {e_k:.3f} x its bound"
        assert torch.equal(k[~r["guided"]], r["pc32"][~r["guided"]]), "an unguided row's slope is pc"
        assert torch.equal(tor(out[23]), r["want_d"]), "d_buf: the stored rows are pc - pu in fp32, every other row untouched"
        mask = torch.ones(o.x.shape[0], dtype=torch.bool)
        mask[rs] = False
        assert torch.equal(x[mask], o.x[mask]) and (o.last or torch.equal(x, o.x)), "x was written outside its rows"
    return holds(chk), max(e_acc, e_k)


def ring_list(reduced):
    """The multistep form (N20): k_out IS the buffer of the oldest earlier slope.  Stage cases with an earlier slope that is read."""
    torch, gu, su = _mods()
    cs = [c for c in stage_list(False) if not c.euler and not c.apg and c.stage >= 1 and float(c.coef[0]) != 0.0]
    return cover(cs, lambda c: [(c.inst, c.n_mel), (c.inst, c.Rc), (c.inst, c.stage)]) if reduced else cs


# ---------------------------------------------------------------------------------------------------- ode_diff / cfg_drift
def _edge_tables(lens, overstate=7):
    """row_start / len of the items back to back, the last one's device len overstating the Rc rows, and one more item whose device
    row_start lies past Rc: the kernels clamp both and that item has no rows."""
    starts = [sum(lens[:b]) for b in range(len(lens))]
    Rc = sum(lens)
    return np.array(starts + [Rc + 5], np.int32), np.array(list(lens[:-1]) + [lens[-1] + overstate, 10], np.int32), Rc


def diff_add(bt, M, with_prev):
    from tests import multistep_util as mu
    f, p = mu.edge_slopes(M)
    rs, ln, Rc = _edge_tables(mu.EDGE_LENS)
    B, nt = len(rs), mu.EDGE_TILES
    args = [f, p if with_prev else None, Rc, M, rs, ln, nt, H.filled((B, nt, 2), np.float64)]
    want = [mu.report_mirror(f[rs[b]: rs[b] + n], p[rs[b]: rs[b] + n] if with_prev else None) for b, n in enumerate(mu.EDGE_LENS)] + [(0.0, 0.0)]
    return bt.add("ode_diff_reduce", (nt, B), 256, args), dict(rs=rs, ln=ln, Rc=Rc, nt=nt, B=B, want=np.array(want), lens=mu.EDGE_LENS, part=7)


def drift_add(bt, M):
    from tests import cfg_reuse_util as ru
    pc, pu, d_old = ru.edge_predictions(M)
    lens = ru.EDGE_LENS
    rs, ln, Rc = _edge_tables(lens)
    B, nt, ldp = len(rs), ru.EDGE_TILES, M + 4
    Ru = sum(n for n, c in zip(lens, ru.EDGE_COMPUTED) if c)
    pred = np.full((Rc + Ru, M), NANF, np.float32)
    pred[:Rc] = pc
    u_row = np.full(Rc, -1, np.int32)
    dbuf = np.full((Rc, M), NANF, np.float32)
    want, upos = [], Rc
    for b, n in enumerate(lens):
        rows = slice(rs[b], rs[b] + n)
        if ru.EDGE_HAS_OLD[b]:
            dbuf[rows] = d_old[rows]
        if ru.EDGE_COMPUTED[b]:
            pred[upos: upos + n] = pu[rows]
            u_row[rows] = upos + np.arange(n)
            upos += n
            want.append(ru.drift_mirror(pc[rows], pu[rows], d_old[rows] if ru.EDGE_HAS_OLD[b] else None))
        else:
            want.append((0.0, 0.0))
    want.append((0.0, 0.0))
    args = [plane(pred, ldp, NANF), ldp, Rc, M, u_row, dbuf, flag_words(list(ru.EDGE_HAS_OLD) + [1]), rs, ln, nt, H.filled((B, nt, 2), np.float64)]
    return bt.add("cfg_drift_reduce", (nt, B), 256, args), dict(rs=rs, ln=ln, Rc=Rc, nt=nt, B=B, want=np.array(want), lens=lens, part=10)


def finish_add(bt, m, part):
    return bt.add("ode_diff_finish", m["B"], 64, [part, m["nt"], m["Rc"], m["rs"], m["ln"], H.filled((m["B"], 2), np.float64)])


def finish_check(m, part, report):
    TILE = 32
    owned = np.zeros(part.shape[:2], bool)
    for b, n in enumerate(m["lens"]):
        owned[b, :-(-n // TILE)] = True
    return bool(H.still_filled(part[~owned]) and same_bytes(report, m["want"])), 0.0



# ---------------------------------------------------------------------------------------------------- block caching (N23)
def span_list(reduced):
    """Every form of the span kernel: MARK / DIFF / APPLY, nothing pending / fp32 / bf16 deltas, D 128 and 1024, 1 / 3 / 86 rows.  Reduced:
    every mode with every dtype at the largest shape (two workgroups, 43 trips of the loop) and once at the smallest."""
    from tests import block_cache_util as bu
    full = [(m, p, D, R) for m in (bu.MARK, bu.DIFF, bu.APPLY) for p in bu.SPAN_PENDING for D in bu.SPAN_DIMS for R in bu.SPAN_ROWS]
    return [c for c in full if (c[2], c[3]) == (1024, 86) or (c[1] == "f32" and (c[2], c[3]) == (128, 1))] if reduced else full


def span_add(bt, case):
    from tests import block_cache_util as bu
    mode, pending, D, R = case
    G = bu.GUARD
    x, d1, d2, buf = (a[G: G + R].copy() for a in bu.span_operands(R, D))
    if pending == "none":
        d1 = d2 = a1 = a2 = None
    elif pending == "bf16":
        d1, d2 = bu.bf16_round(d1), bu.bf16_round(d2)
        a1, a2 = ((d.view(np.uint32) >> 16).astype(np.uint16) for d in (d1, d2))
    else:
        a1, a2 = d1, d2
    name = f"block_span<{'bf16' if pending == 'bf16' else 'f32'},{('mark', 'diff', 'apply')[mode]}>"
    n4 = R * D // 4
    k = bt.add(name, grid2(n4), 256, [x, a1, a2, buf, n4])
    return k, bu.span_expected(mode, x, d1, d2, buf), (a1, a2)


def span_check(want, deltas, out):
    ok = same_bytes(out[0], want[0]) and same_bytes(out[3], want[1])
    ok = ok and all(a is None or same_bytes(out[i + 1], a) for i, a in enumerate(deltas))
    return bool(ok), 0.0


def bdrift_add(bt, D, with_prev, branch0):
    """The report's reduction on block_cache_util's edge sequences (0, 31, 32, 33 and 45 rows, the last one's device length overstated,
    one more sequence whose device row_start lies past the rows)."""
    from tests import block_cache_util as bu
    d_new, d_prev = bu.edge_planes(D)
    rs, ln, R = _edge_tables(bu.EDGE_LENS)
    S, nt = len(rs), bu.EDGE_TILES
    args = [d_new, d_prev if with_prev else None, R, D, rs, ln, nt, H.filled((S, nt, 2), np.float64)]
    want = [bu.report_mirror(d_new[rs[s]: rs[s] + n], d_prev[rs[s]: rs[s] + n] if with_prev else None) for s, n in enumerate(bu.EDGE_LENS)] + [(0.0, 0.0)]
    return bt.add("block_drift_reduce", (nt, S), 256, args), dict(rs=rs, ln=ln, R=R, nt=nt, S=S, want=np.array(want), lens=bu.EDGE_LENS, branch0=branch0)


def bfinish_add(bt, m, part, zero=False):
    """The finishing kernel on one branch of S items; zero: over no tiles, the partials a null pointer."""
    return bt.add("block_drift_finish", m["S"], 64, [None if zero else part, 0 if zero else m["nt"], m["R"], m["rs"], m["ln"], m["S"], m["branch0"],
                                                     H.filled((m["S"], 2, 2), np.float64)])


def bfinish_check(m, part, report, zero=False):
    owned = np.zeros(part.shape[:2], bool)
    for s, n in enumerate(m["lens"]):
        owned[s, :-(-n // 32)] = True
    c = m["branch0"]
    want = np.zeros_like(m["want"]) if zero else m["want"]
    return bool(H.still_filled(part[~owned]) and same_bytes(report[:, c], want) and H.still_filled(report[:, 1 - c]))


def block_cache_cases(exe, work, reduced=False):
    """The cases of the two N23 kernels alone (tests/test_block_cache_cpu.py runs these; cases() runs them among the others)."""
    bt, spans, sums = H.Batch(exe, work, NAME), [], []
    for case in span_list(reduced):
        k, want, deltas = span_add(bt, case)
        spans.append((k, want, deltas, f"block_span mode {case[0]} pending {case[1]} D {case[2]} R {case[3]}"))
    for D in (128, 1024):
        for with_prev, branch0 in ((True, 0), (False, 1)):
            k, m = bdrift_add(bt, D, with_prev, branch0)
            sums.append((k, m, f"block_drift D {D} d_prev {'given' if with_prev else 'null'} branch {branch0}"))
    outs = bt.run()
    for k, want, deltas, label in spans:
        yield H.check(label, span_check(want, deltas, outs[k])[0])
    second = []
    for k, m, label in sums:
        part = outs[k][7].copy()
        second.append((bfinish_add(bt, m, part), m, part, label, False))
    second.append((bfinish_add(bt, sums[0][1], None, zero=True), sums[0][1], outs[sums[0][0]][7].copy(), "block_drift over no tiles", True))
    outs2 = bt.run()
    for k, m, part, label, zero in second:
        yield H.check(label, bfinish_check(m, part, outs2[k][7], zero))


# ---------------------------------------------------------------------------------------------------- CFG-Zero* / rescale (N24)
def cfg_norm_cases(exe, work, reduced=False):
    """The three N24 kernels: cfg_gram_reduce on cfg_norm_util's items of 1, 31, 32, 33, 97 and 0 rows (permuted places, one item
    unguided, a tile of partials nobody owns, pad columns that end the block behind the last row), bit for bit against gram_mirror;
    cfg_norm_coef on those partials under coef_exact's bound; ode_stage<norm> on the stage cases of the device test under its counted bound.
    Reduced: one width of each and the stage cases that bring a new shape, row count, map or stage form."""
    torch, gu, su = _mods()
    from tests import cfg_norm_util as nu
    bt, grams, stages = H.Batch(exe, work, NAME), [], []
    nt = -(-max(nu.LENS) // nu.TILE) + 1
    B = len(nu.LENS)
    for M, ldp in (((100, 104),) if reduced else ((4, 4), (4, 8), (100, 100), (100, 104), (100, 128))):
        o = nu.coef_ops(M, ldp)
        pred = plane(npy(o["pred"][:, :M]), ldp, NANF)
        h = dict(pred=pred, u_row=npy(o["u_row"]), row_start=np.array(o["start"], np.int32), len=np.array(o["lens"], np.int32))
        k = bt.add("cfg_gram_reduce", (nt, B), 256, [pred, ldp, o["Rc"], M, h["u_row"], h["row_start"], h["len"], nt, H.filled((B, nt, 5), np.float64)])
        grams.append((k, o, h, f"cfg_gram M {M} ldp {ldp}"))
    cs = nu.stage_cases()
    if reduced:
        cs = cover([c for c in cs if c.n_mel in (4, 100)], lambda c: [("M", c.n_mel, c.ldp - c.n_mel in (0, 4) and c.ldp - c.n_mel), ("Rc", c.Rc), ("last", c.last),
                                                                    ("u", c.u_map), ("item", c.per_item), ("stage", c.stage)])
    for case in cs:
        o = case.ops()
        g = torch.Generator().manual_seed(case.seed)
        coef = torch.stack([0.7 + 0.3 * torch.rand(case.B, generator=g), 0.5 + 0.4 * torch.rand(case.B, generator=g)], dim=1).contiguous()
        Rc, M = case.Rc, case.n_mel
        cf = [float(c) for c in case.coef]
        kp = [npy(o.k_prev[j]) if j < case.stage and cf[j] != 0 else None for j in range(3)]
        cc = [cf[j] if kp[j] is not None else 0.0 for j in range(3)]
        args = [npy(o.x), pred_plane(o, M, case.ldp)[0], case.ldp, Rc, M, case.g, None if o.g_item is None else npy(o.g_item), case.N, npy(o.row_src),
                kp[0], kp[1], kp[2], cc[0], cc[1], cc[2], cf[case.stage], H.filled((Rc, M), np.float32), None if case.last else H.filled((Rc, M), np.float32),
                npy(o.u_row), npy(coef).reshape(-1), None, 0, 0.0]
        stages.append((bt.add("ode_stage<norm>", grid2(Rc * M // 4), 256, args), case, o, coef))
    outs = bt.run()
    second = []
    for k, o, h, label in grams:
        part = outs[k][8]
        pred2 = npy(o["pred"])
        M = o["n_mel"]
        ok = True
        for b, n in enumerate(nu.LENS):
            own = -(-n // nu.TILE)
            rows = np.arange(o["start"][b], o["start"][b] + n)
            ok = ok and H.still_filled(part[b, own:])
            if n and nu.GUIDED[b]:
                want, _ = nu.gram_mirror(pred2[rows, :M], pred2[h["u_row"][rows], :M])
                ok = ok and same_bytes(part[b, :own], want)
            elif n:
                ok = ok and not part[b, :own].any()
        yield H.check(label + " (partials equal the mirror)", bool(ok))
        args = [part.copy(), nt, o["Rc"], M, h["u_row"], h["row_start"], h["len"], 9.0, np.array(nu.G_ITEM, np.float32), np.array(nu.STAR, np.float32),
                np.array(nu.RESC, np.float32), H.filled((B, 2), np.float32), H.filled((B, 2), np.float32)]
        second.append((bt.add("cfg_norm_coef", B, 64, args), o, h, label))
    for k, case, o, coef in stages:
        ref = nu.stage_ref(case, o, coef)
        out = outs[k]
        x = tor(out[0])
        state = x[o.xr] if case.last else tor(out[17])
        ek = gu.parity_err(tor(out[16]), ref["k"], ref["K"].clamp_min(1e-300))[0]
        ea = gu.parity_err(state, ref["acc"], ref["mag"].clamp_min(1e-300))[0]
        good = ek <= nu.NORM_SLOPE_C * gu.EPS24 and ea <= su.STATE_C * gu.EPS24
        if not case.last:
            good = good and su.same_bits(x, o.x)
        yield H.check(f"{case.name} (slope err / bound {ek / (nu.NORM_SLOPE_C * gu.EPS24):.3f})", bool(good))
    outs2 = bt.run()
    for k, o, h, label in second:
        coef, rep_ = outs2[k][11], outs2[k][12]
        pred2 = npy(o["pred"])
        M = o["n_mel"]
        ok = same_bytes(coef, rep_)
        for b, n in enumerate(nu.LENS):
            rows = np.arange(o["start"][b], o["start"][b] + n)
            if not n or not nu.GUIDED[b]:
                ok = ok and coef[b].tolist() == [1.0, 1.0]
                continue
            s, f, bs, bf = nu.coef_exact(pred2[rows, :M], pred2[h["u_row"][rows], :M], nu.G_ITEM[b], nu.STAR[b] != 0, nu.RESC[b])
            ok = ok and abs(float(coef[b, 0]) - float(s)) <= bs and abs(float(coef[b, 1]) - float(f)) <= bf
        yield H.check(label.replace("cfg_gram", "cfg_norm_coef") + " (inside the derived bound)", bool(ok))


# ---------------------------------------------------------------------------------------------------- the lists
def cases(exe, work, reduced=False):
    """Runs every case through exe; yields (label, equal to the mirror / inside the bound of the device test)."""
    bt, post = H.Batch(exe, work, NAME), []
    for case, pad in ln_list(reduced):
        k, o, args = ln_add(bt, case, pad)
        post.append((k, f"{case.name} ld D+{pad}", lambda out, c=case, p=pad, o=o, a=args: ln_check(c, p, o, a, out)))
    for case in gn_list(reduced):
        k, o = gn_add(bt, case)
        post.append((k, case.name, lambda out, c=case, o=o: gn_check(c, o, out)))
    for case in te_list(reduced):
        k, o = te_add(bt, case)
        post.append((k, case.name, lambda out, c=case, o=o: te_check(c, o, out)))
    for case in dw_list(reduced):
        k, o = dw_add(bt, case)
        post.append((k, case.name, lambda out, c=case, o=o: dw_check(c, o, out)))
    grn = []
    for case in grn_list(reduced):
        k, o = grn_add(bt, case)
        grn.append((k, case, o))
    for c in bc_list(reduced):
        k, ops = bc_add(bt, c)
        post.append((k, f"build_cat masked {c[0]} n_mel {c[1]}", lambda out, c=c, ops=ops: bc_check(c, ops, out)))
    for case in stage_list(reduced):
        k, o = stage_add(bt, case)
        post.append((k, case.name, lambda out, c=case, o=o: stage_check(c, o, out)))
    for case in ring_list(reduced):
        k, o = stage_add(bt, case, ring=True)
        post.append((k, case.name + " k_out = k_prev[0]", lambda out, c=case, o=o: stage_check(c, o, out, ring=True)))
    for case in reuse_list(reduced):
        k, o = reuse_add(bt, case)
        post.append((k, case.name, lambda out, c=case, o=o: reuse_check(c, o, out)))
    sums = []
    for M in (4, 100):
        for with_prev in (True, False):
            k, m = diff_add(bt, M, with_prev)
            sums.append((k, m, f"ode_diff n_mel {M} f_prev {'given' if with_prev else 'null'}"))
        k, m = drift_add(bt, M)
        sums.append((k, m, f"cfg_drift n_mel {M}"))
    apg = []
    for case in apg_list(reduced):
        k, o = apg_add(bt, case)
        apg.append((k, case, o))
    for case, only_x, dt in pack_list(reduced):
        k, o = pack_add(bt, case, only_x, dt)
        post.append((k, f"{case.name} only_x {int(only_x)} {dt}", lambda out, c=case, ox=only_x, dt=dt, o=o: pack_check(c, ox, dt, o, out)))
    for case in table_list(reduced):
        k, where = table_add(bt, case)
        post.append((k, case.name, lambda out, c=case, w=where: table_check(c, w, out)))
    lens = [(len_add(bt, case), case) for case in len_list(reduced)]
    ropes = [(rope_add(bt, n, rows), n, rows) for n, rows in rope_list(reduced)]
    outs = bt.run()
    su = _mods()[2]
    for ((k1, k2), o), case in lens:
        want = su.len_ref(case, o)
        yield H.check(case.name, outs[k1][1].tolist() == want["ref_len"] and outs[k2][2].reshape(len(case.mult), case.B).tolist() == want["decode"])
    for ((k1, k2), (w1, w2)), n, rows in ropes:
        yield H.check(f"rope n {n} rows {rows}", same_bytes(outs[k1][2], w1) and same_bytes(outs[k2][2], w2))
    for k, label, fn in post:
        good, ratio = fn(outs[k])
        yield H.check(f"{label} (err / bound {ratio:.3f})", good)
    # the second pass: what runs on a first-pass result
    second = []
    for k, case, o in grn:
        ss = outs[k][1].copy()
        second.append((grn_add_apply(bt, case, o, ss), case, o, ss))
    third = []
    for k, case, o in apg:
        part = outs[k][11].copy()
        third.append((apg_add_coef(bt, case, o, part), case, o, part))
    fourth = []
    for k, m, label in sums:
        part = outs[k][m["part"]].copy()
        fourth.append((finish_add(bt, m, part), m, part, label))
    outs2 = bt.run()
    for k, case, o, ss in second:
        good, ratio = grn_check(case, o, ss, outs2[k][0])
        yield H.check(f"{case.name} (err / bound {ratio:.3f})", good)
    for k, case, o, part in third:
        good, ratio = apg_check(case, o, part, outs2[k][12])
        yield H.check(f"{case.name} (partials err / bound {ratio:.3f})", good)
    for k, m, part, label in fourth:
        yield H.check(label, finish_check(m, part, outs2[k][5])[0])
    yield from block_cache_cases(exe, work, reduced)
    yield from cfg_norm_cases(exe, work, reduced)


if __name__ == "__main__":
    H.main(NAME, cases, __doc__)
