"""-m gpu: N11, adaptive projected guidance: per-item eta and norm limit on the guidance difference.

The two reduction kernels (vv_apg_coef) and the projected stage kernel (vv_ode_stage_apg) against float64 numpy with DERIVED bounds; the
reduction bit for bit independent of the item's place; the solver entry against a float64 reference solver written here around
``Oracle.dit_forward`` with the rule of the issue; "off" and the structure properties bit for bit; the error paths; the engine level.
PARITY UNPINNED against the paper's code (not available offline): the arithmetic of DESIGN N11 is the specification.  No test claims a
quality gain: the synthetic weights cannot show one."""
import ctypes as C
import math

import numpy as np
import pytest
import torch

from tests.test_e2e_gpu import make_batch

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
LONG = "Hôm nay trời đẹp quá, chúng ta cùng nhau đi dạo quanh hồ nhé. " * 4
RAGGED = dict(a=[256 * 20, 256 * 12 + 100, 256 * 30], t=[30, 11, 47], g=[24, 9, 40])     # the ragged batch of test_ode_gpu.py
TOL = 1e-3            # max-abs state error in units of the reference's range: the project's figure for N7 and N8
TILE = 32             # VV_APG_TILE
EPS32, EPS64 = 2.0 ** -24, 2.0 ** -53
# solver level: per-item eta and RMS caps.  Item 0 has no cap (never capped), item 1's cap lies far below the RMS of its data-space
# difference at the first evaluations (capped there); both facts are asserted on the reference side.
ETAS = [0.0, 0.5, 1.0]
CAPS = [None, 0.05, 0.4]


def _mods():
    from vietvoice_tts_amd import runtime as rt
    from vietvoice_tts_amd.model_spec import ODE_METHODS, ode_plan
    return rt, ODE_METHODS, ode_plan


# ------------------------------------------------------------------------------------------------ float64 references
def coef_ref(pc, pu, xe, t_e, g, eta, r):
    """The rule of DESIGN N11 for one item in float64: pc, pu, xe [frames][n_mel] (fp32 values), t_e the fp32 evaluation time.
    Returns (A, C, capped, terms): terms = what the error bound is made of."""
    pc, pu, xe = (np.asarray(v, dtype=np.float64) for v in (pc, pu, xe))
    n = pc.size
    if n == 0:
        return 0.0, 0.0, False, None
    omt = 1.0 - float(np.float32(t_e))
    D = pc - pu
    d = xe + omt * pc
    S1, S2, S3 = float((D * d).sum()), float((d * d).sum()), float((D * D).sum())
    rms = omt * math.sqrt(S3 / n)
    capped = r is not None and r > 0 and rms > r
    s = r / rms if capped else 1.0
    A = g * s
    Cc = 0.0 if S2 == 0.0 else g * s * (eta - 1.0) * S1 / S2
    return A, Cc, capped, dict(n=n, S1=S1, S2=S2, S3=S3, T1=float(np.abs(D * d).sum()), s=s, g=g, eta=eta)


def coef_bound(A, Cc, tm):
    """DERIVED, not tuned.  A float64 sum of n terms in any order is within gamma * sum|terms| of the exact one, gamma = (n + 8) * 2^-52:
    n * 2^-53 for the device's order and as much for numpy's, the 8 for the roundings of the terms themselves on both sides (one in d, one in
    the product / fma).  S2 and S3 have positive terms (relative error gamma); S1 can cancel (absolute error gamma * T1, T1 = sum |D d|).
    s = r / ((1 - t) sqrt(S3 / n)) takes half of S3's relative error plus four float64 roundings (division, sqrt, product, division): rel_s <=
    gamma / 2 + 4 * 2^-53.  A = g s: rel_s + one float64 rounding, then ONE fp32 rounding (2^-24 |A|).  C = g s (eta - 1) S1 / S2: the absolute
    S1 term, S2's relative error, rel_s, four float64 roundings, then one fp32 rounding."""
    gamma = (tm["n"] + 8) * 2.0 ** -52
    rel_s = gamma / 2 + 4 * EPS64
    bA = abs(A) * (rel_s + EPS64) + EPS32 * abs(A)
    bC = 0.0
    if tm["S2"] != 0.0:
        bC = abs(tm["g"] * tm["s"] * (tm["eta"] - 1.0)) / tm["S2"] * gamma * tm["T1"] + abs(Cc) * (gamma + rel_s + 4 * EPS64) + EPS32 * abs(Cc)
    return bA, bC


def ref_solve_apg(orc, pre, x, method, nfe_step, g, eta, r, guided=None, apg=True):
    """N7's reference solver with the projected combine, one item, in the oracle's dtype (float64 here).  Returns (x, capped per
    evaluation).  apg False: the plain rule k = pc + (pc - pu) g.  guided[e] false: k = pc (N8)."""
    _, _, ode_plan = _mods()
    plan = ode_plan(nfe_step, orc.spec.sway_coef, method)
    ropes = (pre["rope_cos_q"], pre["rope_sin_q"], pre["rope_cos_k"], pre["rope_sin_k"])
    capped = []
    for n in range(plan.dt.numel()):
        h, k = float(plan.dt[n]), []
        for i in range(plan.s):
            e = n * plan.s + i
            xi = x
            for j in range(i):
                if plan.a[i][j] != 0.0:
                    xi = xi + (h * plan.a[i][j]) * k[j]
            t_e = float(plan.t[e])
            orc.t_grid = [t_e]
            pc = orc.dit_forward(xi, pre["cat_mel_text"], ropes, 0)
            if guided is not None and not guided[e]:
                k.append(pc)
                capped.append(False)
                continue
            pu = orc.dit_forward(xi, pre["cat_mel_text_drop"], ropes, 0)
            if not apg:
                k.append(pc + (pc - pu) * g)
                capped.append(False)
                continue
            D = pc - pu
            d = xi + (1.0 - t_e) * pc
            S1, S2, S3 = float((D * d).sum()), float((d * d).sum()), float((D * D).sum())
            rms = (1.0 - t_e) * math.sqrt(S3 / D.numel())
            cap = r is not None and rms > r
            s = r / rms if cap else 1.0
            capped.append(cap)
            Cc = 0.0 if S2 == 0.0 else g * s * (eta - 1.0) * S1 / S2
            k.append(pc + (g * s) * D + Cc * d)
        for j in range(plan.s):
            if plan.b[j] != 0.0:
                x = x + (h * plan.b[j]) * k[j]
    return x, capped


def _oracle_pre(orc, batch, b):
    la, lt, sl = int(batch["audio_len"][b]), int(batch["text_len"][b]), int(batch["seq_len"][b])
    return orc.preprocess(batch["audio"][b, :la], batch["ids"][b, :lt], sl, batch["noise"][b, :sl]), sl


# ------------------------------------------------------------------------------------------------ fixtures and small helpers
@pytest.fixture(scope="module")
def own(tiny_setup):
    """Engines of this module's own (hip_tiny is shared: its plan is never changed here) and a float64 Oracle whose t_grid is ours to set."""
    from oracle.vv_oracle import Oracle
    from vietvoice_tts_amd.runtime import HipSynth
    spec, w, _ = tiny_setup
    engs = {"f32": HipSynth(spec, w, acoustic_dtype="fp32", nfe_step=8), "bf16": HipSynth(spec, w, acoustic_dtype="bf16", nfe_step=8)}
    yield engs, Oracle(spec, w, nfe_step=8, dtype=torch.float64)
    for e in engs.values():
        e.close()


def _dev(batch):
    d = {k: (v.to(DEV) if torch.is_tensor(v) else v) for k, v in batch.items()}
    d["lens"] = [int(v) for v in batch["seq_len"]]
    return d


def _pre(eng, d):
    return eng.preprocess(d["audio"], d["audio_len"], d["ids"], d["text_len"], d["seq_len"], d["N"], seq_len_host=d["lens"])


def _host(d):
    return (C.c_int32 * len(d["lens"]))(*d["lens"])


def _apg(etas, caps):
    """The pair the entry takes: fp32 [B] on the device, a cap of 0 = none."""
    return (torch.tensor([float(v) for v in etas], dtype=torch.float32, device=DEV),
            torch.tensor([0.0 if v is None else float(v) for v in caps], dtype=torch.float32, device=DEV))


def _run(eng, d, pre, guide=None, cfg=None, step0=0, n=None, ws=None, x=None, apg=None):
    x = d["noise"].clone() if x is None else x
    eng.transformer_steps_ex(x, pre, step0, eng.n_steps - step0 if n is None else n, _host(d), cfg, ws=ws, guide=guide, apg=apg)
    return x


def _one(spec, d, batch, b):
    sl, la, lt = int(batch["seq_len"][b]), int(batch["audio_len"][b]), int(batch["text_len"][b])
    one = dict(audio=d["audio"][b: b + 1, :max(la, spec.n_fft)].contiguous(), audio_len=d["audio_len"][b: b + 1].contiguous(),
               ids=d["ids"][b: b + 1, :lt].contiguous(), text_len=d["text_len"][b: b + 1].contiguous(),
               seq_len=d["seq_len"][b: b + 1].contiguous(), N=sl, noise=d["noise"][b: b + 1, :sl].contiguous(), lens=[sl])
    return one, sl


def _err(x, ref):
    return float((x.double() - ref.double()).abs().max()) / float(ref.abs().max())


# ------------------------------------------------------------------------------------------------ 1. vv_apg_coef
KL_LENS = [1, 31, 32, 33, 97, 0]         # a lone frame, both sides of a tile edge, several tiles, an empty item -- one launch
KL_N, KL_M, KL_LDP = 128, 100, 128


def _layout(lens, N):
    """Packed rows of a padded [B][N] batch: row_src, row_start, Rc."""
    row_src = torch.cat([b * N + torch.arange(n) for b, n in enumerate(lens)]).to(torch.int32)
    starts = np.concatenate([[0], np.cumsum(lens)[:-1]]).astype(np.int32)
    return row_src, torch.from_numpy(starts), int(sum(lens))


def _coef(eng, pred, Rc, x_e, row_src, u_row, row_start, lens, N, t_e, g, g_item, eta, norm, M=KL_M, ldp=KL_LDP):
    """vv_apg_coef on host tensors; returns (rc, coef [B][2] on the host)."""
    rt = _mods()[0]
    B = len(lens)
    n_tiles = (N + TILE - 1) // TILE
    keep = [t.to(DEV) if t is not None else None for t in (pred, x_e, row_src, u_row, row_start, torch.tensor(lens, dtype=torch.int32),
                                                            g_item, eta, norm)]
    part = torch.full((B, n_tiles, 3), float("nan"), dtype=torch.float64, device=DEV)
    coef = torch.full((B, 2), 7.0, dtype=torch.float32, device=DEV)
    a = rt.vv_apg_coef_args()
    a.pred, a.ldp, a.Rc, a.n_mel = keep[0].data_ptr(), ldp, Rc, M
    a.x_e = keep[1].data_ptr()
    a.row_src = None if keep[2] is None else keep[2].data_ptr()
    a.u_row = None if keep[3] is None else keep[3].data_ptr()
    a.B, a.n_tiles, a.row_start, a.len = B, n_tiles, keep[4].data_ptr(), keep[5].data_ptr()
    a.t_e, a.g = t_e, g
    a.g_item, a.eta, a.norm_rms = (None if t is None else t.data_ptr() for t in keep[6:9])
    a.partials, a.coef = part.data_ptr(), coef.data_ptr()
    rc = eng.lib.vv_apg_coef(eng.ctx, C.byref(a), torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return rc, coef.cpu()


def _kl_inputs(seed, lens=KL_LENS, N=KL_N):
    gen = torch.Generator().manual_seed(seed)
    row_src, row_start, Rc = _layout(lens, N)
    x = torch.randn(len(lens) * N, KL_M, generator=gen)
    pred = torch.randn(2 * Rc, KL_LDP, generator=gen)
    return x, pred, row_src, row_start, Rc


COEF_CASES = ["inactive", "active", "edge", "s2_zero", "t_one", "unguided", "permuted"]


@pytest.mark.parametrize("case", COEF_CASES)
def test_apg_coef_against_float64(hip_tiny, case):
    """The bound is coef_bound's derivation; the observed maximum in units of it is printed (profiles/apg/notes.md records both)."""
    eng = hip_tiny["f32"]
    lens, N, B = KL_LENS, KL_N, len(KL_LENS)
    x, pred, row_src, row_start, Rc = _kl_inputs(11 + COEF_CASES.index(case))
    g_item = torch.tensor([2.0, 1.5, -0.5, 3.0, 2.5, 2.0])
    eta = torch.tensor([0.0, 0.5, 1.0, -0.3, 2.0, 0.25])
    norm = torch.full((B,), 1e3)                 # far above any RMS here: the cap is inactive
    t_e, u_row = 0.4, None
    rs = row_src.long()
    if case == "active":
        norm = torch.tensor([0.1, 0.2, 0.05, 0.3, 0.15, 0.1])      # the RMS of (1 - t) D is about 0.6 * sqrt(2)
    elif case in ("edge", "s2_zero"):
        t_e = 0.5
        pred[:Rc] = torch.round(pred[:Rc] * 1024) / 1024            # pc on a 2^-10 grid: pc -+ 2 and pc / 2 are exact
    if case == "edge":
        sign = torch.where(torch.rand(Rc, KL_LDP, generator=torch.Generator().manual_seed(5)) < 0.5, -2.0, 2.0)
        pred[Rc:] = pred[:Rc] - sign                                  # D = +-2 everywhere: S3 / n = 4 in any order, (1 - t) sqrt(4) = 1 exactly
        norm = torch.tensor([1.0, 1.0 - 2.0 ** -24, 1.0, 1.0 - 2.0 ** -24, 1.0, 1.0])
    elif case == "s2_zero":
        x[rs] = -0.5 * pred[:Rc, :KL_M]                              # d = x + (1 - t) pc = 0 exactly
    elif case == "t_one":
        t_e, norm = 1.0, torch.full((B,), 1e-6)                       # (1 - t) = 0: the data-space difference vanishes, nothing is capped
    elif case == "unguided":
        u_row = torch.full((Rc,), -1, dtype=torch.int32)
        u = 0
        for b in (0, 2, 4):                                           # items 1 and 3 have no unconditional rows; the others' are compacted
            u_row[int(row_start[b]): int(row_start[b]) + lens[b]] = Rc + u + torch.arange(lens[b], dtype=torch.int32)
            u += lens[b]
    elif case == "permuted":
        u_row = (Rc + torch.randperm(Rc, generator=torch.Generator().manual_seed(6))).to(torch.int32)
    rc, coef = _coef(eng, pred, Rc, x, row_src, u_row, row_start, lens, N, t_e, 2.0, g_item, eta, norm)
    assert rc == 0, eng.lib.vv_last_error(eng.ctx).decode()
    worst = 0.0
    for b in range(B):
        r0, n = int(row_start[b]), lens[b]
        rows = torch.arange(r0, r0 + n)
        if n == 0 or (u_row is not None and int(u_row[r0]) < 0):
            assert coef[b].tolist() == [0.0, 0.0], (case, b)
            continue
        pu_rows = rows + Rc if u_row is None else u_row[rows].long()
        A, Cc, capped, tm = coef_ref(pred[rows, :KL_M].numpy(), pred[pu_rows, :KL_M].numpy(), x[rs[rows]].numpy(), t_e, float(g_item[b]),
                                     float(eta[b]), float(norm[b]))
        bA, bC = coef_bound(A, Cc, tm)
        eA, eC = abs(float(coef[b, 0]) - A), abs(float(coef[b, 1]) - Cc)
        worst = max(worst, eA / bA if bA else 0.0, eC / bC if bC else 0.0)
        assert eA <= bA and eC <= bC, (case, b, eA, bA, eC, bC)
        if case == "inactive" or case == "t_one":
            assert not capped and float(coef[b, 0]) == float(g_item[b]), (case, b)
        if case == "active":
            assert capped and abs(float(coef[b, 0])) < abs(float(g_item[b])), (case, b)
        if case == "edge":                                            # exactly at the edge: s = 1; one fp32 ulp below it: capped
            at_edge = float(norm[b]) == 1.0
            assert capped == (not at_edge)
            assert (float(coef[b, 0]) == float(g_item[b])) == at_edge, (case, b, float(coef[b, 0]))
        if case == "s2_zero" or float(eta[b]) == 1.0:
            assert float(coef[b, 1]) == 0.0, (case, b)
    print(f"apg_coef {case}: max |error| / derived bound = {worst:.3e}")


def test_apg_coef_is_independent_of_the_items_place(hip_tiny):
    """torch.equal: each item alone (another N, its own row 0) and in a second batch (reversed order, N = 160, a neighbour between) gives
    the coefficients it has in the first batch; a mapped u_row that names the plain rows gives the plain layout's."""
    eng = hip_tiny["f32"]
    lens, N, B = KL_LENS, KL_N, len(KL_LENS)
    x, pred, row_src, row_start, Rc = _kl_inputs(41)
    g_item = torch.tensor([2.0, 1.5, -0.5, 3.0, 2.5, 2.0])
    eta = torch.tensor([0.0, 0.5, 1.0, -0.3, 2.0, 0.25])
    norm = torch.tensor([0.1, 0.0, 0.05, 1e3, 0.15, 0.1])
    t_e = 0.3
    rc, base = _coef(eng, pred, Rc, x, row_src, None, row_start, lens, N, t_e, 2.0, g_item, eta, norm)
    assert rc == 0
    rc, mapped = _coef(eng, pred, Rc, x, row_src, (Rc + torch.arange(Rc)).to(torch.int32), row_start, lens, N, t_e, 2.0, g_item, eta, norm)
    assert rc == 0 and torch.equal(mapped, base)
    rs = row_src.long()
    for b in range(B):
        n, r0 = lens[b], int(row_start[b])
        if n == 0:
            continue
        N1 = n + 3                                                   # alone: packed rows 0..n-1 of a [1][N1] batch
        x1 = torch.zeros(N1, KL_M)
        x1[:n] = x[rs[r0: r0 + n]]
        p1 = torch.cat([pred[r0: r0 + n], pred[Rc + r0: Rc + r0 + n]])
        rc, alone = _coef(eng, p1, n, x1, torch.arange(n, dtype=torch.int32), None, torch.zeros(1, dtype=torch.int32), [n], N1, t_e, 2.0,
                          g_item[b: b + 1], eta[b: b + 1], norm[b: b + 1])
        assert rc == 0 and torch.equal(alone[0], base[b]), (b, alone, base[b])
    order = [4, 5, 3, 2, 1, 0]                                       # another index, another N, other neighbours
    lens2, N2 = [lens[b] for b in order], 160
    row_src2, row_start2, Rc2 = _layout(lens2, N2)
    assert Rc2 == Rc
    x2, p2 = torch.zeros(B * N2, KL_M), torch.zeros(2 * Rc, KL_LDP)
    for i, b in enumerate(order):
        n, r0, q0 = lens[b], int(row_start[b]), int(row_start2[i])
        x2[i * N2: i * N2 + n] = x[rs[r0: r0 + n]]
        p2[q0: q0 + n] = pred[r0: r0 + n]
        p2[Rc + q0: Rc + q0 + n] = pred[Rc + r0: Rc + r0 + n]
    idx = torch.tensor(order)
    rc, moved = _coef(eng, p2, Rc, x2, row_src2, None, row_start2, lens2, N2, t_e, 2.0, g_item[idx], eta[idx], norm[idx])
    assert rc == 0 and torch.equal(moved, base[idx])


# ------------------------------------------------------------------------------------------------ 2. vv_ode_stage_apg
def _stage_apg(eng, x, pred, ldp, Rc, M, n_prev, k_prev, coef, k_out, x_out, g, g_item, seq_n, row_src, u_row, apg):
    """apg = (coef [B][2] device, x_e device, packed, t_e) or None (the plain / guided entries)."""
    rt = _mods()[0]
    a = rt.vv_ode_stage_args()
    a.x, a.pred, a.ldp, a.Rc, a.n_mel, a.n_prev = x.data_ptr(), pred.data_ptr(), ldp, Rc, M, n_prev
    for j in range(3):
        a.k_prev[j] = k_prev[j].data_ptr() if j < len(k_prev) and k_prev[j] is not None else None
    for j, v in enumerate(coef):
        a.coef[j] = v
    a.k_out = None if k_out is None else k_out.data_ptr()
    a.x_out = None if x_out is None else x_out.data_ptr()
    a.g, a.g_item, a.seq_n = g, None if g_item is None else g_item.data_ptr(), seq_n
    a.row_src = row_src.data_ptr()
    st = torch.cuda.current_stream().cuda_stream
    if apg is None:
        if u_row is None:
            return eng.lib.vv_ode_stage(eng.ctx, C.byref(a), st)
        return eng.lib.vv_ode_stage_guided(eng.ctx, C.byref(a), u_row.data_ptr(), st)
    q = rt.vv_apg_stage_args(apg[0].data_ptr(), apg[1].data_ptr(), 1 if apg[2] else 0, apg[3])
    return eng.lib.vv_ode_stage_apg(eng.ctx, C.byref(a), None if u_row is None else u_row.data_ptr(), C.byref(q), st)


@pytest.mark.parametrize("mapped", [False, True])
@pytest.mark.parametrize("name", ["euler", "midpoint", "rk4"])
def test_apg_stage_against_float64(hip_tiny, name, mapped):
    """Every stage of three methods on ragged rows (lengths 40 / 17 / 29, n_mel 100, ldp 128), fed the device's own coefficients.
    ``mapped``: item 1 has no unconditional rows (u_row -1, coef {0, 0}), the others' are compacted.  Stage 0 reads x_e = x through
    row_src, later stages a packed state.  The reference takes the kernel's two rounded constants as they are (coef and the fp32 1 - t_e).
    Bound per element, N7's form with the extra term: 8 * 2^-24 * (|x| + sum_j |h a_ij| K_j), K = |pc| + |A| |D| + |C| |d| for the fresh
    slope; k_out within 6 * 2^-24 * K (five fp32 roundings: D, the two fused multiply-adds of the combine, d, and one to spare)."""
    ODE_METHODS = _mods()[1]
    eng = hip_tiny["f32"]
    a_t, b_t = ODE_METHODS[name]
    s = len(b_t)
    gen = torch.Generator().manual_seed(500 + s)
    B, N, M, ldp, h = 3, 40, 100, 128, 0.07
    lens = [40, 17, 29]
    row_src, row_start, Rc = _layout(lens, N)
    g_item = torch.tensor([2.0, 1.5, 3.0])
    eta = torch.tensor([0.0, 0.5, 1.0])                              # item 2: C = 0, the combine stops after the plain part
    norm = torch.tensor([0.0, 0.3, 0.2])
    u_row = None
    if mapped:
        u_row = torch.full((Rc,), -1, dtype=torch.int32)
        u_row[:40] = Rc + torch.arange(40, dtype=torch.int32)
        u_row[57:] = Rc + 40 + torch.arange(29, dtype=torch.int32)
    Ru = Rc if u_row is None else int((u_row >= 0).sum())
    has_u = torch.ones(Rc, dtype=torch.bool) if u_row is None else u_row >= 0
    rs = row_src.long()
    item = rs // N
    for i in range(s):
        last = i == s - 1
        t_e = [0.3, 0.55, 0.8125, 1.0][i]
        coef = [np.float32(h * float(b_t[j] if last else a_t[i + 1][j])) for j in range(i + 1)]
        x = torch.randn(B * N, M, generator=gen)
        pred = torch.randn(Rc + Ru, ldp, generator=gen)
        xs = torch.randn(Rc, M, generator=gen)                       # the packed state of a later stage
        k_prev = [torch.randn(Rc, M, generator=gen) for _ in range(i)]
        x_e, xe_rows = (x, x[rs]) if i == 0 else (xs, xs)
        rc, ac = _coef(eng, pred, Rc, x_e, row_src if i == 0 else None, u_row, row_start, lens, N, t_e, 2.0, g_item, eta, norm, M=M, ldp=ldp)
        assert rc == 0, eng.lib.vv_last_error(eng.ctx).decode()
        if mapped:
            assert ac[1].tolist() == [0.0, 0.0]
        assert float(ac[2, 1]) == 0.0 and float(ac[0, 1]) != 0.0
        dx, dp, dxe, dac = x.clone().to(DEV), pred.to(DEV), x_e.to(DEV), ac.to(DEV)
        dk = [k.to(DEV) if coef[j] != 0 else None for j, k in enumerate(k_prev)]
        k_out = torch.full((Rc, M), 7.0, device=DEV)
        x_out = None if last else torch.full((Rc, M), 7.0, device=DEV)
        d_u = None if u_row is None else u_row.to(DEV)
        rc = _stage_apg(eng, dx, dp, ldp, Rc, M, i, dk, [float(c) for c in coef], k_out, x_out, 9.0, None, N, row_src.to(DEV), d_u,
                        (dac, dx if i == 0 else dxe, i > 0, t_e))
        assert rc == 0, eng.lib.vv_last_error(eng.ctx).decode()
        torch.cuda.synchronize()
        pc = pred[:Rc, :M].double()
        pu = torch.zeros_like(pc)
        pu[has_u] = pred[(torch.arange(Rc) + Rc)[has_u] if u_row is None else u_row[has_u].long(), :M].double()
        A, Cc = ac[item, 0].double()[:, None], ac[item, 1].double()[:, None]
        omt = float(np.float32(1.0) - np.float32(t_e))
        D, d = pc - pu, xe_rows.double() + omt * pc
        k = torch.where(has_u[:, None], pc + A * D + Cc * d, pc)
        K = torch.where(has_u[:, None], pc.abs() + A.abs() * D.abs() + Cc.abs() * d.abs(), pc.abs())
        acc, mag = x[rs].double(), x[rs].double().abs()
        for j in range(i):
            if coef[j] != 0:
                acc = acc + float(coef[j]) * k_prev[j].double()
                mag = mag + abs(float(coef[j])) * k_prev[j].double().abs()
        if coef[i] != 0:
            acc = acc + float(coef[i]) * k
            mag = mag + abs(float(coef[i])) * K
        got = (dx.cpu()[rs] if last else x_out.cpu()).double()
        excess = float(((got - acc).abs() - 8 * EPS32 * mag).max())
        k_excess = float(((k_out.cpu().double() - k).abs() - 6 * EPS32 * K).max())
        print(f"{name} stage {i} mapped={mapped}: max excess over the bounds {excess:.3e} (state) {k_excess:.3e} (slope)")
        assert excess <= 0.0 and k_excess <= 0.0, (name, i, mapped, excess, k_excess)
        assert torch.equal(k_out.cpu()[~has_u], pred[:Rc, :M][~has_u])
        untouched = torch.ones(B * N, dtype=torch.bool)
        untouched[rs] = False
        assert torch.equal(dx.cpu()[untouched], x[untouched])
        if not last:
            assert torch.equal(dx.cpu(), x)
        # every item (eta 1, no cap): the coefficients are {g, 0} and the launch has the bits of the plain / guided entry
        rc, off = _coef(eng, pred, Rc, x_e, row_src if i == 0 else None, u_row, row_start, lens, N, t_e, 2.0, g_item, torch.ones(B), torch.zeros(B),
                        M=M, ldp=ldp)
        assert rc == 0
        for b in range(B):
            assert off[b].tolist() == ([float(g_item[b]), 0.0] if bool(has_u[int(row_start[b])]) else [0.0, 0.0])
        outs = []
        for apg in ((off.to(DEV), None, i > 0, t_e), None):
            px = x.clone().to(DEV)
            pk = torch.full((Rc, M), 7.0, device=DEV)
            pxo = None if last else torch.full((Rc, M), 7.0, device=DEV)
            if apg is not None:
                apg = (apg[0], px if i == 0 else dxe, apg[2], apg[3])
            assert _stage_apg(eng, px, dp, ldp, Rc, M, i, dk, [float(c) for c in coef], pk, pxo, 9.0 if apg else 2.0,
                              None if apg else g_item.to(DEV), N, row_src.to(DEV), d_u, apg) == 0
            torch.cuda.synchronize()
            outs.append((px, pk, pxo))
        assert torch.equal(outs[0][0], outs[1][0]) and torch.equal(outs[0][1], outs[1][1]) and (last or torch.equal(outs[0][2], outs[1][2]))


def test_kernel_entries_refuse_and_stay_usable(hip_tiny):
    eng = hip_tiny["f32"]
    x, pred, row_src, row_start, Rc = _kl_inputs(71)
    ok = lambda **kw: _coef(eng, pred, Rc, x, row_src, None, row_start, KL_LENS, KL_N, 0.4, 2.0, None, None, None, **kw)
    rc, base = ok()
    assert rc == 0
    assert ok(M=98)[0] == -22                                         # n_mel % 4
    assert ok(ldp=96)[0] == -22                                       # ldp < n_mel
    big = 1025                                                        # more items than N8's tables take
    rc, _ = _coef(eng, pred, Rc, x, row_src, None, torch.zeros(big, dtype=torch.int32), [0] * big, KL_N, 0.4, 2.0, None, None, None)
    assert rc == -22
    rc, _ = _coef(eng, pred, Rc, x, row_src, None, row_start, KL_LENS, KL_N, float("nan"), 2.0, None, None, None)
    assert rc == -22
    # the stage: x_e must not be the launch's x_out, and coef is required
    M, ldp = KL_M, KL_LDP
    dx, dp, drs = x.clone().to(DEV), pred.to(DEV), row_src.to(DEV)
    x_out, k_out = torch.zeros(Rc, M, device=DEV), torch.zeros(Rc, M, device=DEV)
    dac = base.to(DEV)
    assert _stage_apg(eng, dx, dp, ldp, Rc, M, 0, [], [0.1], k_out, x_out, 2.0, None, KL_N, drs, None, (dac, x_out, True, 0.4)) == -22
    assert _stage_apg(eng, dx, dp, ldp, Rc, M, 0, [], [0.1], k_out, x_out, 2.0, None, 0, drs, None, (dac, dx, False, 0.4)) == -22      # seq_n
    torch.cuda.synchronize()
    assert torch.equal(dx.cpu(), x) and float(x_out.abs().max()) == 0.0                   # nothing ran
    assert _stage_apg(eng, dx, dp, ldp, Rc, M, 0, [], [0.1], k_out, x_out, 2.0, None, KL_N, drs, None, (dac, dx, False, 0.4)) == 0
    rc, again = ok()
    assert rc == 0 and torch.equal(again, base)


# ------------------------------------------------------------------------------------------------ 3. the solver entry against the reference
@pytest.mark.parametrize("name", ["euler", "rk4"])
def test_apg_against_the_reference_solver(own, tiny_setup, name):
    spec = tiny_setup[0]
    engs, orc = own
    eng = engs["f32"]
    g = float(spec.cfg_strength)
    batch = make_batch(spec, RAGGED["a"], RAGGED["t"], RAGGED["g"], seed=3)
    d = _dev(batch)
    eng.set_nfe(5, name)                                             # a 5-point grid: 4 ODE steps
    x = _run(eng, d, _pre(eng, d), apg=_apg(ETAS, CAPS)).cpu()
    torch.cuda.synchronize()
    ever = []
    for b in range(3):
        pre, sl = _oracle_pre(orc, batch, b)
        ref, capped = ref_solve_apg(orc, pre, pre["noise"], name, 5, g, ETAS[b], CAPS[b])
        ever.append(any(capped))
        err = _err(x[b, :sl], ref)
        print(f"{name} item {b} eta {ETAS[b]} cap {CAPS[b]}: err {err:.3e} of range; capped at {sum(capped)} of {len(capped)} evaluations")
        assert err < TOL, (name, b, err)
        if b == 0:                                                   # eta = 0 must move the trajectory, or the test shows nothing
            plain, _ = ref_solve_apg(orc, pre, pre["noise"], name, 5, g, 1.0, None, apg=False)
            apart = _err(ref, plain)
            print(f"{name}: eta = 0 reference vs the plain-CFG reference {apart:.3e} of range")
            assert apart > 1e-2, (name, apart)
    assert not ever[0] and ever[1], ever                              # one item is never capped, one is capped somewhere


# ------------------------------------------------------------------------------------------------ 4. off means off
@pytest.mark.parametrize("name", ["euler", "rk4"])
@pytest.mark.parametrize("dt", ["f32", "bf16"])
def test_off_means_off(own, tiny_setup, dt, name):
    """Every item (eta 1, no cap) THROUGH the projected kernels == the existing entries, bit for bit; the Python entry does not even
    reach them when the pair is a pair of Nones."""
    spec = tiny_setup[0]
    eng = own[0][dt]
    d = _dev(make_batch(spec, RAGGED["a"], RAGGED["t"], RAGGED["g"], seed=3))
    off = _apg([1.0] * 3, [None] * 3)
    cfg = torch.tensor([2.0, 0.75, 3.25], dtype=torch.float32, device=DEV)
    try:
        eng.set_nfe(8 if name == "euler" else 3, name)
        pre = _pre(eng, d)
        mask = torch.ones((eng.n_evals, 3), dtype=torch.uint8)
        mask[1:3, 1] = 0
        mask[:, 2] = 0
        for lanes in (1, 2):
            eng.set_option("lanes", lanes)
            x0 = _run(eng, d, pre)                                   # vv_transformer_steps_ex
            x1 = _run(eng, d, pre, apg=off)
            x2 = _run(eng, d, pre, apg=(off[0], None))
            x3 = _run(eng, d, pre, apg=(None, off[1]))
            g0 = _run(eng, d, pre, guide=mask, cfg=cfg)              # vv_transformer_steps_guided
            g1 = _run(eng, d, pre, guide=mask, cfg=cfg, apg=off)
            x4 = d["noise"].clone()
            eng.transformer_steps(x4, pre, 0, eng.n_steps, apg=(None, None))
            torch.cuda.synchronize()
            assert torch.equal(x1, x0) and torch.equal(x2, x0) and torch.equal(x3, x0) and torch.equal(x4, x0), (dt, name, lanes)
            assert torch.equal(g1, g0), (dt, name, lanes)
    finally:
        eng.set_option("lanes", 0)


# ------------------------------------------------------------------------------------------------ 5. invariances, bit for bit
@pytest.mark.parametrize("dt,name", [("f32", "rk4"), ("bf16", "euler"), ("bf16", "midpoint")])
def test_invariances_are_bit_identical(own, tiny_setup, dt, name):
    spec = tiny_setup[0]
    eng = own[0][dt]
    batch = make_batch(spec, RAGGED["a"], RAGGED["t"], RAGGED["g"], seed=11)
    d = _dev(batch)
    eng.set_nfe({"rk4": 3, "euler": 9, "midpoint": 5}[name], name)
    assert eng.n_evals == 8
    cfg = torch.tensor([2.0, 0.75, 3.25], dtype=torch.float32, device=DEV)
    etas, caps = [0.0, 0.5, 0.25], [None, 0.05, 0.4]
    apg = _apg(etas, caps)
    pre = _pre(eng, d)
    try:
        eng.set_option("lanes", 1)
        x1 = _run(eng, d, pre, cfg=cfg, apg=apg)
        xp = _run(eng, d, pre, cfg=cfg)
        torch.cuda.synchronize()
        assert not torch.equal(x1, xp)
        eng.set_option("lanes", 2)
        x2 = _run(eng, d, pre, cfg=cfg, apg=apg)
        torch.cuda.synchronize()
        assert torch.equal(x1, x2), "lanes"
        for b in range(3):                                           # batch == each item alone (one lane, and its branches as the lanes)
            one, sl = _one(spec, d, batch, b)
            for lanes in (1, 2):
                eng.set_option("lanes", lanes)
                xa = _run(eng, one, _pre(eng, one), cfg=cfg[b: b + 1].contiguous(), apg=_apg(etas[b: b + 1], caps[b: b + 1]))
                torch.cuda.synchronize()
                assert torch.equal(xa[0], x1[b, :sl]), ("alone", b, lanes)
        eng.set_option("lanes", 0)
        xs = d["noise"].clone()                                      # split by step0 / n_steps: nothing is carried between the calls
        half = eng.n_steps // 2
        _run(eng, d, pre, cfg=cfg, apg=apg, step0=0, n=half, x=xs)
        _run(eng, d, pre, cfg=cfg, apg=apg, step0=half, n=eng.n_steps - half, x=xs)
        torch.cuda.synchronize()
        assert torch.equal(xs, x1), "split"
        lens = [int(v) for v in batch["seq_len"]]                    # a caller-owned workspace of the size the library names
        need = eng.apg_ws_bytes(3, d["N"], lens)
        assert need > eng.guided_ws_bytes(3, d["N"], lens)
        ws = torch.empty((need,), dtype=torch.uint8, device=DEV)
        xw = _run(eng, d, pre, cfg=cfg, apg=apg, ws=ws)
        torch.cuda.synchronize()
        assert torch.equal(xw, x1), "ws"
        with pytest.raises(RuntimeError, match="too small"):
            _run(eng, d, pre, cfg=cfg, apg=apg, ws=ws[: eng.guided_ws_bytes(3, d["N"], lens)])
        xg = d["noise"].clone()                                      # captured into a hipGraph: no synchronisation, nothing that moves
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            _run(eng, d, pre, cfg=cfg, apg=apg, ws=ws, x=xg)
        xg.copy_(d["noise"])
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(xg, x1), "graph"
        del graph
        # an N8 mask: items 0 and 1 guided at evaluations 4..7 alone, item 2 never.  Up to the first guided evaluation (ODE steps before
        # it) the run IS the masked run without APG; item 2, never guided, is untouched through the whole run; the masked APG run itself
        # keeps the structure properties
        mask = torch.zeros((8, 3), dtype=torch.uint8)
        mask[4:, :2] = 1
        first = 4 // (8 // eng.n_steps)                              # the ODE step of evaluation 4
        ma = _run(eng, d, pre, guide=mask, cfg=cfg, apg=apg, n=first)
        mp = _run(eng, d, pre, guide=mask, cfg=cfg, n=first)
        torch.cuda.synchronize()
        assert torch.equal(ma, mp), "outside the interval"
        ma = _run(eng, d, pre, guide=mask, cfg=cfg, apg=apg)
        mp = _run(eng, d, pre, guide=mask, cfg=cfg)
        eng.set_option("lanes", 2)
        m2 = _run(eng, d, pre, guide=mask, cfg=cfg, apg=apg)
        eng.set_option("lanes", 0)
        mw = _run(eng, d, pre, guide=mask, cfg=cfg, apg=apg, ws=ws)
        torch.cuda.synchronize()
        assert torch.equal(ma[2], mp[2]), "an unguided item"
        assert not torch.equal(ma[0], mp[0]) and not torch.equal(ma[1], mp[1])
        assert torch.equal(m2, ma) and torch.equal(mw, ma), "masked: lanes / ws"
    finally:
        eng.set_option("lanes", 0)


# ------------------------------------------------------------------------------------------------ 6. bf16: the format's cost
def test_bf16_error_stays_the_formats(own, tiny_setup):
    """N7's convention: the RMSE of the bf16 run against the float64 reference of the SAME rule, pooled over the items' valid frames;
    the projected rule's may be at most 1.5 x the plain rule's measured here (both figures are printed)."""
    spec = tiny_setup[0]
    engs, orc = own
    eng = engs["bf16"]
    g = float(spec.cfg_strength)
    batch = make_batch(spec, RAGGED["a"], RAGGED["t"], RAGGED["g"], seed=3)
    d = _dev(batch)
    eng.set_nfe(5, "euler")
    pre = _pre(eng, d)
    xa = _run(eng, d, pre, apg=_apg(ETAS, CAPS)).cpu()
    xp = _run(eng, d, pre).cpu()
    torch.cuda.synchronize()
    se = {"apg": 0.0, "plain": 0.0}
    n = 0
    for b in range(3):
        opre, sl = _oracle_pre(orc, batch, b)
        ra, _ = ref_solve_apg(orc, opre, opre["noise"], "euler", 5, g, ETAS[b], CAPS[b])
        rp, _ = ref_solve_apg(orc, opre, opre["noise"], "euler", 5, g, 1.0, None, apg=False)
        se["apg"] += float(((xa[b, :sl].double() - ra) ** 2).sum())
        se["plain"] += float(((xp[b, :sl].double() - rp) ** 2).sum())
        n += ra.numel()
    rmse_a, rmse_p = math.sqrt(se["apg"] / n), math.sqrt(se["plain"] / n)
    print(f"bf16 RMSE against float64: projected {rmse_a:.4e}, plain {rmse_p:.4e}, ratio {rmse_a / rmse_p:.3f}")
    assert rmse_a <= 1.5 * rmse_p, (rmse_a, rmse_p)


# ------------------------------------------------------------------------------------------------ 7. errors
def test_refused_calls_leave_the_context_usable(own, tiny_setup):
    spec = tiny_setup[0]
    eng = own[0]["bf16"]
    rt = _mods()[0]
    d = _dev(make_batch(spec, RAGGED["a"], RAGGED["t"], RAGGED["g"], seed=8))
    eng.set_nfe(8, "euler")
    pre = _pre(eng, d)
    apg = _apg(ETAS, CAPS)
    mask = torch.zeros((7, 3), dtype=torch.uint8)
    mask[2:5] = 1
    x0 = _run(eng, d, pre, guide=mask, apg=apg)
    x = d["noise"].clone()
    with pytest.raises(RuntimeError, match="ld_guide"):
        _run(eng, d, pre, guide=mask[:, :2].contiguous(), apg=apg, x=x)
    with pytest.raises(ValueError):
        _run(eng, d, pre, apg=(apg[0][:2].contiguous(), apg[1]), x=x)           # not [B]
    with pytest.raises(ValueError):
        _run(eng, d, pre, apg=(apg[0].cpu(), apg[1]), x=x)                      # not on the device
    try:
        eng.set_option("split_k_tail", 1)
        with pytest.raises(RuntimeError, match="split_k_tail"):
            _run(eng, d, pre, guide=mask, apg=apg, x=x)
    finally:
        eng.set_option("split_k_tail", 0)
    a = rt.vv_steps_args()                                                       # the C entry itself: no t_host, and 1025 items
    a.B, a.N, a.seq_len, a.x = 3, d["N"], pre["seq_len"].data_ptr(), x.data_ptr()
    host = _host(d)
    a.seq_len_host = C.cast(host, C.c_void_p)
    a.cat_mel_text, a.cat_mel_text_drop = pre["cat_mel_text"].data_ptr(), pre["cat_mel_text_drop"].data_ptr()
    a.rope_cos_q, a.rope_sin_q = pre["rope_cos_q"].data_ptr(), pre["rope_sin_q"].data_ptr()
    a.rope_cos_k, a.rope_sin_k = pre["rope_cos_k"].data_ptr(), pre["rope_sin_k"].data_ptr()
    a.step0, a.n_steps = 0, eng.n_steps
    q = rt.vv_apg_args(apg[0].data_ptr(), apg[1].data_ptr(), None)
    st = torch.cuda.current_stream().cuda_stream
    assert eng.lib.vv_transformer_steps_apg(eng.ctx, C.byref(a), None, 0, C.byref(q), st) == -22
    big = (C.c_int32 * 1025)(*([4] * 1025))
    a.B, a.seq_len_host = 1025, C.cast(big, C.c_void_p)
    q = rt.vv_apg_args(apg[0].data_ptr(), apg[1].data_ptr(), C.cast(eng._t_host, C.c_void_p))
    assert eng.lib.vv_transformer_steps_apg(eng.ctx, C.byref(a), None, 0, C.byref(q), st) == -22
    nb = C.c_uint64()
    assert eng.lib.vv_transformer_apg_ws_bytes(eng.ctx, 1025, d["N"], big, C.byref(nb)) == -22
    torch.cuda.synchronize()
    assert torch.equal(x, d["noise"])                                          # nothing ran
    x1 = _run(eng, d, pre, guide=mask, apg=apg)
    torch.cuda.synchronize()
    assert torch.equal(x1, x0)


# ------------------------------------------------------------------------------------------------ 8. the profiler's classes
def test_new_launches_count_as_elementwise(own, tiny_setup):
    """Two more launches per evaluation and lane under VV_PROF_ELEMWISE; no other class moves."""
    spec = tiny_setup[0]
    eng = own[0]["bf16"]
    d = _dev(make_batch(spec, RAGGED["a"], RAGGED["t"], RAGGED["g"], seed=6))
    eng.set_nfe(9, "euler")
    pre = _pre(eng, d)
    cfg = torch.full((3,), 2.0, dtype=torch.float32, device=DEV)      # the plain run through the stage kernel too
    try:
        eng.set_option("lanes", 1)
        got = {}
        for kind, apg in (("plain", None), ("apg", _apg(ETAS, CAPS))):
            eng.prof_enable(True)
            eng.prof_collect()
            _run(eng, d, pre, cfg=cfg, apg=apg)
            got[kind] = eng.prof_collect()
            eng.prof_enable(False)
        assert got["apg"]["elementwise"]["launches"] - got["plain"]["elementwise"]["launches"] == 2 * eng.n_evals
        for cls in got["plain"]:
            if cls != "elementwise":
                assert got["apg"][cls]["launches"] == got["plain"][cls]["launches"], cls
    finally:
        eng.prof_enable(False)
        eng.set_option("lanes", 0)


# ------------------------------------------------------------------------------------------------ 9. engine level
ENGINE_APG = dict(apg_eta=0.0, apg_norm=0.3)


def _engine(tmp, **kw):
    from vietvoice_tts_amd.core import ModelConfig, TTSEngine
    cfg = ModelConfig(model_cache_dir=str(tmp), synthetic_model=True, model_spec="tiny", nfe_step=8, acoustic_dtype="fp32",
                      max_chunk_duration=8.0, **kw)
    return TTSEngine(cfg)


def _lsb(a, b):
    return int(np.abs(a.astype(np.int32) - b.astype(np.int32)).max())


def test_engine_device_session_and_stream_paths(tmp_path):
    """The <= 2 LSB figures are the N2 / N7 / N8 tolerances of the same comparisons without projected guidance."""
    e1 = _engine(tmp_path, **ENGINE_APG)
    wave_dev, _ = e1.synthesize(LONG)
    assert len(e1._last_plan) > 1
    e1.cleanup()
    for fuse in (1, 2):
        e2 = _engine(tmp_path, fuse_nfe=fuse, **ENGINE_APG)
        ref, txt = e2.model_session_manager.select_sample()
        waves = e2._synthesize_sessions(e2._prepare_inputs(ref, txt, LONG))
        wave_ses = e2.audio_processor.concatenate_with_crossfade_improved(waves, e2.config.cross_fade_duration, e2.config.sample_rate)
        e2.cleanup()
        assert wave_ses.shape == wave_dev.shape and _lsb(wave_ses, wave_dev) <= 2, fuse
    e3 = _engine(tmp_path, **ENGINE_APG)
    got = np.concatenate(list(e3.synthesize_stream(LONG, chunks_per_step=1)))
    e3.cleanup()
    assert got.shape == wave_dev.shape and _lsb(got, wave_dev) <= 2
    e4 = _engine(tmp_path)                                                       # the default engine, same seed: another trajectory
    wave_all, _ = e4.synthesize(LONG)
    e4.cleanup()
    assert wave_all.shape == wave_dev.shape and _lsb(wave_all, wave_dev) > 2
    e5 = _engine(tmp_path, apg_eta=1.0)                                          # eta 1 without a cap is "off": the default engine's samples
    wave_off, _ = e5.synthesize(LONG)
    e5.cleanup()
    assert np.array_equal(wave_off, wave_all)


def test_engine_edit_speech(tmp_path):
    from vietvoice_tts_amd.pack import MAX_POS
    from vietvoice_tts_amd.speech_edit import plan_edit
    e = _engine(tmp_path, **ENGINE_APG)
    e0 = _engine(tmp_path)
    sr, hop = e.config.sample_rate, e.config.hop_length
    clip, _ = e0.synthesize("Xin chào các bạn, hôm nay trời đẹp quá.")
    dur = clip.size / sr
    parts, fix, text = [(0.3 * dur, 0.5 * dur)], [0.3 * dur], "Xin chào các anh, hôm nay trời đẹp quá."
    out, _ = e.edit_speech(clip, text, parts, fix_duration=fix, seed=11)
    base, _ = e0.edit_speech(clip, text, parts, fix_duration=fix, seed=11)
    plan = plan_edit(clip.size, parts, fix, sr, hop, e.model_session_manager.spec.n_fft, MAX_POS)
    assert out.dtype == np.int16 and out.size == plan.spliced_len
    assert base.shape == out.shape and _lsb(base, out) > 2
    # the kept frames are restored exactly: the state after the edit holds the conditioning's mel there, with and without APG
    eng = e.model_session_manager.engine
    ids = e.text_processor.text_to_indices([list(e.text_processor.clean_text(text))])
    entry = e.voice_bank.get(e.audio_processor.to_wav_bytes(clip, sr))
    dev = eng.device
    keep = torch.from_numpy(plan.keep.reshape(1, -1)).to(dev)
    noise = torch.randn((1, plan.n_frames, eng.spec.n_mel), generator=torch.Generator().manual_seed(11)).to(dev)
    args = (entry.pcm_dev, plan.rows(), [plan.spliced_len], torch.from_numpy(np.ascontiguousarray(ids, dtype=np.int32)).to(dev),
            torch.tensor([ids.shape[1]], dtype=torch.int32, device=dev), keep)
    eng.set_nfe(e.config.nfe_step, e.config.ode_method)
    xa, _, _ = eng.edit_batch(*args, noise, apg=eng.apg_tensors([0.0], [0.3]))
    xp, _, _ = eng.edit_batch(*args, noise)
    torch.cuda.synchronize()
    kept = torch.from_numpy(plan.keep[: plan.n_frames].astype(bool))
    assert 0 < int(kept.sum()) < plan.n_frames
    assert torch.equal(xa[0].cpu()[kept], xp[0].cpu()[kept])                     # both ARE the conditioning's mel there
    assert not torch.equal(xa[0].cpu()[~kept], xp[0].cpu()[~kept])
    e.cleanup()
    e0.cleanup()


def test_batching_frontend_per_request_apg(tmp_path):
    from vietvoice_tts_amd.batching import BatchingFrontend
    e = _engine(tmp_path)
    fe = BatchingFrontend(e, max_wait_ms=300.0, max_requests=8)
    text, bye = "Xin chào các bạn, hôm nay thế nào?", "Tạm biệt và hẹn gặp lại."
    try:
        alone = fe.submit(text, speed=1.0, serial=7, apg_eta=0.0, apg_norm=0.3).result(timeout=300)[0]
        plain_a = fe.submit(text, speed=1.0, serial=7).result(timeout=300)[0]
        plain_b = fe.submit(bye, speed=1.3, serial=8, gender="male").result(timeout=300)[0]
        n0 = fe.batches_run
        futs = [fe.submit(bye, speed=1.3, serial=8, gender="male"),
                fe.submit(text, speed=1.0, serial=7, apg_eta=0.0, apg_norm=0.3),
                fe.submit(text, speed=1.0, serial=7)]
        outs = [f.result(timeout=300)[0] for f in futs]
        assert fe.batches_run == n0 + 1                                          # plain and projected requests share one batch
        assert outs[1].shape == alone.shape and _lsb(outs[1], alone) <= 2
        assert outs[0].shape == plain_b.shape and _lsb(outs[0], plain_b) <= 2    # the plain ones: their plain-engine output
        assert outs[2].shape == plain_a.shape and _lsb(outs[2], plain_a) <= 2
        assert plain_a.shape == alone.shape and _lsb(plain_a, alone) > 2
        for bad in (dict(apg_eta=float("nan")), dict(apg_norm=0.0), dict(apg_norm=-1.0), dict(apg_eta="x")):
            with pytest.raises(ValueError):
                fe.submit(text, **bad).result(timeout=5)
    finally:
        fe.close()
        e.cleanup()
