"""Cases, float64 references, scales, counts, yardsticks and launch helpers for the kernels between the transformer's prediction and
the PCM (tests/test_step_gpu.py on the device, tests/test_step_ref_cpu.py without one):

  vv_elementwise.hip  pack_cat / pack_cat_guided, cfg_euler, ode_stage (four instantiations), apg_reduce / apg_coef, row_tables /
                      guided_tables, ref_len / decode_len, rope_compact / rope_rows
  vv_vocoder.hip      conv_post (four instantiations), mel_slice
  vv_vocos.hip        vocos_lens, vocos_im2col, vocos_spectrum, vocos_ola

The standard is that of gpu_util: a float64 reference on the operands as the kernel receives them, err = max_e (|got_e - ref_e| -
allow_e) / A_e with a per-element scale A_e, a bound max(c 2^-24, 4 x yardstick) where c is counted from the kernel's roundings and the
yardstick is the CPU library's fp32 evaluation under the same metric; a gather or an integer table is compared bit for bit.  Every
reference takes ``mut``: a named, plausible bug applied to the formula, which test_step_ref_cpu.py requires the bound to reject.

Every launch helper puts outputs between bands of 7.0, NaN into the padding columns and behind every operand, inputs that a length or
an offset indexes between NaN guard rows, checks the guards after the launch, and runs twice and requires the same bits."""
import ctypes as C
import dataclasses
import math

import numpy as np
import torch

from tests.gpu_util import CONV_FILL, DEV, EPS24, NAN, _bands_intact, _guarded, check, parity_err, stream
from vietvoice_tts_amd import runtime as rt
from vietvoice_tts_amd.model_spec import ODE_METHODS

FILL = CONV_FILL
GUARD_ROWS = 3
APG_TILE = rt.APG_TILE
EPS53 = 2.0 ** -53
F32_MIN_NORMAL = 2.0 ** -126
I32 = torch.int32


def grid_for(total):
    """vv_elementwise.hip grid_for: workgroups of 256 threads, at most 2048 of them; a grid-stride loop covers the rest."""
    return min((total + 255) // 256, 256 * 8)


def grid_1d(total):
    """vv_vocos.hip grid_1d: at most 8192 workgroups."""
    return min((total + 255) // 256, 256 * 32)


def wraps(total, grid):
    """True when one trip of the grid-stride loop does not cover `total` work items."""
    return total > grid(total) * 256


def _gen(seed):
    return torch.Generator().manual_seed(seed)


def same_bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and bool((a.contiguous().view(torch.uint8) == b.contiguous().view(torch.uint8)).all())


def twice(launch):
    """Run a launch helper twice on fresh buffers; every returned tensor must have the same bits both times."""
    a, b = launch(), launch()
    for k in a:
        if a[k] is not None:
            assert same_bits(a[k], b[k]), f"{k}: the repeat differs from the first launch"
    return a


def framed(t, front=GUARD_ROWS, behind=GUARD_ROWS, fill=NAN):
    """t [R][...] on the device inside a larger allocation with `front` / `behind` guard rows of `fill` -> (whole, view of t)."""
    t = t.contiguous()
    row = int(math.prod(t.shape[1:])) if t.dim() > 1 else 1
    whole = torch.full(((front + t.shape[0] + behind) * row,), fill, dtype=t.dtype, device=DEV)
    view = whole[front * row:(front + t.shape[0]) * row].view(t.shape)
    view.copy_(t)
    return whole, view


def frame_intact(whole, view, what, fill=NAN):
    n0 = (view.data_ptr() - whole.data_ptr()) // whole.element_size()
    rest = torch.cat([whole[:n0], whole[n0 + view.numel():]])
    ok = torch.isnan(rest).all() if fill != fill else (rest == fill).all()
    assert bool(ok), f"{what}: a guard row was written"


def table(values, poison, n_behind=8):
    """An int32 table on the device with `n_behind` poison entries behind it: indices that are valid to dereference but name a NaN row (or
    a sentinel), so an entry read past the table shows in the result and never leaves the test's memory."""
    t = torch.cat([torch.as_tensor(values, dtype=I32).reshape(-1), torch.full((n_behind,), int(poison), dtype=I32)]).to(DEV)
    return t, t[:t.numel() - n_behind]


def ptr(t):
    return None if t is None else t.data_ptr()


def out_rows(R, ld, dtype=torch.float32):
    """[R][ld] output of 7.0 between bands of GUARD_ROWS rows of 7.0 -> (whole, view, guard elements)."""
    guard = GUARD_ROWS * ld
    whole, view = _guarded((R, ld), guard, FILL, init=torch.full((R, ld), FILL, dtype=dtype), dtype=dtype)
    return whole, view, guard


def bound_of(c, yard=0.0):
    return max(c * EPS24, 4.0 * yard)


# ================================================================================================ ode_stage / cfg_euler
# Counts (derived; the device result plays no part).  Per element, in units of 2^-24 x the scale:
#   slope   k = pc + (pc - pu) g:  D = fl(pc - pu) errs by <= |D| <= |pc| + |pu|, carried by |g|; then either one fma or a product and an
#           add: <= |g D| + |k|.  Sum <= 3 K with K = |pc| + |g| (|pc| + |pu|); 4 leaves one to spare.                    SLOPE_C = 4
#   APG     k' = fma(C, d, k), d = fma(1 - t, pc, xe): one rounding of d carried by |C|, one of k'.  K gains |C| |d|.      APG_SLOPE_C = 6
#   state   acc = ((x + c_1 k_1) + c_2 k_2) + ... + c_new k, at most four terms, the fresh slope last.  Products: |t_j| each; the m-th add
#           <= |x| + sum_{j <= m} |t_j|; the fresh slope's own error (3 K, or 5 K with APG) carried by |c_new|.  The coefficient of |x| is 4,
#           of |t_1| 5, |t_2| 4, |t_3| 3 and of |c_new| K at most 1 + 1 + 5 = 7: all <= 8 x mag, mag = |x| + sum |c_j| K_j.  STATE_C = 8
#           (with fused multiply-adds there are fewer roundings, never more).
SLOPE_C, APG_SLOPE_C, STATE_C = 4.0, 6.0, 8.0
STAGE_SHAPES = ((4, 4), (4, 8), (4, 128), (100, 100), (100, 104), (100, 128), (128, 128), (128, 132))      # (n_mel, ldp)
STAGE_LENS = {1: ((1,), 5), 3: ((1, 1, 1), 5), 86: ((40, 17, 29), 40), 21000: ((7000, 7000, 7000), 7000)}  # Rc -> (item lengths, seq_n)
STAGE_G = (0.0, 2.0, -0.5)
U_MAPS = ("all", "none", "alt", "identity")
T_E = (0.3, 0.55, 0.8125, 1.0)


def method_stages():
    return [(m, i) for m in ("euler", "midpoint", "heun2", "heun3", "rk4") for i in range(len(ODE_METHODS[m][1]))]


@dataclasses.dataclass
class StageCase:
    name: str
    inst: str                  # plain | guided | apg | apg_guided: ode_stage_kernel<GUIDED, APG>;  euler | euler_rows: cfg_euler_kernel
    n_mel: int
    ldp: int
    Rc: int
    method: str = "euler"
    stage: int = 0
    g: float = 2.0
    per_item: bool = False
    rows: bool = True          # x is the padded [B][N] plane read through row_src; False: x is [Rc][n_mel], item = r // seq_n
    u_map: str = "all"
    c_zero: bool = False
    seed: int = 0
    h: float = 0.07

    @property
    def lens(self):
        return STAGE_LENS[self.Rc][0]

    @property
    def N(self):
        return STAGE_LENS[self.Rc][1]

    @property
    def B(self):
        return len(self.lens) if self.rows else -(-self.Rc // self.N)

    @property
    def euler(self):
        return self.inst.startswith("euler")

    @property
    def guided(self):
        return self.inst in ("guided", "apg_guided")

    @property
    def apg(self):
        return self.inst.startswith("apg")

    @property
    def last(self):
        return self.stage == len(ODE_METHODS[self.method][1]) - 1

    @property
    def coef(self):
        """h a[i + 1][j] (h b[j] on the last stage) as the fp32 values the launcher receives; j = stage is the fresh slope's."""
        a_t, b_t = ODE_METHODS[self.method]
        return [np.float32(self.h * float(b_t[j] if self.last else a_t[self.stage + 1][j])) for j in range(self.stage + 1)]

    @property
    def total(self):
        return self.Rc * (self.n_mel // 4)

    def ops(self):
        g = _gen(self.seed)
        Rc, M, N, B = self.Rc, self.n_mel, self.N, self.B
        o = type("Ops", (), {})()
        if self.rows:
            o.row_src = torch.cat([b * N + torch.arange(n) for b, n in enumerate(self.lens)]).to(I32)
            o.x = torch.randn(B * N, M, generator=g)
            named = torch.zeros(B * N, dtype=torch.bool)
            named[o.row_src.long()] = True
            o.x[~named] = NAN                                        # rows of x no row_src entry names
        else:
            o.row_src = None
            o.x = torch.randn(Rc, M, generator=g)
        xr = o.row_src.long() if self.rows else torch.arange(Rc)
        o.xr, o.item = xr, xr // N
        o.u_row = None
        Ru = Rc
        if self.guided:
            mapped = {"all": torch.ones(Rc, dtype=torch.bool), "identity": torch.ones(Rc, dtype=torch.bool),
                      "none": torch.zeros(Rc, dtype=torch.bool), "alt": (o.item % 2) == 0}[self.u_map]
            Ru = int(mapped.sum())
            o.u_row = torch.full((Rc,), -1, dtype=I32)
            o.u_row[mapped] = Rc + torch.arange(Ru, dtype=I32)
        o.Ru = Ru
        o.pred = torch.randn(Rc + Ru, self.ldp, generator=g)
        o.pred[:, M:] = NAN
        o.k_prev = [torch.randn(Rc, M, generator=g) for _ in range(self.stage)]
        o.g_item = torch.tensor([(2.0, -0.5, 3.5, 0.0)[b % 4] for b in range(B)]) if self.per_item else None
        o.apg_coef = o.x_e = None
        o.xe_packed = 0
        if self.apg:
            o.apg_coef = torch.stack([2.0 + 0.5 * torch.randn(B, generator=g), 0.3 * torch.randn(B, generator=g)], dim=1).contiguous()
            if self.c_zero:
                o.apg_coef[:, 1] = 0.0
            elif B > 1:
                o.apg_coef[1, 1] = 0.0                               # one item stops after the plain part
            o.t_e = T_E[self.stage]
            if self.stage > 0:
                o.x_e, o.xe_packed = torch.randn(Rc, M, generator=g), 1      # the packed state of a later stage
        return o


STAGE_MUTATIONS = ("swap_sign", "item_of_r", "skip_coef", "pu_from_Rc_r", "xe_from_r")


def stage_mut_applies(case, mut):
    """-> None when the mutation changes what the case computes, else the reason it is skipped."""
    nz = [c for c in case.coef if c != 0]
    if mut == "swap_sign":
        if (case.g == 0.0 and not case.per_item and not case.apg) or (case.guided and case.u_map == "none"):
            return "no guided row, or g == 0: the difference does not enter"
        return None if (case.euler or case.coef[-1] != 0) else "the fresh slope has a zero coefficient and k_out is not compared here"
    if mut == "item_of_r":
        if not (case.per_item or case.apg) or case.euler:
            return "no per-item strength"
        if not case.rows or case.B == 1 or all(n == case.N for n in case.lens[:-1]):
            return "r / seq_n and row_src[r] / seq_n name the same item on every row"
        if case.guided and case.u_map == "none":
            return "no guided row"
        return None
    if mut == "skip_coef":
        return None if nz else "every coefficient is zero"
    if mut == "pu_from_Rc_r":
        return None if case.guided and case.u_map == "alt" and case.B > 1 else "u_row is not compacted"
    if mut == "xe_from_r":
        if not case.apg or case.stage > 0 or not case.rows or case.c_zero or (case.guided and case.u_map == "none"):
            return "x_e is packed, or C == 0 everywhere"
        return None if any(n != case.N for n in case.lens[:-1]) else "row r is row row_src[r]"
    raise KeyError(mut)


def stage_eval(case, o, dtype=torch.float64, mut=None):
    """-> dict(k, K, acc, mag): the slope and the state of the packed rows in `dtype`, and their scales (always float64)."""
    Rc, M, N = case.Rc, case.n_mel, case.N
    t = lambda v: v.to(dtype)
    pc = t(o.pred[:Rc, :M])
    r = torch.arange(Rc)
    item = (r // N) if mut == "item_of_r" else o.item
    has_u = torch.ones(Rc, dtype=torch.bool) if o.u_row is None else o.u_row >= 0
    ur = (Rc + r) if (o.u_row is None or mut == "pu_from_Rc_r") else o.u_row.long()
    if mut == "pu_from_Rc_r":
        has_u = torch.ones(Rc, dtype=torch.bool)
    pool = torch.cat([o.pred[:, :M], torch.full((Rc, M), NAN)])      # a row past pred is a NaN guard row
    pu = t(pool[ur.clamp_min(0)])
    if case.apg:
        A, Cc = t(o.apg_coef[item, 0])[:, None], t(o.apg_coef[item, 1])[:, None]
    else:
        A = t(o.g_item[item])[:, None] if o.g_item is not None else torch.tensor(case.g, dtype=dtype)
        Cc = None
    D = (pu - pc) if mut == "swap_sign" else (pc - pu)
    k = pc + D * A
    K = pc.double().abs() + A.double().abs() * (pc.double().abs() + pu.double().abs())
    if case.apg:
        omt = torch.tensor(float(np.float32(1.0) - np.float32(o.t_e)), dtype=dtype)
        if o.xe_packed:
            xe = t(o.x_e)
        else:
            xe = t(o.x[r if mut == "xe_from_r" else o.xr])
        d = xe + omt * pc
        k = torch.where(Cc != 0, k + Cc * d, k)
        K = K + Cc.double().abs() * d.double().abs()
    k = torch.where(has_u[:, None], k, pc)
    K = torch.where(has_u[:, None], K, pc.double().abs())
    if case.euler:
        coef, prev = [np.float32(case.h)], []
    else:
        coef, prev = list(case.coef), o.k_prev
    skip = max((j for j, c in enumerate(coef) if c != 0), default=-1) if mut == "skip_coef" else -1
    acc = t(o.x[o.xr])
    mag = acc.double().abs()
    for j, c in enumerate(coef):
        if c == 0:
            continue
        kj, Kj = (k, K) if j == len(coef) - 1 else (t(prev[j]), prev[j].double().abs())
        mag = mag + abs(float(c)) * Kj
        if j != skip:
            acc = acc + torch.tensor(float(c), dtype=dtype) * kj
    return dict(k=k, K=K, acc=acc, mag=mag)


def stage_bounds(case):
    return dict(k=bound_of(APG_SLOPE_C if case.apg else SLOPE_C), acc=bound_of(STATE_C))


def stage_yard(case, o, ref=None):
    """The fp32 CPU evaluation of the same formula under the same metric (a ceiling check for the counts: never part of the bound)."""
    ref = ref or stage_eval(case, o)
    y = stage_eval(case, o, torch.float32)
    return dict(k=parity_err(y["k"], ref["k"], ref["K"])[0], acc=parity_err(y["acc"], ref["acc"], ref["mag"])[0])


def _stage_args(case, o, d, n, r0):
    a = rt.vv_ode_stage_args()
    a.x, a.pred, a.ldp, a.Rc, a.n_mel, a.n_prev = ptr(d["x"]), ptr(d["pred"]), case.ldp, n, case.n_mel, case.stage
    for j in range(3):
        a.k_prev[j] = ptr(d["k_prev"][j]) if j < case.stage and case.coef[j] != 0 else None        # a zero coefficient: no buffer at all
    for j, c in enumerate(case.coef):
        a.coef[j] = float(c)
    a.k_out, a.x_out = ptr(d["k_out"]), ptr(d["x_out"])
    a.g, a.g_item, a.seq_n, a.row_src = case.g, ptr(d["g_item"]), case.N, ptr(d["row_src"])
    return a


def stage_launch(eng, case, o, rows=None, u_row="case", apg="case", xdev=None):
    """One launch -> dict(x, k, x_out) on the CPU.  rows = (r0, r1): only those packed rows, as a launch of its own (plain / Euler forms:
    the unconditional half is cut out with them).  u_row / apg: override the case's tables (bit-equality checks).  xdev: a framed x that
    stays on the device across the launches of a sliced run (x is then not copied back: the caller reads it once at the end)."""
    Rc, M = case.Rc, case.n_mel
    r0, r1 = rows or (0, Rc)
    n = r1 - r0
    assert rows is None or not case.guided
    keep = []
    xw, dx = xdev or framed(o.x)
    if rows is not None and not case.rows:
        dx_l = dx[r0:r1]
    else:
        dx_l = dx
    u = o.u_row if isinstance(u_row, str) else u_row
    if rows is None:
        pred = o.pred
    else:
        pred = torch.cat([o.pred[r0:r1], o.pred[Rc + r0:Rc + r1]])
    pw, dp = framed(pred)
    nan_row = pred.shape[0]                                        # the first guard row behind pred
    d = dict(x=dx_l, pred=dp, g_item=None, row_src=None, k_prev=[], k_out=None, x_out=None)
    if case.rows:
        unnamed = int((~torch.isfinite(o.x[:, 0])).nonzero()[0]) if bool((~torch.isfinite(o.x[:, 0])).any()) else 0
        tw, d["row_src"] = table(o.row_src[r0:r1], unnamed)
        keep.append(tw)
    if o.g_item is not None:
        gw, d["g_item"] = framed(o.g_item, 0, 8)
        keep.append(gw)
    for j in range(case.stage if not case.euler else 0):
        kw, kv = framed(o.k_prev[j][r0:r1])
        keep.append(kw)
        d["k_prev"].append(kv)
    du = None
    if u is not None:
        uw, du = table(u, nan_row)
        keep.append(uw)
    st = stream()
    outs = {}
    if case.euler:
        fn = eng.lib.vv_cfg_euler_rows if case.inst == "euler_rows" else eng.lib.vv_cfg_euler
        extra = (ptr(d["row_src"]),) if case.inst == "euler_rows" else ()
        check(eng, fn(eng.ctx, ptr(dx_l), ptr(dp), case.ldp, n, M, case.g, case.h, *extra, st))
    else:
        kb, d["k_out"], kg = out_rows(n, M)
        outs["k"] = (kb, d["k_out"], kg)
        if not case.last:
            xb, d["x_out"], xg = out_rows(n, M)
            outs["x_out"] = (xb, d["x_out"], xg)
        a = _stage_args(case, o, d, n, r0)
        ap = None
        spec = (o.apg_coef, o.x_e, o.xe_packed, o.t_e) if (apg == "case" and case.apg) else (None if isinstance(apg, str) else apg)
        if spec is not None:
            cw, dc = framed(spec[0], 0, 4)
            xe_dev = dx if spec[1] is None else framed(spec[1])[1]
            keep += [cw, xe_dev]
            ap = rt.vv_apg_stage_args()
            ap.coef, ap.x_e, ap.x_e_packed, ap.t_e = ptr(dc), ptr(xe_dev), int(spec[2]), float(spec[3])
        if ap is not None:
            rc = eng.lib.vv_ode_stage_apg(eng.ctx, C.byref(a), ptr(du), C.byref(ap), st)
        elif du is not None:
            rc = eng.lib.vv_ode_stage_guided(eng.ctx, C.byref(a), ptr(du), st)
        else:
            rc = eng.lib.vv_ode_stage(eng.ctx, C.byref(a), st)
        check(eng, rc)
    torch.cuda.synchronize()
    frame_intact(xw, dx, case.name + ": x")
    frame_intact(pw, dp, case.name + ": pred")
    res = dict(x=None if xdev else dx.cpu(), k=None, x_out=None)
    for key, (whole, view, guard) in outs.items():
        _bands_intact(whole, guard, FILL, f"{case.name}: {key}")
        res[key] = view.cpu()
    return res


def stage_cases():
    """Every stage of every method x the four instantiations, walking the shape, row-count, strength and u_row lists (coprime lengths, so
    every shape meets every row count), then both Euler forms on every shape, then the wrap cases."""
    cases, i = [], 0
    for inst in ("plain", "guided", "apg", "apg_guided"):
        for m, s in method_stages():
            (M, ldp), Rc = STAGE_SHAPES[i % 8], (1, 3, 86)[i % 3]
            per_item = i % 2 == 1
            g = STAGE_G[(i // 2) % 3]
            u_map = U_MAPS[(i // 3) % 4] if inst.endswith("guided") else "all"
            rows = s == 0 or i % 4 != 2                                  # stage 0 reads x through row_src in the stage driver; later ones either way
            cases.append(StageCase(f"stage/{inst}/{m}{s}/M{M}_ld{ldp}_Rc{Rc}" + ("_item" if per_item else f"_g{g}") +
                                   (f"_{u_map}" if inst.endswith("guided") else "") + ("" if rows else "_norows"),
                                   inst, M, ldp, Rc, m, s, g, per_item, rows, u_map, False, 3000 + i))
            i += 1
    for inst in ("euler", "euler_rows"):
        for j, (M, ldp) in enumerate(STAGE_SHAPES):
            Rc, g = (1, 3, 86)[j % 3], STAGE_G[(j + (inst == "euler")) % 3]
            cases.append(StageCase(f"{inst}/M{M}_ld{ldp}_Rc{Rc}_g{g}", inst, M, ldp, Rc, g=g, rows=inst == "euler_rows", seed=3200 + j))
    cases.append(StageCase("stage/plain/rk41/wrap_Rc21000", "plain", 100, 100, 21000, "rk4", 1, 2.0, True, True, seed=3300))
    cases.append(StageCase("euler_rows/wrap_Rc21000", "euler_rows", 100, 104, 21000, g=2.0, seed=3301))
    return cases


# ================================================================================================ apg_reduce / apg_coef
# Partials: float64 on the device.  Thread q % 256 takes its float4s serially (4 elements each, one fma per sum), then an 8-level tree:
# a partial is a sum whose longest chain is 4 ceil(total / 256) + 8 additions, each <= 2^-53 of the sum of |terms|, plus the roundings of
# a term itself (D is exact or one rounding, d one fma rounding, carried into the product): 2 more.  The reference sums in extended
# precision (numpy longdouble, eps 2^-64 on x86), so its own error is three orders below the bound.
@dataclasses.dataclass
class ApgCase:
    name: str
    lens: tuple
    n_mel: int = 100
    ldp: int = 104
    guided: tuple = None        # per item; None: u_row NULL (every item guided, p_u at Rc + r)
    t_e: float = 0.3
    eta: tuple = None
    norm: tuple = None
    g_item: tuple = None
    zero_d: bool = False        # x_e = 0 and t_e = 1: d == 0, S2 == 0
    rows: bool = True
    seed: int = 0
    extra_tiles: int = 0        # n_tiles beyond what the longest item needs: partials nobody writes
    overstate: int = 0          # the DEVICE len of the last item says this many rows more than the Rc rows hold: the kernels clamp it

    @property
    def B(self):
        return len(self.lens)

    @property
    def Rc(self):
        return sum(self.lens)

    @property
    def N(self):
        return max(self.lens) + 2

    @property
    def n_tiles(self):
        return -(-max(self.lens) // APG_TILE) + self.extra_tiles

    @property
    def lens_dev(self):
        return tuple(self.lens[:-1]) + (self.lens[-1] + self.overstate,)

    def ops(self):
        g = _gen(self.seed)
        o = type("Ops", (), {})()
        B, N, M, Rc = self.B, self.N, self.n_mel, self.Rc
        o.row_start = torch.tensor([sum(self.lens[:b]) for b in range(B)], dtype=I32)
        o.row_src = torch.cat([b * N + torch.arange(n) for b, n in enumerate(self.lens)]).to(I32)
        o.item = o.row_src.long() // N
        guided = torch.tensor(self.guided if self.guided is not None else [True] * B)
        mapped = guided[o.item]
        o.Ru = int(mapped.sum()) if self.guided is not None else Rc
        o.u_row = None
        if self.guided is not None:
            o.u_row = torch.full((Rc,), -1, dtype=I32)
            o.u_row[mapped] = Rc + torch.arange(o.Ru, dtype=I32)
        o.pred = torch.randn(Rc + o.Ru, self.ldp, generator=g)
        o.pred[:, M:] = NAN
        if self.rows:
            o.x_e = torch.randn(B * N, M, generator=g)
            named = torch.zeros(B * N, dtype=torch.bool)
            named[o.row_src.long()] = True
            o.x_e[~named] = NAN
        else:
            o.x_e = torch.randn(Rc, M, generator=g)
        if self.zero_d:
            o.x_e[torch.isfinite(o.x_e)] = 0.0
        o.eta = torch.tensor(self.eta if self.eta is not None else [0.0] * B, dtype=torch.float32)
        o.norm = torch.tensor(self.norm if self.norm is not None else [0.0] * B, dtype=torch.float32)
        o.g_item = torch.tensor(self.g_item if self.g_item is not None else [2.0] * B, dtype=torch.float32)
        return o


APG_MUTATIONS = ("drop_tile_last_frame", "S1_over_S3", "cap_without_omt")


def apg_ref(case, o, mut=None):
    """-> partials [B][n_tiles][3] (float64 of the extended-precision sums; NaN where nothing is written), their scales, the chain length per
    tile, coef [B][2] in float64 and the absolute float64 share of its bound."""
    B, M, Rc, nt = case.B, case.n_mel, case.Rc, case.n_tiles
    ld = np.longdouble
    omt = 1.0 - float(np.float32(case.t_e))
    part = np.full((B, nt, 3), np.nan)
    scale = np.ones((B, nt, 3))
    chain = np.zeros((B, nt))
    coef = np.zeros((B, 2))
    slack = np.zeros((B, 2))
    pred, xe = o.pred.numpy().astype(np.float64), o.x_e.numpy().astype(np.float64)
    for b in range(B):
        r0, n = int(o.row_start[b]), case.lens[b]
        guided = n > 0 and (o.u_row is None or int(o.u_row[r0]) >= 0)
        S, T = np.zeros(3, dtype=ld), np.zeros(3, dtype=ld)
        for tl in range(-(-n // APG_TILE)):
            f0, f1 = tl * APG_TILE, min((tl + 1) * APG_TILE, n)
            chain[b, tl] = 4 * -(-((f1 - f0) * (M // 4)) // 256) + 8 + 2
            rows = np.arange(r0 + f0, r0 + f1)
            if mut == "drop_tile_last_frame" and f1 - f0 > 0:
                rows = rows[:-1]
            ur = (rows + Rc) if o.u_row is None else o.u_row.numpy()[rows]
            rows, ur = rows[ur >= 0], ur[ur >= 0]
            pc, pu = pred[rows, :M].astype(ld), pred[ur, :M].astype(ld)
            x = xe[o.row_src.numpy()[rows] if case.rows else rows].astype(ld)
            D, d = pc - pu, x + ld(omt) * pc
            terms = [D * d, d * d, D * D]
            s = np.array([t.sum() for t in terms], dtype=ld)
            a = np.array([np.abs(t).sum() for t in terms], dtype=ld)
            part[b, tl] = s.astype(np.float64)
            scale[b, tl] = np.maximum(a.astype(np.float64), 1e-300)
            S, T = S + s, T + a
        if not guided:
            continue
        S1, S2, S3 = (float(v) for v in S)
        gb, e, r = float(o.g_item[b]), float(o.eta[b]), float(o.norm[b])
        rms = (1.0 if mut == "cap_without_omt" else omt) * math.sqrt(S3 / (n * M))
        sc = r / rms if (r > 0.0 and rms > r) else 1.0
        den = S3 if mut == "S1_over_S3" else S2
        coef[b] = gb * sc, (0.0 if (e == 1.0 or S2 == 0.0) else gb * sc * (e - 1.0) * S1 / den)
        # float64 share: the chain of the longest tile plus the tiles' serial sum on S1 (absolute, it may cancel), S2, S3 (relative), and a
        # handful of float64 roundings of the formula itself
        gam = (float(chain[b].max()) + nt + 8) * EPS53
        rel = gam / 2 + 8 * EPS53
        slack[b, 0] = abs(coef[b, 0]) * rel
        if coef[b, 1] != 0.0:
            slack[b, 1] = abs(gb * sc * (e - 1.0)) / S2 * gam * float(T[0]) + abs(coef[b, 1]) * (gam + rel)
    return dict(part=torch.from_numpy(part), scale=torch.from_numpy(scale), chain=torch.from_numpy(chain), coef=torch.from_numpy(coef),
                slack=torch.from_numpy(slack))


def apg_launch(eng, case, o):
    B, nt = case.B, case.n_tiles
    pw, dp = framed(o.pred)
    xw, dxe = framed(o.x_e)
    nan_x = int((~torch.isfinite(o.x_e[:, 0])).nonzero()[0]) if case.rows else 0
    keep = [table(o.row_start, 0), table(torch.tensor(case.lens_dev), 0), table(o.row_src, nan_x)]
    du = table(o.u_row, o.pred.shape[0])[1] if o.u_row is not None else None
    fl = [framed(v, 0, 4)[1] for v in (o.g_item, o.eta, o.norm)]
    parts_w, parts = _guarded((B, nt, 3), 6, FILL, init=torch.full((B, nt, 3), FILL, dtype=torch.float64), dtype=torch.float64)
    coef_w, coef = _guarded((B, 2), 4, FILL, init=torch.full((B, 2), FILL))
    a = rt.vv_apg_coef_args()
    a.pred, a.ldp, a.Rc, a.n_mel, a.u_row = ptr(dp), case.ldp, case.Rc, case.n_mel, ptr(du)
    a.x_e, a.row_src, a.B, a.n_tiles = ptr(dxe), ptr(keep[2][1]) if case.rows else None, B, nt
    a.row_start, a.len, a.t_e, a.g = ptr(keep[0][1]), ptr(keep[1][1]), case.t_e, 9.0
    a.g_item, a.eta, a.norm_rms, a.partials, a.coef = ptr(fl[0]), ptr(fl[1]), ptr(fl[2]), ptr(parts), ptr(coef)
    check(eng, eng.lib.vv_apg_coef(eng.ctx, C.byref(a), stream()))
    torch.cuda.synchronize()
    _bands_intact(parts_w, 6, FILL, case.name + ": partials")
    _bands_intact(coef_w, 4, FILL, case.name + ": coef")
    frame_intact(pw, dp, case.name + ": pred")
    frame_intact(xw, dxe, case.name + ": x_e")
    return dict(part=parts.cpu(), coef=coef.cpu())


def apg_cases():
    T = APG_TILE
    return [
        ApgCase("apg/tile_edges", (T - 1, T, T + 1, 1), eta=(0.0, 0.5, 0.25, 0.0), norm=(0.0, 0.3, 0.0, 0.1), g_item=(2.0, 1.5, 3.0, -0.5), seed=4000),
        ApgCase("apg/unguided_between", (T + 1, 5, 2 * T + 3), guided=(True, False, True), eta=(0.0, 0.0, 0.5), norm=(0.0, 0.0, 0.0), seed=4001),
        ApgCase("apg/eta_one_and_caps", (7, 9, 11), eta=(1.0, 0.0, 0.0), norm=(0.0, 0.05, 50.0), seed=4002),      # eta == 1; a cap that binds; one that does not
        ApgCase("apg/S2_zero", (3, T), t_e=1.0, zero_d=True, eta=(0.0, 0.5), seed=4003),
        ApgCase("apg/n_mel4_packed", (1, T + 1), n_mel=4, ldp=4, rows=False, eta=(0.0, 0.5), norm=(0.2, 0.0), seed=4004),
        # an empty item among lengths round a tile, one item unguided, a tile of partials nobody owns, a device len that overstates Rc
        ApgCase("apg/lens_0_31_32_33_45", (0, T - 1, T, T + 1, T + 13), guided=(True, True, False, True, True), eta=(0.0, 0.5, 0.0, 0.25, 0.5),
                norm=(0.0, 0.3, 0.0, 0.0, 0.1), extra_tiles=1, overstate=7, seed=4005),
        ApgCase("apg/lens_0_31_32_33_45_n_mel4", (0, T - 1, T, T + 1, T + 13), n_mel=4, ldp=8, eta=(0.0, 0.5, 0.0, 0.25, 0.5), extra_tiles=1, overstate=7,
                seed=4006),
    ]


# ================================================================================================ pack_cat / pack_cat_guided
@dataclasses.dataclass
class PackCase:
    name: str
    guided: bool
    n_mel: int
    cond_dim: int
    ldo: int
    lens: tuple
    N: int
    flags: tuple = None         # guided: which items have unconditional rows
    window: tuple = None        # guided: (row0, n_rows); None = every row
    x_packed: bool = False
    rows: bool = True           # pack_cat: row_src given
    seed: int = 0

    @property
    def Rc(self):
        return sum(self.lens)

    @property
    def B(self):
        return len(self.lens)

    def ops(self):
        g = _gen(self.seed)
        o = type("Ops", (), {})()
        B, N, M, CD, Rc = self.B, self.N, self.n_mel, self.cond_dim, self.Rc
        o.row_src = torch.cat([b * N + torch.arange(n) for b, n in enumerate(self.lens)]).to(I32)
        named = torch.zeros(B * N, dtype=torch.bool)
        named[o.row_src.long()] = True
        if not self.rows:
            named[:] = False
            named[:Rc] = True                                          # pack_cat without row_src: rows [0, BN) of the padded inputs
        o.xp = torch.randn(B * N, M, generator=g)
        o.cat = torch.randn(B * N, CD, generator=g)
        o.cat_drop = torch.randn(B * N, CD, generator=g)
        for t in (o.xp, o.cat, o.cat_drop):
            t[~named] = NAN                                            # source rows nobody names
        o.xs = torch.randn(Rc, M, generator=g)                         # the packed stage state
        if self.guided:
            rows = [(b, t) for b, n in enumerate(self.lens) for t in range(n) if self.flags[b]]
            starts = [sum(self.lens[:b]) for b in range(B)]
            o.u_src = torch.tensor([b * N + t for b, t in rows], dtype=I32)
            o.u_crow = torch.tensor([starts[b] + t for b, t in rows], dtype=I32)
            o.Ru = len(rows)
        return o


PACK_MUTATIONS = ("cat_for_drop", "crow_for_src", "pad_unwritten", "only_x_wide")


def pack_mut_applies(case, mut, only_x, dtype):
    if mut == "cat_for_drop":
        return "only the state columns are written" if only_x else (None if (not case.guided or case._window_has_unc()) else "no unconditional row in the window")
    if mut == "crow_for_src":
        if not case.guided or not case._window_has_unc():
            return "no unconditional row through u_src"
        return "the packed state is read through u_crow either way" if (only_x and case.x_packed) else None
    if mut == "pad_unwritten":
        return None if (not only_x and case.ldo > case.n_mel + case.cond_dim) else "no padding column is written"
    if mut == "only_x_wide":
        return None if only_x else "every column is written anyway"
    raise KeyError(mut)


def _window_has_unc(self):
    row0, n = self.window or (0, self.Rc + sum(l for l, f in zip(self.lens, self.flags) if f))
    return row0 + n > self.Rc


PackCase._window_has_unc = _window_has_unc


def pack_ref(case, o, only_x, dtype, mut=None):
    """-> (the whole [rows][ldo] buffer after the launch, started from 7.0; first row written; rows written): the gather written in torch,
    rounded to nearest even when bf16."""
    M, CD, ldo, Rc = case.n_mel, case.cond_dim, case.ldo, case.Rc
    x = o.xs if case.x_packed else o.xp
    if case.guided:
        total = Rc + o.Ru
        row0, n = case.window or (0, total)
        src = torch.cat([o.row_src, o.u_crow if mut == "crow_for_src" else o.u_src]).long()
        xrow = torch.cat([torch.arange(Rc), o.u_crow.long()]) if case.x_packed else src
        unc = torch.arange(total) >= Rc
    else:
        total, row0, n = 2 * Rc, 0, 2 * Rc
        base = o.row_src.long() if case.rows else torch.arange(Rc)
        src = torch.cat([base, base])
        xrow = torch.arange(Rc).repeat(2) if case.x_packed else src
        unc = torch.arange(total) >= Rc
    full = torch.zeros(total, ldo)
    full[:, :M] = x[xrow]
    if CD:
        drop = o.cat if mut == "cat_for_drop" else o.cat_drop
        full[:, M:M + CD] = torch.where(unc[:, None], drop[src], o.cat[src])
    out = torch.full((total, ldo), FILL)
    width = (M + 4 if mut == "only_x_wide" else M) if only_x else (M + CD if mut == "pad_unwritten" else ldo)
    out[row0:row0 + n, :width] = full[row0:row0 + n, :width]
    return out.to(dtype), row0, n


def pack_launch(eng, case, o, only_x, dtype):
    M, CD, ldo, Rc = case.n_mel, case.cond_dim, case.ldo, case.Rc
    total = Rc + o.Ru if case.guided else 2 * Rc
    x = o.xs if case.x_packed else o.xp
    frames = [framed(t) for t in (x, o.cat, o.cat_drop)]
    (xw, dx), (cw, dc), (dw, dd) = frames
    whole, view, guard = out_rows(total, ldo, dtype)
    nan_row = int((~torch.isfinite(o.xp[:, 0])).nonzero()[0]) if bool((~torch.isfinite(o.xp[:, 0])).any()) else 0
    code = rt.VV_BF16 if dtype == torch.bfloat16 else rt.VV_F32
    keep = [table(o.row_src, nan_row)]
    if case.guided:
        row0, n = case.window or (0, total)
        keep += [table(o.u_src, nan_row), table(o.u_crow, 0)]
        rc = eng.lib.vv_pack_cat_guided(eng.ctx, code, ptr(dx), ptr(dc), ptr(dd), ptr(view), ldo, Rc, row0, n, M, CD, int(only_x), int(case.x_packed),
                                        ptr(keep[0][1]), ptr(keep[1][1]), ptr(keep[2][1]), stream())
    else:
        rs = keep[0][1] if (case.rows and not case.x_packed) else None
        rc = eng.lib.vv_pack_cat(eng.ctx, code, ptr(dx), ptr(dc), ptr(dd), ptr(view), ldo, Rc, M, CD, int(only_x), ptr(rs), stream())
    check(eng, rc)
    torch.cuda.synchronize()
    _bands_intact(whole, guard, FILL, case.name)
    for (w, v), what in zip(frames, ("x", "cat", "cat_drop")):
        frame_intact(w, v, f"{case.name}: {what}")
    return dict(out=view.cpu())


def pack_cases():
    return [
        PackCase("pack/rows_tight", False, 100, 28, 128, (5, 1, 3), 6, seed=5000),
        PackCase("pack/rows_padded", False, 4, 8, 32, (2, 3), 4, seed=5001),
        PackCase("pack/norows", False, 100, 28, 160, (4, 4), 4, rows=False, seed=5002),
        PackCase("pack/state_packed", False, 100, 28, 128, (5, 1, 3), 6, x_packed=True, rows=False, seed=5003),      # row_src NULL: the stage state
        PackCase("pack/wrap", False, 100, 412, 512, (1100, 1000), 1100, seed=5004),                   # 2 x 2100 x 128 float4s > 524288
        PackCase("pack_guided/all", True, 100, 28, 128, (5, 1, 3), 6, flags=(1, 1, 1), seed=5010),
        PackCase("pack_guided/middle_window", True, 100, 28, 160, (5, 1, 3), 6, flags=(0, 1, 1), window=(7, 6), seed=5011),   # rows 7, 8 conditional, 9..12 unconditional
        PackCase("pack_guided/packed_state", True, 4, 8, 12, (2, 3, 2), 4, flags=(0, 1, 1), x_packed=True, seed=5012),
        PackCase("pack_guided/cond_only_window", True, 100, 28, 128, (5, 1, 3), 6, flags=(1, 0, 0), window=(2, 5), seed=5013),
        PackCase("pack_guided/wrap", True, 100, 412, 512, (2100, 2100), 2100, flags=(1, 0), seed=5014),     # 6300 x 128 float4s
    ]


def pack_total(case, only_x=False):
    rows = case.Rc + sum(l for l, f in zip(case.lens, case.flags) if f) if case.guided else 2 * case.Rc
    if case.guided and case.window:
        rows = case.window[1]
    return rows * ((case.n_mel if only_x else case.ldo) // 4)


# ================================================================================================ row_tables / guided_tables / lengths
SENTINEL = -77


@dataclasses.dataclass
class TableCase:
    name: str
    seq_len: tuple              # the DEVICE lengths
    N: int
    Rc: int                     # the host's count of conditional rows
    flags: tuple = None
    Ru: int = 0


def tables_restated(case, mut=None):
    """The contract of row_tables_kernel / guided_tables_kernel as documented above them, in prefix sums.  -> dict of int lists; entries the
    contract leaves unwritten hold SENTINEL."""
    B, N, Rc = len(case.seq_len), case.N, case.Rc
    cl = [min(max(v, 0), N) for v in case.seq_len]
    S = SENTINEL
    t = dict(row_start=[S] * (2 * B), kv_len=[S] * (2 * B), row_src=[S] * Rc, row_pos=[S] * (2 * Rc))
    r0 = 0
    ends = []
    for b in range(B):
        pre = sum(case.seq_len[:b]) if mut == "prefix_unclamped" else sum(cl[:b])
        r0 = min(max(pre, 0), Rc)
        ln = min(cl[b], Rc - r0)
        t["row_start"][b], t["row_start"][B + b], t["kv_len"][b], t["kv_len"][B + b] = r0, Rc + r0, ln, ln
        for q in range(ln):
            t["row_src"][r0 + q] = b * N + q
            t["row_pos"][r0 + q] = t["row_pos"][Rc + r0 + q] = q
        ends.append((r0, ln))
    r0, ln = ends[-1]
    for r in range(r0 + ln, Rc):
        p = min(ln + (r - (r0 + ln)), N - 1)
        t["row_src"][r] = (B - 1) * N + p
        t["row_pos"][r] = t["row_pos"][Rc + r] = p
    return t


def tables_brute(case):
    """The same tables by walking the rows one at a time."""
    B, N, Rc = len(case.seq_len), case.N, case.Rc
    S = SENTINEL
    t = dict(row_start=[S] * (2 * B), kv_len=[0] * (2 * B), row_src=[S] * Rc, row_pos=[S] * (2 * Rc))
    r = 0
    for b in range(B):
        t["row_start"][b], t["row_start"][B + b] = r, Rc + r
        q = 0
        while q < case.seq_len[b] and q < N and r < Rc:
            t["row_src"][r], t["row_pos"][r], t["row_pos"][Rc + r] = b * N + q, q, q
            q, r = q + 1, r + 1
        t["kv_len"][b] = t["kv_len"][B + b] = q
    q = t["kv_len"][B - 1]
    while r < Rc:                                                     # orphan rows: the last item's padding rows
        p = min(q, N - 1)
        t["row_src"][r], t["row_pos"][r], t["row_pos"][Rc + r] = (B - 1) * N + p, p, p
        q, r = q + 1, r + 1
    return t


GUIDED_MUTATIONS = ("prefix_unclamped", "flag_bit_b_plus_1", "orphan_u_row_kept")


def guided_restated(case, mut=None):
    B, N, Rc, Ru = len(case.seq_len), case.N, case.Rc, case.Ru
    S = SENTINEL
    nb = sum(1 for f in case.flags if f)
    t = dict(row_start=[S] * (2 * B), rs_rel=[S] * B, kv_len=[S] * (2 * B), row_pos=[S] * (Rc + Ru), u_src=[S] * Ru, u_crow=[S] * Ru, u_row=[S] * Rc)
    flag = lambda b: bool(case.flags[b + 1] if b + 1 < B else 0) if mut == "flag_bit_b_plus_1" else bool(case.flags[b])
    r0 = u0 = j = 0
    for b in range(B):
        if mut == "prefix_unclamped":
            r0 = min(max(sum(case.seq_len[:b]), 0), Rc)
        ln = min(min(max(case.seq_len[b], 0), N), Rc - r0)
        ul = min(ln, Ru - u0) if flag(b) else 0
        t["row_start"][b], t["kv_len"][b] = r0, ln
        if flag(b):
            t["row_start"][B + j], t["rs_rel"][j], t["kv_len"][B + j] = Rc + u0, u0, ul
        for q in range(ln):
            t["row_pos"][r0 + q] = q
            t["u_row"][r0 + q] = Rc + u0 + q if q < ul else -1
        for q in range(ul):
            t["row_pos"][Rc + u0 + q], t["u_src"][u0 + q], t["u_crow"][u0 + q] = q, b * N + q, r0 + q
        if b == B - 1:
            for r in range(r0 + ln, Rc):
                t["row_pos"][r] = min(ln + (r - (r0 + ln)), N - 1)
                if mut != "orphan_u_row_kept":
                    t["u_row"][r] = -1
            for u in range(u0 + ul, Ru):
                p = min(ln + (u - (u0 + ul)), N - 1)
                t["row_pos"][Rc + u], t["u_src"][u], t["u_crow"][u] = p, b * N + p, Rc - 1
        r0, u0, j = r0 + ln, u0 + ul, j + (1 if flag(b) else 0)
    return t


def guided_brute(case):
    """Row by row: conditional rows as in tables_brute; an unconditional row for each conditional row of a flagged item while rows remain."""
    B, N, Rc, Ru = len(case.seq_len), case.N, case.Rc, case.Ru
    S = SENTINEL
    t = dict(row_start=[S] * (2 * B), rs_rel=[S] * B, kv_len=[S] * (2 * B), row_pos=[S] * (Rc + Ru), u_src=[S] * Ru, u_crow=[S] * Ru, u_row=[S] * Rc)
    r = u = j = 0
    q = 0
    for b in range(B):
        t["row_start"][b] = r
        if case.flags[b]:
            t["row_start"][B + j], t["rs_rel"][j] = Rc + u, u
        q = nu = 0
        while q < case.seq_len[b] and q < N and r < Rc:
            t["row_pos"][r] = q
            t["u_row"][r] = -1
            if case.flags[b] and u < Ru:
                t["u_row"][r], t["row_pos"][Rc + u], t["u_src"][u], t["u_crow"][u] = Rc + u, q, b * N + q, r
                u, nu = u + 1, nu + 1
            q, r = q + 1, r + 1
        t["kv_len"][b] = q
        if case.flags[b]:
            t["kv_len"][B + j] = nu
            j += 1
    k = q
    while r < Rc:
        t["row_pos"][r], t["u_row"][r] = min(k, N - 1), -1
        k, r = k + 1, r + 1
    k = q
    while u < Ru:
        p = min(k, N - 1)
        t["row_pos"][Rc + u], t["u_src"][u], t["u_crow"][u] = p, (B - 1) * N + p, Rc - 1
        k, u = k + 1, u + 1
    return t


def table_ranges(case, t):
    """Every written entry lies inside the buffer it indexes."""
    B, N, Rc = len(case.seq_len), case.N, case.Rc
    Ru = case.Ru if case.flags is not None else Rc
    lim = dict(row_start=(0, Rc + Ru), rs_rel=(0, Ru), kv_len=(0, N), row_pos=(0, N - 1), row_src=(0, B * N - 1), u_src=(0, B * N - 1),
               u_crow=(0, Rc - 1), u_row=(-1, Rc + Ru - 1))
    for k, vals in t.items():
        for v in vals:
            if v != SENTINEL:
                assert lim[k][0] <= v <= lim[k][1], (case.name, k, v, lim[k])


def tables_launch(eng, case):
    B, N, Rc = len(case.seq_len), case.N, case.Rc
    guided = case.flags is not None
    sl = table(torch.tensor(case.seq_len), 10 ** 6)
    sizes = dict(row_start=2 * B, rs_rel=B, kv_len=2 * B, row_pos=Rc + case.Ru, u_src=case.Ru, u_crow=case.Ru, u_row=Rc) if guided else \
        dict(row_start=2 * B, row_src=Rc, row_pos=2 * Rc, kv_len=2 * B)
    bufs = {k: torch.full((n + 16,), SENTINEL, dtype=I32, device=DEV) for k, n in sizes.items()}
    p = {k: v[8:].data_ptr() for k, v in bufs.items()}
    if guided:
        flags = (C.c_uint8 * B)(*[int(bool(f)) for f in case.flags])
        rc = eng.lib.vv_guided_tables(eng.ctx, ptr(sl[1]), C.cast(flags, C.c_void_p), B, N, Rc, case.Ru, p["row_start"], p["rs_rel"], p["kv_len"],
                                      p["row_pos"], p["u_src"], p["u_crow"], p["u_row"], stream())
    else:
        rc = eng.lib.vv_row_tables(eng.ctx, ptr(sl[1]), B, N, Rc, p["row_start"], p["row_src"], p["row_pos"], p["kv_len"], stream())
    check(eng, rc)
    torch.cuda.synchronize()
    out = {}
    for k, n in sizes.items():
        v = bufs[k].cpu()
        assert bool((v[:8] == SENTINEL).all()) and bool((v[8 + n:] == SENTINEL).all()), f"{case.name}: the sentinels around {k} were written"
        out[k] = v[8:8 + n].clone()
    return out


def _flags(B, pattern):
    return tuple({"all": 1, "none": 0, "alt": b % 2, "alt1": (b + 1) % 2, "last": int(b == B - 1), "notlast": int(b != B - 1)}[pattern] for b in range(B))


def table_cases():
    """-> (row_tables cases, guided_tables cases).  The host's Rc / Ru are what the host lengths and flags give, unless the name says the
    device lengths disagree."""
    def lens(B, N, zero=()):
        return tuple(0 if b in zero else 1 + (b * 7) % N for b in range(B))

    plain, guided = [], []
    for B in (1, 3, 33, 65):
        N = 9
        sl = lens(B, N)
        plain.append(TableCase(f"tables/B{B}", sl, N, sum(sl)))
        for pat in ("all", "alt", "last", "notlast"):
            fl = _flags(B, pat)
            guided.append(TableCase(f"guided/B{B}_{pat}", sl, N, sum(sl), fl, sum(l for l, f in zip(sl, fl) if f)))
    for zero, tag in (((0,), "first"), ((4,), "last"), ((2,), "middle"), ((0, 1, 4), "three")):
        sl = lens(5, 9, zero)
        plain.append(TableCase(f"tables/zero_{tag}", sl, 9, sum(sl)))
        guided.append(TableCase(f"guided/zero_{tag}", sl, 9, sum(sl), (1, 0, 1, 1, 1), sum(l for l, f in zip(sl, (1, 0, 1, 1, 1)) if f)))
    odd = dict(more=((5, 9, 9, 4), 9, 14), fewer=((2, 1, 3), 9, 17), fewer_past_N=((2, 1, 8), 9, 24), negative=((4, -3, 6, -1), 9, 10),
               above_N=((40, 3, 17), 9, 21), all_zero=((0, 0, 0), 9, 4))
    for tag, (sl, N, Rc) in odd.items():
        plain.append(TableCase(f"tables/device_{tag}", sl, N, Rc))
        for pat in ("all", "alt", "alt1"):
            fl = _flags(len(sl), pat)
            hostu = min(Rc, sum(min(max(l, 0), N) for l, f in zip(sl, fl) if f))
            for Ru, ru_tag in ((0, "Ru0"), (Rc, "RuRc"), (max(hostu - 2, 0), "cut"), (min(hostu + 2, Rc), "spare")):
                guided.append(TableCase(f"guided/device_{tag}_{pat}_{ru_tag}", sl, N, Rc, fl, Ru))
    return plain, guided


@dataclasses.dataclass
class LenCase:
    name: str
    B: int
    N: int
    T_max: int
    hop: int = 256
    mult: tuple = (1, 8, 64, 256)

    def ops(self):
        g = _gen(self.B * 31 + self.N)
        o = type("Ops", (), {})()
        B, N = self.B, self.N
        o.seq_len = torch.randint(-3, N + 6, (B,), generator=g).to(I32)
        o.ref_len = torch.randint(-3, N + 6, (B,), generator=g).to(I32)
        edge = [(N, 0), (N, N), (N + 5, 0), (N + 5, N + 1), (0, 0), (-2, -2), (5, -1), (N, N - 1), (N, N - self.T_max), (N, N - self.T_max - 1)]
        for b, (s, r) in enumerate(edge[:B]):
            o.seq_len[b], o.ref_len[b] = s, r
        o.audio_len = torch.randint(0, 50000, (B,), generator=g).to(I32)
        o.audio_len[0] = self.hop - 1
        if B > 1:
            o.audio_len[1] = self.hop
        return o


def gen_slice(seq_len, ref_len, N, T_max=None, mut=None):
    """(first row, frames) of an item's generated slice: both ends clamped into [0, min(seq_len, N)], the frames to T_max."""
    sl = max(seq_len if mut == "seq_unclamped" else min(seq_len, N), 0)
    rl = min(max(ref_len, 0), sl)
    tg = sl - rl
    if mut == "start_minus_1":
        rl -= 1
    return rl, (tg if T_max is None else min(tg, T_max))


def len_ref(case, o):
    B = case.B
    tg = [gen_slice(int(o.seq_len[b]), int(o.ref_len[b]), case.N, case.T_max)[1] for b in range(B)]
    return dict(ref_len=[int(a) // case.hop + 1 for a in o.audio_len], vocos=tg, decode=[[t * m for t in tg] for m in case.mult])


def len_launch(eng, case, o):
    B = case.B
    ins = {k: table(getattr(o, k), 10 ** 6) for k in ("seq_len", "ref_len", "audio_len")}
    mult = table(torch.tensor(case.mult), 10 ** 6)
    sizes = dict(ref_len=B, vocos=B, decode=len(case.mult) * B)
    bufs = {k: torch.full((n + 16,), SENTINEL, dtype=I32, device=DEV) for k, n in sizes.items()}
    p = {k: v[8:].data_ptr() for k, v in bufs.items()}
    st = stream()
    check(eng, eng.lib.vv_ref_len(eng.ctx, ptr(ins["audio_len"][1]), p["ref_len"], B, case.hop, st))
    check(eng, eng.lib.vv_vocos_lens(eng.ctx, ptr(ins["seq_len"][1]), ptr(ins["ref_len"][1]), p["vocos"], B, case.N, case.T_max, st))
    check(eng, eng.lib.vv_decode_len(eng.ctx, ptr(ins["seq_len"][1]), ptr(ins["ref_len"][1]), p["decode"], B, len(case.mult), ptr(mult[1]), case.N,
                                     case.T_max, st))
    torch.cuda.synchronize()
    out = {}
    for k, n in sizes.items():
        v = bufs[k].cpu()
        assert bool((v[:8] == SENTINEL).all()) and bool((v[8 + n:] == SENTINEL).all()), f"{case.name}: the sentinels around {k} were written"
        out[k] = v[8:8 + n].tolist()
    out["decode"] = [out["decode"][l * B:(l + 1) * B] for l in range(len(case.mult))]
    return out


def len_cases():
    return [LenCase(f"lens/B{B}", B, 40, 12) for B in (1, 10, 64, 65)]


# ================================================================================================ rope_compact / rope_rows
def rope_launch(eng, n, pos):
    """-> compact [n][64] from cos / sin tables [n][64], and rows [len(pos)][64] gathered from it; the references beside them."""
    g = _gen(6000 + n + len(pos))
    cos, sin = torch.randn(n, 64, generator=g), torch.randn(n, 64, generator=g)
    cw, dc = framed(cos)
    sw, ds = framed(sin)
    whole, comp, guard = out_rows(n, 64)
    check(eng, eng.lib.vv_rope_compact(eng.ctx, ptr(dc), ptr(ds), ptr(comp), n, stream()))
    want = torch.empty(n, 64)
    want[:, 0::2], want[:, 1::2] = cos[:, 0::2], sin[:, 0::2]
    rows = len(pos)
    tw, dt = framed(want)                                             # the gather reads the reference's compact table, not the device's
    pt = table(torch.tensor(pos), n)                                  # behind the table: the first NaN guard row
    whole2, out, guard2 = out_rows(rows, 64)
    check(eng, eng.lib.vv_rope_rows(eng.ctx, ptr(dt), ptr(pt[1]), ptr(out), rows, stream()))
    torch.cuda.synchronize()
    _bands_intact(whole, guard, FILL, "rope_compact")
    _bands_intact(whole2, guard2, FILL, "rope_rows")
    return dict(compact=comp.cpu(), rows=out.cpu()), dict(compact=want, rows=want[torch.tensor(pos)])


ROPE_SIZES = (1, 7, 8, 9)


def rope_positions(n, rows):
    """Out of order and repeated."""
    return [(n - 1 - 3 * r) % n if r % 3 else (5 * r) % n for r in range(rows)]


# ================================================================================================ mel_slice / vocos_im2col
@dataclasses.dataclass
class SliceCase:
    name: str
    n_mel: int
    T: int                      # mel_slice's T, im2col's T_max
    N: int
    seq_len: tuple
    ref_len: tuple
    k: int = 7
    ld_extra: int = 0

    @property
    def B(self):
        return len(self.seq_len)

    def ops(self):
        g = _gen(7000 + self.T * 13 + self.n_mel + self.N)
        o = type("Ops", (), {})()
        o.x = torch.randn(self.B * self.N, self.n_mel, generator=g)
        return o


SLICE_MUTATIONS = ("start_minus_1", "seq_unclamped", "no_tap_offset")
SLICE_FRONT = 48                # NaN guard rows around x: more than any wrong offset of these cases can reach


def slice_ref(case, o, mut=None):
    """-> dict(mel [B][n_mel][T], cols [B * T][k * n_mel + pad]); a row outside x reads the NaN guard rows."""
    B, N, M, T, k = case.B, case.N, case.n_mel, case.T, case.k
    pool = torch.cat([torch.full((SLICE_FRONT, M), NAN), o.x, torch.full((SLICE_FRONT, M), NAN)])
    row = lambda b, t: pool[SLICE_FRONT + b * N + t]
    mel = torch.zeros(B, M, T)
    ld = k * M + case.ld_extra
    cols = torch.zeros(B * T, ld)
    half = 0 if mut == "no_tap_offset" else k // 2
    for b in range(B):
        rl, tg = gen_slice(case.seq_len[b], case.ref_len[b], N, mut=mut)
        for t in range(min(tg, T)):
            mel[b, :, t] = row(b, rl + t)
        tgc = min(tg, T)
        for t in range(T):
            for j in range(k):
                tt = t + j - half
                if 0 <= tt < tgc:
                    cols[b * T + t, j * M:(j + 1) * M] = row(b, rl + tt)
    return dict(mel=mel, cols=cols)


def slice_ref_fast(case, o):
    """slice_ref without mutations, vectorised for the wrap case."""
    B, N, M, T, k = case.B, case.N, case.n_mel, case.T, case.k
    cols = torch.zeros(B, T, k * M + case.ld_extra)
    for b in range(B):
        rl, tg = gen_slice(case.seq_len[b], case.ref_len[b], N, T)
        seg = o.x[b * N + rl:b * N + rl + tg]
        for j in range(k):
            sh = j - k // 2                                            # cols[t] tap j = seg[t + sh]
            lo, hi = max(0, -sh), min(T, tg - sh)
            if hi > lo:
                cols[b, lo:hi, j * M:(j + 1) * M] = seg[lo + sh:hi + sh]
    return cols.reshape(B * T, -1)


def slice_launch(eng, case, o, which):
    B, N, M, T = case.B, case.N, case.n_mel, case.T
    xw, dx = framed(o.x, SLICE_FRONT, SLICE_FRONT)
    sl, rl = table(torch.tensor(case.seq_len), 10 ** 6), table(torch.tensor(case.ref_len), 10 ** 6)
    if which == "mel":
        whole, out = _guarded((B, M, T), 64, FILL, init=torch.full((B, M, T), FILL))
        check(eng, eng.lib.vv_mel_slice(eng.ctx, ptr(dx), B, N, M, ptr(rl[1]), ptr(sl[1]), ptr(out), T, stream()))
        guard = 64
    else:
        ld = case.k * M + case.ld_extra
        whole, out, guard = out_rows(B * T, ld)
        check(eng, vocos_im2col(eng, ptr(dx), B, N, M, ptr(rl[1]), ptr(sl[1]), T, case.k, ptr(out), ld))
    torch.cuda.synchronize()
    _bands_intact(whole, guard, FILL, case.name)
    frame_intact(xw, dx, case.name + ": x")
    return dict(out=out.cpu())


def vocos_im2col(eng, x, B, N, M, ref_len, seq_len, T_max, k, out, ld_out):
    """The context-free entry: n_mel and the tap count are arguments (vv_vocos_im2col takes them from a Vocos context)."""
    return eng.lib.vv_vocos_im2col_ex(eng.ctx, x, B, N, M, ref_len, seq_len, T_max, k, out, ld_out, stream())


def slice_cases(n_mels=(4, 100)):
    cases = []
    for M in n_mels:
        for T in (1, 31, 32, 33):
            N = T + 9
            # generated lengths 0, 1, T; ref_len 0 and > seq_len; seq_len > N; a negative ref_len (clamped: the item starts at row 0)
            # and seq_len > N with ref_len = N: nothing is generated, where the unclamped length would read the next item's rows
            seq = (5, 6, 5 + T, T, 4, N + 7, 3, T + 2, N + 3)
            ref = (5, 5, 5, 0, 9, 2, -2, -40, N)
            cases.append(SliceCase(f"slice/M{M}_T{T}", M, T, N, seq, ref, ld_extra=0 if T % 2 else 12))
    return cases


# ================================================================================================ vocos_spectrum
# No document shipped with the device library states the accuracy of expf / sincosf, so the bound is the yardstick's: 4 x the error of
# the CPU library's fp32 exp / sin / cos on the same operands under the same metric, over a floor of 3 x 2^-24: what correctly rounded
# functions leave (one rounding each of the magnitude, the sine and their product).  Below the smallest normal fp32 carries no relative
# accuracy (and a library may flush): an absolute 2^-126 is allowed per element.
SPECTRUM_FLOOR_C = 3.0
PHASES = (0.0, math.pi, 50.0, 1e4, 1e6, 1e8)
LOG_100 = math.log(100.0)


@dataclasses.dataclass
class SpecCase:
    name: str
    phase: float
    R: int = 6
    n: int = 16
    ld_extra: int = 6

    @property
    def ld(self):
        return self.n + 2 + self.ld_extra

    def ops(self):
        g = _gen(8000 + int(self.phase) % 1000 + self.R)
        o = type("Ops", (), {})()
        nb = self.n // 2 + 1
        head = torch.full((self.R, self.ld), NAN)
        head[:, :nb] = torch.randn(self.R, nb, generator=g) * 2.0
        below = float(np.nextafter(np.float32(LOG_100), np.float32(0)))
        above = float(np.nextafter(np.float32(LOG_100), np.float32(10)))
        special = torch.tensor([below, above, -100.0, 90.0, LOG_100, 0.0])
        for r in range(self.R):
            for i, v in enumerate(special):
                head[r, (r + i) % nb] = v                              # every special magnitude meets every kind of column, 0 and n/2 included
        ph = torch.full((self.R, nb), float(np.float32(self.phase)))
        ph[1::2] = -ph[1::2]
        if self.phase > 0:
            ph[2:] = ph[2:] * (1.0 + 0.25 * torch.rand(self.R - 2, nb, generator=g))     # rows 0, 1: +-phase itself; the rest spread above it
        else:
            ph[2:] = torch.randn(self.R - 2, nb, generator=g)
        head[:, nb:2 * nb] = ph
        o.head = head
        return o


SPEC_MUTATIONS = ("no_clip", "sine_at_n", "fast_sine")


def spec_eval(case, o, dtype=torch.float64, mut=None):
    """-> out [R * n + 1]: the plane and the element behind it (what a sine stored for column n/2 would hit), and the scale A_e = mag."""
    R, n = case.R, case.n
    h, nb = n // 2, n // 2 + 1
    lm, ph = o.head[:, :nb].to(dtype), o.head[:, nb:2 * nb].to(dtype)
    mag = torch.exp(lm)
    if mut != "no_clip":
        mag = mag.clamp_max(100.0)
    if mut == "fast_sine":                                             # the angle reduced in fp32 by a single-float 2 pi
        p32 = o.head[:, nb:2 * nb]
        two_pi = torch.tensor(2 * math.pi, dtype=torch.float32)
        ph = (p32 - torch.round(p32 / two_pi) * two_pi).to(dtype)
    c, s = mag * torch.cos(ph), mag * torch.sin(ph)
    out = torch.zeros(R * n + 1, dtype=dtype)
    A = torch.zeros(R * n + 1, dtype=torch.float64)
    plane, Ap = out[:R * n].view(R, n), A[:R * n].view(R, n)
    plane[:, :nb] = c
    plane[:, nb:] = s[:, 1:h]
    m64 = torch.exp(o.head[:, :nb].double()).clamp_max(100.0)
    Ap[:, :nb], Ap[:, nb:] = m64, m64[:, 1:h]
    if mut == "sine_at_n":
        for r in range(R):                                             # row r's sine of column n/2 lands on row r + 1's column 0
            out[(r + 1) * n] = s[r, h]
    A[R * n] = 1.0
    if mut != "sine_at_n":
        out[R * n] = FILL
    return out, A


def spec_launch(eng, case, o):
    hw, dh = framed(o.head)
    whole, out, guard = out_rows(case.R, case.n)
    check(eng, eng.lib.vv_vocos_spectrum(eng.ctx, ptr(dh), case.ld, case.R, case.n, ptr(out), stream()))
    torch.cuda.synchronize()
    _bands_intact(whole, guard, FILL, case.name)
    frame_intact(hw, dh, case.name + ": head")
    return dict(out=torch.cat([out.cpu().reshape(-1), torch.tensor([FILL])]))


def spec_cases():
    return [SpecCase(f"spectrum/phase_{p:g}", p) for p in PHASES] + [SpecCase("spectrum/wrap_R4100", 50.0, R=4100, n=1024, ld_extra=2)]


# ================================================================================================ vocos_ola
# Per sample, k = n_fft / hop frames overlap: k - 1 serial adds of the frames (each <= 2^-24 sum |frame|), k fused multiply-adds of the
# positive envelope (relative 2^-24 each), one division: c = 2 k + 1 on A_e = sum |frame| / env.
@dataclasses.dataclass
class OlaCase:
    name: str
    n: int
    hop: int
    T_max: int
    lens: tuple
    ld_f_extra: int = 4
    ld_extra: int = 3
    wave: bool = True
    seed: int = 0

    @property
    def B(self):
        return len(self.lens)

    @property
    def c(self):
        return 2.0 * (self.n // self.hop) + 1.0

    def ops(self):
        g = _gen(self.seed)
        o = type("Ops", (), {})()
        o.window = 0.2 + 0.8 * torch.rand(self.n, generator=g)
        o.frames = torch.full((self.B * self.T_max, self.n + self.ld_f_extra), NAN)
        o.frames[:, :self.n] = torch.randn(self.B * self.T_max, self.n, generator=g) * 0.4
        for b, L in enumerate(self.lens):                              # frames past an item's length are computed by the GEMM and never read
            o.frames[b * self.T_max + min(max(L, 0), self.T_max):(b + 1) * self.T_max] = NAN
        return o


OLA_MUTATIONS = ("env_sum_w", "t_lo_minus_1", "no_trim", "last_frame_out")


def ola_eval(case, o, dtype=torch.float64, mut=None, items=None):
    """-> y [B][T_max * hop], A, pcm_len [B].  Frames outside [0, T_b) read as NaN (they are NaN in the operand)."""
    n, hop, Tm = case.n, case.hop, case.T_max
    L = Tm * hop
    B = case.B
    y, A = torch.zeros(B, L, dtype=dtype), torch.ones(B, L, dtype=torch.float64)
    plen = []
    w = o.window.to(dtype)
    w64 = o.window.double()
    for b in (range(B) if items is None else items):
        T = min(max(case.lens[b], 0), Tm)
        plen.append(hop * max(T - 1, 0))
        fr = o.frames[b * Tm:(b + 1) * Tm, :n].to(dtype)
        for j in range(plen[-1]):
            i = j + (0 if mut == "no_trim" else n // 2)
            t_lo = ((i - n) // hop + 1 if i >= n else 0) - (1 if mut == "t_lo_minus_1" else 0)
            t_hi = min(i // hop, T - 1) - (1 if mut == "last_frame_out" else 0)
            acc = torch.zeros((), dtype=dtype)
            env = torch.zeros((), dtype=dtype)
            a = 0.0
            e64 = 0.0
            for t in range(t_lo, t_hi + 1):
                q = i - t * hop
                v = fr[t, q] if 0 <= t < Tm and 0 <= q < n else torch.tensor(NAN, dtype=dtype)
                wq = w[q] if 0 <= q < n else torch.tensor(NAN, dtype=dtype)
                acc = acc + v
                env = env + (wq if mut == "env_sum_w" else wq * wq)
                if 0 <= t < T and 0 <= q < n:
                    a += abs(float(fr[t, q].double()))
                    e64 += float(w64[q]) ** 2
            y[b, j] = acc / env
            A[b, j] = a / e64 if e64 > 0 else 1.0
    return y, A, plen


def pcm_of(wave, mut=None):
    """trunc(clamp(fl32(wave x 32767))) in fp32 on the CPU: the int16 a launch must return for the waveform the same launch returned."""
    v = (wave.float() * torch.tensor(32767.0)).clamp(-32768.0, 32767.0)
    return (torch.round(v) if mut == "round_nearest" else torch.trunc(v)).to(torch.int16)


def ola_launch(eng, case, o, items=None):
    """items: launch only those items, each as a batch of one (-> the same dict, rows in that order)."""
    n, hop, Tm = case.n, case.hop, case.T_max
    L = Tm * hop
    res = dict(pcm=[], wave=[], pcm_len=[])
    groups = [list(range(case.B))] if items is None else [[b] for b in items]
    ww, dw = framed(o.window.reshape(-1, 1), 0, 4)
    for grp in groups:
        nb = len(grp)
        fw, df = framed(torch.cat([o.frames[b * Tm:(b + 1) * Tm] for b in grp]), 2 * Tm, 2 * Tm)
        lens = table(torch.tensor([case.lens[b] for b in grp]), 10 ** 6)
        ld_pcm, ld_wave = L + case.ld_extra, L + case.ld_extra + 1
        pw, pcm = _guarded((nb, ld_pcm), 64, 1234, init=torch.full((nb, ld_pcm), 1234, dtype=torch.int16), dtype=torch.int16)
        lw, plen = _guarded((nb,), 8, SENTINEL, init=torch.full((nb,), SENTINEL, dtype=I32), dtype=I32)
        wv = None
        if case.wave:
            wvw, wv, wg = out_rows(nb, ld_wave)
        check(eng, eng.lib.vv_vocos_ola(eng.ctx, ptr(df), n + case.ld_f_extra, nb, Tm, ptr(lens[1]), ptr(dw), n, hop, ptr(pcm), ld_pcm, ptr(plen),
                                        ptr(wv), ld_wave, stream()))
        torch.cuda.synchronize()
        _bands_intact(pw, 64, 1234, case.name + ": pcm")
        _bands_intact(lw, 8, SENTINEL, case.name + ": pcm_len")
        frame_intact(fw, df, case.name + ": frames")
        assert bool((pcm[:, L:] == 1234).all()), f"{case.name}: pcm was written behind T_max * hop"
        res["pcm"].append(pcm[:, :L].cpu())
        res["pcm_len"].append(plen.cpu())
        if case.wave:
            _bands_intact(wvw, wg, FILL, case.name + ": wave")
            assert bool((wv[:, L:] == FILL).all()), f"{case.name}: wave was written behind T_max * hop"
            res["wave"].append(wv[:, :L].cpu())
    return dict(pcm=torch.cat(res["pcm"]), pcm_len=torch.cat(res["pcm_len"]), wave=torch.cat(res["wave"]) if case.wave else None)


def ola_cases():
    k = 4
    return [
        OlaCase("ola/n16_hop4", 16, 4, 30, (0, 1, 2, k, k + 1, 30, -3, 99), seed=9000),
        OlaCase("ola/n16_hop4_no_wave", 16, 4, 6, (6, 3), wave=False, seed=9001),
        OlaCase("ola/n8_hop8", 8, 8, 5, (5, 1, 2), seed=9002),
        OlaCase("ola/n64_hop16_two_blocks", 64, 16, 20, (20, 7), seed=9003),          # 320 samples: a second workgroup of 256
    ]


# ================================================================================================ conv_post
# z = bias + sum_{c, k} w lrelu(x): one fp32 fma chain of 7 C steps; A_z = |bias| + sum |w| |lrelu x|.  y = tanh z moves by (1 - y^2) dz
# and takes tanhf's own rounding, relative to |y|: A_e = A_z (1 - y^2) + |y|.  Bound: conv_bound's floor of 8 x 2^-24 (gpu_util: a product
# rounding and the epilogue's, with room) or 4 x the yardstick -- the CPU library's fp32 conv1d + tanh -- whichever is larger.
POST_C = 8.0
POST_WAVE, POST_WG = 248, 992
POST_SEAM_LENS = tuple(range(245, 252)) + tuple(range(989, 996))
POST_SMALL_LENS = (0, 1, 3, 4, 5)


@dataclasses.dataclass
class PostCase:
    name: str
    C: int
    T: int
    lens: tuple                 # per item; None entries = T
    shift: int = 0              # floats the `in` pointer is moved by (1: 4 bytes, the non-VEC form at T % 4 == 0)
    ld_extra: int = 1
    seed: int = 0

    @property
    def B(self):
        return len(self.lens)

    @property
    def form(self):
        """(VEC, CB) of the instantiation vvk_conv_post picks."""
        vec = self.T % 4 == 0 and self.shift % 4 == 0
        return (True, 8) if vec and self.C % 8 == 0 else (True, 4) if vec and self.C % 4 == 0 else (True, 1) if vec else (False, 1)

    def ops(self):
        g = _gen(self.seed)
        o = type("Ops", (), {})()
        o.x = torch.randn(self.B, self.C, self.T, generator=g)
        o.w = torch.randn(self.C, 7, generator=g) / math.sqrt(self.C * 7) * 0.9
        o.bias = -0.03
        o.lens = [self.T if v is None else v for v in self.lens]
        return o


POST_MUTATIONS = ("causal", "mask_at_T", "no_lrelu")
POST_SLOPE = 0.01


def post_eval(case, o, dtype=torch.float64, mut=None):
    """-> (y [B][T], A_e)."""
    B, Cc, T = case.B, case.C, case.T
    x = o.x.to(dtype).clone()
    if mut != "mask_at_T":
        for b, L in enumerate(o.lens):
            x[b, :, min(max(L, 0), T):] = 0.0
    a = x if mut == "no_lrelu" else torch.where(x >= 0, x, x * torch.tensor(POST_SLOPE, dtype=dtype))
    left = 6 if mut == "causal" else 3
    ap = torch.nn.functional.pad(a, (left, 6 - left))
    w = o.w.to(dtype)
    bias = torch.tensor(o.bias, dtype=torch.float32).to(dtype)
    if dtype == torch.float32:
        z = torch.nn.functional.conv1d(ap, w[None], bias[None]).reshape(B, T)        # the CPU library's own fp32 convolution
    else:
        z = bias + sum(w[None, :, k, None] * ap[:, :, k:k + T] for k in range(7)).sum(dim=1)
    y = torch.tanh(z)
    Az = bias.double().abs() + sum(o.w.double().abs()[None, :, k, None] * ap.double().abs()[:, :, k:k + T] for k in range(7)).sum(dim=1)
    return y, Az * (1.0 - y.double() ** 2) + y.double().abs()


def post_launch(eng, case, o):
    B, Cc, T = case.B, case.C, case.T
    flat = torch.full((8 + o.x.numel() + 8 + 4,), NAN, device=DEV)
    off = 8 + case.shift
    flat[off:off + o.x.numel()] = o.x.reshape(-1).to(DEV)
    ww, dw = framed(o.w, 0, 2)
    lens = table(torch.tensor(case_lens_raw(case)), 10 ** 6)
    ld = T + case.ld_extra
    pw, pcm = _guarded((B, ld), 64, 1234, init=torch.full((B, ld), 1234, dtype=torch.int16), dtype=torch.int16)
    wvw, wv = _guarded((B, T), 64, FILL, init=torch.full((B, T), FILL))
    check(eng, eng.lib.vv_conv_post(eng.ctx, flat.data_ptr() + 4 * off, ptr(dw), o.bias, ptr(pcm), ld, ptr(wv), B, Cc, T, 7, POST_SLOPE, ptr(lens[1]),
                                    stream()))
    torch.cuda.synchronize()
    _bands_intact(pw, 64, 1234, case.name + ": pcm")
    _bands_intact(wvw, 64, FILL, case.name + ": wave")
    assert bool((pcm[:, T:] == 1234).all()), f"{case.name}: pcm was written behind T"
    return dict(pcm=pcm[:, :T].cpu(), wave=wv.cpu())


def case_lens_raw(case):
    return [case.T if v is None else v for v in case.lens]


def post_cases():
    """Each instantiation (C 8 -> <VEC, 8>, 12 -> <VEC, 4>, 7 -> <VEC, 1>; T % 4 != 0 or a pointer moved by 4 bytes -> <!VEC, 1>) meets every
    valid length around the wave seam (248) and the workgroup seam (992), every residue mod 4 among them, and the small lengths."""
    cases = []
    seam = POST_SEAM_LENS + POST_SMALL_LENS + (None, -5, 5000)
    for Cc in (8, 12, 7):
        cases.append(PostCase(f"conv_post/C{Cc}_T1000_vec", Cc, 1000, seam, ld_extra=0 if Cc == 12 else 1, seed=9500 + Cc))      # ld_pcm % 4 == 0: 8-byte PCM stores
        cases.append(PostCase(f"conv_post/C{Cc}_T1001_scalar", Cc, 1001, seam, seed=9520 + Cc))
        cases.append(PostCase(f"conv_post/C{Cc}_T1000_shift4B", Cc, 1000, seam, shift=1, ld_extra=0 if Cc == 8 else 1, seed=9540 + Cc))
    cases.append(PostCase("conv_post/C64_T4", 64, 4, (4, 3, 0), seed=9560))
    cases.append(PostCase("conv_post/C1_T1", 1, 1, (1, 0), seed=9561))
    return cases
