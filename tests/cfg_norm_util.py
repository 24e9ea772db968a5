"""Helpers of the CFG-Zero* / guidance-rescale tests (tests/test_cfg_norm_cpu.py, tests/test_cfg_norm_gpu.py), no GPU
needed to import.

  the rule        ``rule_exact`` in rationals (Fraction; rho enters as rho^2, which is rational), ``rule64`` in float64 with s and f rounded to
                  fp32 once, as the specification says
  the sums        ``gram_mirror``: cfg_gram_reduce_kernel and the serial tile sum of cfg_norm_coef_kernel restated with numpy alone, bit for
                  bit (tiles of 32 frames from the item's frame 0, float4 q on thread q % 256, a product then an add, one LDS tree)
  the coefficients  ``coef_from_sums``: cfg_norm_coef_kernel's formula in float64; ``coef_exact``: the same from extended-precision sums, with
                  the bound on the device's (s, f) derived from the summation error (below), as coef_bound does in test_apg_gpu.py
  the solver      ``ref_solve_norm``: sampler_util.ref_solve_all's structure with the new slope and the truncated plan of zero-init

The bound on (s, f), derived (the device result plays no part).  A sum S_xy of the device is a float64 sum whose longest chain is
L = 4 ceil(tile float4s / 256) + 8 (thread-serial adds and the tree) + n_tiles (the serial tile sum) additions, plus one rounding of the
product: |dS_xy| <= gam T_xy, gam = (L + 1) 2^-53 and T_xy = sum |x y|.
  s = S_cu / S_uu:  |ds| <= gam (T_cu / S_uu + |s|) + 2 |s| 2^-53 (the division and the quotient rule's second term), then one fp32 rounding
      |s| 2^-24.
  V_xy = S_xy / n - (S_x / n)(S_y / n):  |dV_xy| <= gam (T_xy / n + (T_x |S_y| + |S_x| T_y) / n^2) + 4 2^-53 (|S_xy| / n + |S_x S_y| / n^2).
  var_k = a^2 V_cc + 2 a c V_cu + c^2 V_uu with c = -g s32:  the device's fp32 s may differ from the reference's by the bound of s, so
      |dc| <= |g| bound_s and |dvar| <= a^2 dV_cc + 2 |a c| dV_cu + c^2 dV_uu + |2 a V_cu + 2 c V_uu| |dc| + 8 2^-53 (a^2 |V_cc| + 2 |a c V_cu| +
      c^2 |V_uu|).
  rho = sqrt(V_cc / var_k):  with r = dV_cc / V_cc + dvar / var_k (< 1/2 asserted), |drho| <= rho r (twice the first-order term) + 2 rho 2^-53.
  f = phi rho + (1 - phi):  |df| <= phi drho + 4 |f| 2^-53, then one fp32 rounding |f| 2^-24.
"""
import math
from fractions import Fraction

import numpy as np

from tests.sampler_util import _ab_step, grid64

TILE = 32                     # VV_APG_TILE
THREADS = 256
EPS53 = 2.0 ** -53
EPS24 = 2.0 ** -24
MODEL_SEED = 9527             # sampler_util's: |s* - 1| > 1e-2 on every guided evaluation of the ragged three (checked on the CPU file)
PHI = 0.7
# per-item options of the ragged three (strengths sampler_util.ITEM_G = (2.0, 0.0, 3.0)): name -> ((star, phi) per item)
OPTION_SETS = {
    "star": ((True, None),) * 3,
    "rescale": ((False, PHI),) * 3,
    "both": ((True, PHI),) * 3,
    "mixed": ((True, PHI), (True, None), (False, None)),        # item 2 (strength 3.0) is off: the plain rule in the same call
}
NORM_PLANS = {"euler": ("euler", 8), "rk4": ("rk4", 3), "ab2": ("ab2", 8)}
NORM_SLOPE_C = 6.0            # roundings of k = f (pc + (pc - s pu) g) in units of 2^-24 K, K = |f| (|pc| + |g| (|pc| + |s pu|)): the product s pu, the
                              # difference and the product with g, each carried by |f g| (3 |f g| (|pc| + |s pu|) <= 3 K), the sum and the product
                              # with f (2 K); 6 leaves one to spare


# ------------------------------------------------------------------------------------------------ the rule
def rule_exact(pc, pu, g, star, phi):
    """The rule on rationals.  -> dict(s, k0, var_k, V_cc, rho2, f_of_rho): rho2 = V_cc / var_k (1 where either is <= 0), and f_of_rho(rho)
    = phi rho + 1 - phi, so that a caller can state properties of k = f k0 without a square root."""
    pc, pu = [Fraction(v) for v in pc], [Fraction(v) for v in pu]
    g, phi = Fraction(g), Fraction(phi)
    n = len(pc)
    S = lambda a, b: sum(x * y for x, y in zip(a, b))
    Scu, Suu, Scc, Sc, Su = S(pc, pu), S(pu, pu), S(pc, pc), sum(pc), sum(pu)
    s = Scu / Suu if (star and Suu != 0) else Fraction(1)
    k0 = [c + (c - s * u) * g for c, u in zip(pc, pu)]
    a, c = 1 + g, -g * s
    V = lambda Sxy, Sx, Sy: Sxy / n - (Sx / n) * (Sy / n)
    Vcc, Vcu, Vuu = V(Scc, Sc, Sc), V(Scu, Sc, Su), V(Suu, Su, Su)
    var_k = a * a * Vcc + 2 * a * c * Vcu + c * c * Vuu
    rho2 = Vcc / var_k if (var_k > 0 and Vcc > 0) else Fraction(1)
    return dict(s=s, k0=k0, var_k=var_k, V_cc=Vcc, rho2=rho2, f_of_rho=lambda rho: phi * rho + (1 - phi))


def variance(v):
    v = [Fraction(x) for x in v]
    m = sum(v) / len(v)
    return sum((x - m) ** 2 for x in v) / len(v)


def sums64(pc, pu):
    """The five sums in extended precision (numpy longdouble) and the sums of the absolute terms: (S[5], T[5]) as float64."""
    ld = np.longdouble
    c, u = np.asarray(pc, dtype=np.float64).astype(ld).ravel(), np.asarray(pu, dtype=np.float64).astype(ld).ravel()
    terms = (c * u, u * u, c * c, c, u)
    return np.array([float(t.sum()) for t in terms]), np.array([float(np.abs(t).sum()) for t in terms])


def coef_from_sums(S, n, g, star, phi):
    """cfg_norm_coef_kernel's formula in float64 from the five sums (S_cu, S_uu, S_cc, S_c, S_u) and the element count n -> (s, f) as
    np.float32, each rounded once."""
    Scu, Suu, Scc, Sc, Su = (np.float64(v) for v in S)
    s = np.float32(1.0)
    if star and Suu != 0.0:
        s = np.float32(Scu / Suu)
    f = np.float32(1.0)
    phi = np.float64(np.float32(phi or 0.0))
    if phi != 0.0:
        gb = np.float64(np.float32(g))
        a, c = np.float64(1.0) + gb, -gb * np.float64(s)
        cnt = np.float64(n)
        mc, mu = Sc / cnt, Su / cnt
        Vcc, Vcu, Vuu = Scc / cnt - mc * mc, Scu / cnt - mc * mu, Suu / cnt - mu * mu
        var_k = (a * a) * Vcc + (np.float64(2.0) * a * c) * Vcu + (c * c) * Vuu
        rho = np.sqrt(Vcc / var_k) if (var_k > 0.0 and Vcc > 0.0) else np.float64(1.0)
        f = np.float32(phi * rho + (np.float64(1.0) - phi))
    return s, f


def rule64(pc, pu, g, star, phi):
    """The rule in float64 on one item's predictions (any float arrays of one shape) -> (s, f, k): the sums in extended precision, s and f
    rounded to fp32 once, k = f (pc + (pc - s pu) g) in float64."""
    S, _ = sums64(pc, pu)
    s, f = coef_from_sums(S, np.asarray(pc).size, g, star, phi)
    pc, pu = np.asarray(pc, dtype=np.float64), np.asarray(pu, dtype=np.float64)
    return s, f, float(f) * (pc + (pc - float(s) * pu) * float(np.float32(g)))


# ------------------------------------------------------------------------------------------------ the device's sums, restated
def _tree(v):
    v = v.copy()
    w = THREADS // 2
    while w > 0:
        v[:w] = v[:w] + v[w: 2 * w]
        w //= 2
    return v[0]


def gram_mirror(pc, pu):
    """(partials [n_tiles][5], sums [5]) of one item as cfg_gram_reduce_kernel and the serial tile sum of cfg_norm_coef_kernel compute them:
    pc, pu float32 [frames][n_mel], n_mel a multiple of 4.  Every product rounded, then added (never fused)."""
    pc, pu = np.ascontiguousarray(pc, dtype=np.float32), np.ascontiguousarray(pu, dtype=np.float32)
    frames = pc.shape[0]
    parts = []
    tot = np.zeros(5)
    for f0 in range(0, frames, TILE):
        c = pc[f0: f0 + TILE].astype(np.float64).reshape(-1, 4)                  # float4 q of the tile = row q
        u = pu[f0: f0 + TILE].astype(np.float64).reshape(-1, 4)
        total = c.shape[0]
        rounds = -(-total // THREADS)
        terms = []
        for t in (c * u, u * u, c * c, c, u):
            pad = np.zeros((rounds * THREADS, 4))
            pad[:total] = t
            terms.append(pad)
        acc = [np.zeros(THREADS) for _ in range(5)]
        for r in range(rounds):                                                  # thread t's float4s: q = t, t + 256, ...
            for j in range(4):
                for i in range(5):
                    acc[i] = acc[i] + terms[i][r * THREADS: (r + 1) * THREADS, j]      # a thread past the tile's end adds +0.0: the same bits
        p = np.array([_tree(a) for a in acc])
        parts.append(p)
        tot = tot + p
    return (np.array(parts) if parts else np.zeros((0, 5))), tot


def chain(frames, n_mel):
    """The longest chain of additions behind a sum of an item, and one more for the product's rounding."""
    nt = -(-frames // TILE)
    return 4 * -(-(min(frames, TILE) * (n_mel // 4)) // THREADS) + 8 + nt + 1


def coef_exact(pc, pu, g, star, phi):
    """-> (s, f, bound_s, bound_f): the float64 reference of an item's coefficients from extended-precision sums, and the bounds of the
    module docstring for a device that sums in cfg_gram_reduce_kernel's order."""
    pc, pu = np.asarray(pc, dtype=np.float32), np.asarray(pu, dtype=np.float32)
    n = pc.size
    S, T = sums64(pc, pu)
    s32, f32 = coef_from_sums(S, n, g, star, phi)
    gam = chain(pc.shape[0], pc.shape[1]) * EPS53
    Scu, Suu, Scc, Sc, Su = S
    Tcu, Tuu, Tcc, Tc, Tu = T
    s = float(s32)
    bs = 0.0
    if star and Suu != 0.0:
        bs = gam * (Tcu / Suu + abs(s)) + 2 * abs(s) * EPS53 + abs(s) * EPS24
    bf = 0.0
    phi = float(np.float32(phi or 0.0))
    if phi != 0.0:
        gb = float(np.float32(g))
        a, c = 1.0 + gb, -gb * s
        V = lambda Sxy, Sx, Sy: Sxy / n - (Sx / n) * (Sy / n)
        dV = lambda Sxy, Txy, Sx, Tx, Sy, Ty: gam * (Txy / n + (Tx * abs(Sy) + abs(Sx) * Ty) / n ** 2) + 4 * EPS53 * (abs(Sxy) / n + abs(Sx * Sy) / n ** 2)
        Vcc, Vcu, Vuu = V(Scc, Sc, Sc), V(Scu, Sc, Su), V(Suu, Su, Su)
        dcc, dcu, duu = dV(Scc, Tcc, Sc, Tc, Sc, Tc), dV(Scu, Tcu, Sc, Tc, Su, Tu), dV(Suu, Tuu, Su, Tu, Su, Tu)
        var_k = a * a * Vcc + 2 * a * c * Vcu + c * c * Vuu
        if var_k > 0.0 and Vcc > 0.0:
            dvar = (a * a * dcc + 2 * abs(a * c) * dcu + c * c * duu + abs(2 * a * Vcu + 2 * c * Vuu) * abs(gb) * bs
                    + 8 * EPS53 * (a * a * abs(Vcc) + 2 * abs(a * c * Vcu) + c * c * abs(Vuu)))
            r = dcc / Vcc + dvar / var_k
            assert r < 0.5, "the case is too ill-conditioned for the first-order bound"
            rho = math.sqrt(Vcc / var_k)
            bf = phi * (rho * r + 2 * rho * EPS53)
        bf += 4 * abs(float(f32)) * EPS53 + abs(float(f32)) * EPS24
    return s32, f32, bs, bf


# ------------------------------------------------------------------------------------------------ operands of the kernel entries
LENS = (1, 31, 32, 33, 97, 0)
GUIDED = (True, True, False, True, True, True)           # one unguided item: its rows have u_row < 0 and nothing is reduced for it
ORDER = (4, 0, 5, 2, 1, 3)                               # the items' places in the packed rows: row_start is not ascending
G_ITEM = (2.0, 3.0, 1.5, -0.5, 2.5, 2.0)
STAR = (1.0, 1.0, 1.0, 0.0, 1.0, 1.0)
RESC = (0.7, 0.0, 0.7, 1.0, 0.25, 0.7)


def coef_ops(n_mel, ldp, lens=LENS, order=ORDER, guided=GUIDED, seed=0):
    import torch
    g = torch.Generator().manual_seed(5000 + seed + n_mel + ldp)
    B = len(lens)
    start = [0] * B
    at = 0
    for b in order:
        start[b] = at
        at += lens[b]
    Rc = at
    item = torch.empty(Rc, dtype=torch.long)
    for b in range(B):
        item[start[b]: start[b] + lens[b]] = b
    mapped = torch.tensor(guided)[item]
    Ru = int(mapped.sum())
    u_row = torch.full((Rc,), -1, dtype=torch.int32)
    u_row[mapped] = Rc + torch.arange(Ru, dtype=torch.int32)
    pred = torch.randn(Rc + Ru, ldp, generator=g)
    pred[Rc:, :n_mel] = 0.6 * pred[:Rc][mapped][:, :n_mel] + 0.5 * pred[Rc:, :n_mel] + 0.1      # correlated and off-centre: s away from 1, means not 0
    pred[:, n_mel:] = float("nan")                                                                      # the pad columns of an ldp-wide row
    return dict(B=B, Rc=Rc, Ru=Ru, start=start, lens=lens, u_row=u_row, pred=pred, n_mel=n_mel, ldp=ldp, guided=guided)


def stage_cases():
    """step_util's (n_mel, ldp) pairs x 1, 3 and 86 rows on the guided form, walking the methods' stages, the strengths and the u_row maps."""
    from tests import step_util as T
    out, i = [], 0
    stages = T.method_stages()
    for (M, ldp) in T.STAGE_SHAPES:
        for Rc in (1, 3, 86):
            m, s = stages[(3 * i + 1) % len(stages)]
            out.append(T.StageCase(f"norm/{m}{s}/M{M}_ld{ldp}_Rc{Rc}", "guided", M, ldp, Rc, m, s, T.STAGE_G[i % 3], i % 2 == 1, True,
                                   ("all", "alt", "none")[i % 3] if i % 5 else "all", False, 7000 + i))
            i += 1
    return out


def stage_ref(case, o, coef):
    """float64: k = f (pc + (pc - s pu) g) on the mapped rows, pc elsewhere; the state as step_util.stage_eval forms it; the scales."""
    import torch
    Rc, M = case.Rc, case.n_mel
    pc = o.pred[:Rc, :M].double()
    has_u = o.u_row >= 0
    pool = torch.cat([o.pred[:, :M], torch.full((1, M), float("nan"))]).double()
    pu = pool[o.u_row.long().clamp_min(0)]
    g = o.g_item[o.item].double()[:, None] if o.g_item is not None else torch.tensor(case.g, dtype=torch.float64)
    s, f = coef[o.item, 0].double()[:, None], coef[o.item, 1].double()[:, None]
    k = f * (pc + (pc - s * pu) * g)
    K = f.abs() * (pc.abs() + g.abs() * (pc.abs() + (s * pu).abs()))
    k = torch.where(has_u[:, None], k, pc)
    K = torch.where(has_u[:, None], K, pc.abs())
    acc = o.x[o.xr].double()
    mag = acc.abs()
    coefs = list(case.coef)
    for j, c in enumerate(coefs):
        if c == 0:
            continue
        kj, Kj = (k, K) if j == len(coefs) - 1 else (o.k_prev[j].double(), o.k_prev[j].double().abs())
        mag = mag + abs(float(c)) * Kj
        acc = acc + float(c) * kj
    return dict(k=k, K=K, acc=acc, mag=mag)


# ------------------------------------------------------------------------------------------------ the reference solver
def ref_solve_norm(orc, pre, x, plan, *, g, star=False, phi=None, mask_col=None, skip=0, nfe=None, calls=None, log=None):
    """sampler_util.ref_solve_all's structure with the slope of N24, one item, in the oracle's dtype.  plan: the plan in force (the
    truncated one under zero-init: ``skip`` = K and ``nfe`` = the grid's points name the float64 grid points K ... nfe - 1 an
    Adams-Bashforth plan steps on; the order ramp starts at the first step that exists).  mask_col: 0 / 1 per evaluation of the plan (None:
    1 everywhere).  At a guided evaluation: the five sums in float64, s = S_cu / S_uu (star on and S_uu != 0) and f as
    cfg_norm_coef_kernel forms them, each rounded to fp32 once, and the slope f (pc + (pc - s pu) g).  log: a list that receives
    (evaluation, s, f) of every guided evaluation."""
    import torch
    ropes = (pre["rope_cos_q"], pre["rope_sin_q"], pre["rope_cos_k"], pre["rope_sin_k"])
    cat, drop = pre["cat_mel_text"], pre["cat_mel_text_drop"]
    n_steps, s_ = int(plan.dt.numel()), plan.s
    q = 0 if plan.beta is None else len(plan.beta[0])
    t64 = grid64(nfe if nfe is not None else n_steps + 1, orc.spec.sway_coef)[skip:] if q else None
    calls = [(0, n_steps)] if calls is None else list(calls)
    g32 = float(np.float32(g))

    def slope(e, t_e, xi):
        orc.t_grid = [t_e]
        pc = orc.dit_forward(xi, cat, ropes, 0)
        col = 1 if mask_col is None else mask_col[e]
        if col == 0 or g == 0.0:
            return pc
        pu = orc.dit_forward(xi, drop, ropes, 0)
        c64, u64 = pc.double(), pu.double()
        S = [float((c64 * u64).sum()), float((u64 * u64).sum()), float((c64 * c64).sum()), float(c64.sum()), float(u64.sum())]
        sb, fb = coef_from_sums(S, pc.numel(), g32, star, phi)
        if log is not None:
            log.append((e, float(sb), float(fb)))
        sb, fb = torch.tensor(float(sb), dtype=pc.dtype), torch.tensor(float(fb), dtype=pc.dtype)
        return fb * (pc + (pc - sb * pu) * g32)

    for step0, n in calls:
        f = []
        for st in range(step0, step0 + n):
            if q:
                f.append(slope(st, float(np.float32(t64[st])), x))
                x = _ab_step(x, t64, st, f, min(q, st - step0 + 1))
                f = f[-3:]
                continue
            h, ks = float(plan.dt[st]), []
            for i in range(s_):
                xi = x
                for j in range(i):
                    if plan.a[i][j] != 0.0:
                        xi = xi + (h * plan.a[i][j]) * ks[j]
                ks.append(slope(st * s_ + i, float(plan.t[st * s_ + i]), xi))
            for j in range(s_):
                if plan.b[j] != 0.0:
                    x = x + (h * plan.b[j]) * ks[j]
    return x


_REFS = {}


def reference(dtype, plan_level, b, g, star, phi, interval=None, skip=0, log=None):
    """ref_solve_norm for item b of sampler_util's ragged three on a plan of NORM_PLANS, in the fp32 or the float64 oracle; computed once."""
    from tests import sampler_util as S
    from vietvoice_tts_amd.model_spec import ode_plan
    spec, _, _, orcs, pres = S.setup()
    key = (dtype, plan_level, b, g, bool(star), phi, interval, skip)
    if key not in _REFS:
        method, nfe = NORM_PLANS[plan_level]
        plan = ode_plan(nfe, spec.sway_coef, method, skip=skip)
        t = [float(v) for v in plan.t]
        col = S.mask_column(t, g, interval, None) if (interval is not None or g == 0.0) else None
        pre = pres[dtype, b]
        lg = []
        _REFS[key] = (ref_solve_norm(orcs[dtype], pre, pre["noise"], plan, g=g, star=star, phi=phi, mask_col=col, skip=skip, nfe=nfe, log=lg), lg)
    if log is not None:
        log.extend(_REFS[key][1])
    return _REFS[key][0]


def parity_refs(plan_level, b, g, star, phi, interval=None, skip=0):
    """-> (ref64, yardstick, bound): the float64 reference, the fp32 solver's distance from it and sampler_util.bound of that."""
    from tests import sampler_util as S
    r64 = reference("f64", plan_level, b, g, star, phi, interval, skip)
    y = S.err(reference("f32", plan_level, b, g, star, phi, interval, skip), r64)
    return r64, y, S.bound(y)
