"""Helpers of the N23 tests (block caching and its report), no GPU needed to import.

``schedule`` restates the rule of DESIGN §8 N23 from the evaluation times, NOT through ``model_spec.block_cache_schedule``: the two meet
only in the tests.  ``report_mirror`` restates the report's sums in the tile and thread order of block_drift_reduce_kernel, in numpy
float64 (every difference, product and add rounded on its own, as the kernel's); ``report_plain`` is the same two sums as plain loops.
``ref_forward_cached`` is the DiT forward with the span rule, built from the oracle's parts; ``ref_solve_cached`` the reference solver
around it."""
import numpy as np

TILE = 32             # VV_APG_TILE
THREADS = 256
FULL, STORE, LIGHT = 0, 1, 2
MARK, DIFF, APPLY = 0, 1, 2


def schedule(t, every, interval=None, report=False):
    """t: the evaluation times (non-decreasing); -> a list of 0 / 1 / 2 per evaluation.  The candidates are the evaluations inside the
    interval (all of them without one); the j-th candidate is light when every > 1 and j is no multiple of every; a full evaluation
    stores when the next one is light, or always under a report."""
    cand = [interval is None or interval[0] <= float(v) <= interval[1] for v in t]
    out, j = [], 0
    for c in cand:
        light = False
        if c:
            light = every > 1 and j % every != 0
            j += 1
        out.append(LIGHT if light else FULL)
    for e in range(len(out)):
        if out[e] == FULL and (report or (e + 1 < len(out) and out[e + 1] == LIGHT)):
            out[e] = STORE
    return out


def blocks_run(modes, span, depth):
    """Blocks launched per evaluation: depth, less the span's at a light one."""
    return [depth - (span[1] - span[0]) if m == LIGHT else depth for m in modes]


def check_modes(modes, span, depth, n_evals, e0=0, e1=None):
    """What the steps entry refuses of a schedule, restated: -> None, or the reason as a short word."""
    e1 = n_evals if e1 is None else e1
    if not 0 <= span[0] < span[1] <= depth:
        return "span"
    if len(modes) != n_evals:
        return "n_modes"
    if any(v > 2 for v in modes):
        return "value"
    stored = False
    for e in range(e0, e1):
        if modes[e] == LIGHT and e0 != 0:
            return "step0"
        if modes[e] == LIGHT and not stored:
            return "2 before 1"
        stored = stored or modes[e] == STORE
    return None


def _tree(v):
    """The kernel's LDS tree over the 256 thread sums: red[t] += red[t + w], w = 128 ... 1."""
    v = v.copy()
    w = THREADS // 2
    while w > 0:
        v[:w] = v[:w] + v[w: 2 * w]
        w //= 2
    return v[0]


def report_mirror(d_new, d_prev):
    """(E2, N2) of one sequence (one CFG branch of one item) as block_drift_reduce_kernel and the finishing kernel compute them.  d_new:
    float32 [frames][D] (D a multiple of 4), the stored contribution; d_prev: the one stored before it, or None (the first store of the
    call: E2 = 0).  In float64: d = d_new - d_prev, d * d, sum + that, each rounded on its own.  Tiles of TILE frames from frame 0; float4
    q of a tile on thread q % 256, its four elements in order; one tree per tile; the tiles added in ascending order from 0.0."""
    dn = np.ascontiguousarray(d_new, dtype=np.float32)
    frames = dn.shape[0]
    E2 = N2 = np.float64(0.0)
    for f0 in range(0, frames, TILE):
        a = dn[f0: f0 + TILE].astype(np.float64).reshape(-1, 4)                  # float4 q of the tile = row q
        total = a.shape[0]
        rounds = -(-total // THREADS)
        sq = np.zeros((rounds * THREADS, 4))
        sq[:total] = a * a
        dd = np.zeros((rounds * THREADS, 4))
        if d_prev is not None:
            p = np.ascontiguousarray(d_prev, dtype=np.float32)[f0: f0 + TILE].astype(np.float64).reshape(-1, 4)
            d = a - p
            dd[:total] = d * d
        s1, s2 = np.zeros(THREADS), np.zeros(THREADS)
        for r in range(rounds):                                                   # thread t's float4s: q = t, t + 256, ...
            for j in range(4):
                s2 = s2 + sq[r * THREADS: (r + 1) * THREADS, j]                   # a thread past the tile's end adds +0.0: the same bits
                if d_prev is not None:
                    s1 = s1 + dd[r * THREADS: (r + 1) * THREADS, j]
        E2 = E2 + _tree(s1)
        N2 = N2 + _tree(s2)
    return float(E2), float(N2)


def report_plain(d_new, d_prev):
    """The same two sums as plain float64 loops over the sequence's elements (row by row, left to right)."""
    e2 = n2 = 0.0
    for r in range(d_new.shape[0]):
        for c in range(d_new.shape[1]):
            v = float(d_new[r, c])
            n2 += v * v
            if d_prev is not None:
                d = v - float(d_prev[r, c])
                e2 += d * d
    return e2, n2


def ref_forward_cached(orc, x, cat, ropes, span, mode, cache, key):
    """Oracle.dit_forward at the time orc.t_grid[0] with the span rule: ``mode`` STORE keeps cache[key] = h at the entry of block span[1]
    (or of the final norm) less h at the entry of block span[0]; LIGHT runs blocks [0, span[0]), adds cache[key], runs blocks [span[1],
    depth); FULL is dit_forward."""
    import torch.nn.functional as F
    s, w = orc.spec, orc.w
    d, (a, b) = s.dim, span
    temb = F.silu(orc.time_embed(0))
    h = orc.input_embed(x, cat)
    mark = None
    for i in range(s.depth + 1):
        if mode == LIGHT and a <= i < b:
            if i == a:
                h = h + cache[key]
            continue
        if mode == STORE and i == a:
            mark = h
        if mode == STORE and i == b:
            cache[key] = h - mark
        if i == s.depth:
            break
        p = f"blocks.{i}"
        mod = F.linear(temb, w[p + ".adaln.weight"], w[p + ".adaln.bias"])
        sh_a, sc_a, g_a, sh_m, sc_m, g_m = mod.chunk(6)
        n = F.layer_norm(h, (d,), eps=1e-6) * (1 + sc_a) + sh_a
        h = h + g_a * orc.attention(n, p, ropes)
        m = F.layer_norm(h, (d,), eps=1e-6) * (1 + sc_m) + sh_m
        m = F.gelu(F.linear(m, w[p + ".ff1.weight"], w[p + ".ff1.bias"]), approximate="tanh")
        h = h + g_m * F.linear(m, w[p + ".ff2.weight"], w[p + ".ff2.bias"])
    mod = F.linear(temb, w["final.adaln.weight"], w["final.adaln.bias"])
    sc_f, sh_f = mod.chunk(2)
    h = F.layer_norm(h, (d,), eps=1e-6) * (1 + sc_f) + sh_f
    return F.linear(h, w["final.proj.weight"], w["final.proj.bias"])


def ref_solve_cached(orc, pre, x, method, nfe_step, g, span, modes, planes=None):
    """The reference solver with N23's rule, one item.  modes[e] in 0 / 1 / 2 per evaluation e = step * s + stage; both CFG branches keep
    their own contribution; slope pc + (pc - pu) g.  method: a Runge-Kutta name of model_spec.ODE_METHODS, or "ab2" / "ab3"
    (tests.multistep_util.newton_step on the float64 grid).  planes: a list that receives per evaluation the pair of stored contributions
    (conditional, unconditional) where the evaluation stores, None elsewhere."""
    from tests.multistep_util import grid64, newton_step
    from vietvoice_tts_amd.model_spec import ODE_MULTISTEP, ode_plan
    ropes = (pre["rope_cos_q"], pre["rope_sin_q"], pre["rope_cos_k"], pre["rope_sin_k"])
    cache = {}

    def slope(e, t_e, xi):
        orc.t_grid = [t_e]
        pc = ref_forward_cached(orc, xi, pre["cat_mel_text"], ropes, span, modes[e], cache, "c")
        pu = ref_forward_cached(orc, xi, pre["cat_mel_text_drop"], ropes, span, modes[e], cache, "u")
        if planes is not None:
            planes.append((cache["c"].clone(), cache["u"].clone()) if modes[e] == STORE else None)
        return pc + (pc - pu) * g

    if method in ODE_MULTISTEP:
        t = grid64(nfe_step, orc.spec.sway_coef)
        f = []
        for n in range(nfe_step - 1):
            f.append(slope(n, float(np.float32(t[n])), x))
            x = newton_step(x, t, n, f, ODE_MULTISTEP[method])
            f = f[-3:]
        return x
    plan = ode_plan(nfe_step, orc.spec.sway_coef, method)
    for n in range(plan.dt.numel()):
        h, k = float(plan.dt[n]), []
        for i in range(plan.s):
            xi = x
            for j in range(i):
                if plan.a[i][j] != 0.0:
                    xi = xi + (h * plan.a[i][j]) * k[j]
            k.append(slope(n * plan.s + i, float(plan.t[n * plan.s + i]), xi))
        for j in range(plan.s):
            if plan.b[j] != 0.0:
                x = x + (h * plan.b[j]) * k[j]
    return x


# ------------------------------------------------------------------------------------------------ shared with tools/elementwise_host_check.py
SPAN_ROWS = (1, 3, 86)
SPAN_DIMS = (128, 1024)
SPAN_PENDING = ("none", "f32", "bf16")        # nothing pending (l = 0), two fp32 deltas, two bf16 deltas
GUARD = 2                                     # guard rows around every buffer of a span case

EDGE_LENS = (0, TILE - 1, TILE, TILE + 1, TILE + 13)      # an empty item, one frame short of a tile, a tile, one more, a second tile's part
EDGE_TILES = -(-max(EDGE_LENS) // TILE) + 1               # one more than the longest item needs


def span_operands(R, D, seed=0):
    """-> (x, d1, d2, buf) float32 [R + 2 GUARD][D]: the planes of one span launch with GUARD guard rows in front and behind."""
    rng = np.random.default_rng(2300 + seed + R + D)
    return tuple(rng.standard_normal((R + 2 * GUARD, D)).astype(np.float32) for _ in range(4))


def bf16_round(a):
    """float32 -> the nearest bfloat16 (ties to even), as float32."""
    u = np.ascontiguousarray(a, dtype=np.float32).view(np.uint32).astype(np.uint64)
    u = (u + 0x7FFF + ((u >> 16) & 1)) & 0xFFFF0000
    return u.astype(np.uint32).view(np.float32)


def span_expected(mode, x, d1, d2, buf):
    """The planes after one launch, from float32 numpy operations of the kernel's own: X = (x + d1) + d2 (d1 / d2 None: as given), MARK
    buf = X, DIFF buf = X - buf, APPLY x = X + buf -> (x, buf)."""
    X = x if d1 is None else (x + d1).astype(np.float32)
    X = X if d2 is None else (X + d2).astype(np.float32)
    if mode == MARK:
        return x, X.copy()
    if mode == DIFF:
        return x, (X - buf).astype(np.float32)
    return (X + buf).astype(np.float32), buf


def edge_planes(D, seed=29):
    """-> (d_new, d_prev) float32 [sum(EDGE_LENS)][D], the sequences back to back."""
    rng = np.random.default_rng(seed + D)
    R = sum(EDGE_LENS)
    d_new = rng.standard_normal((R, D)).astype(np.float32)
    return d_new, (d_new + 0.25 * rng.standard_normal((R, D))).astype(np.float32)
