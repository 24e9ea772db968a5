"""Helpers of the N20 tests (Adams-Bashforth multistep solvers and the step report), no GPU needed to import.

``newton_step`` / ``ref_multistep`` are a reference solver written from the Newton form of the interpolating polynomial, NOT from
``model_spec.multistep_weights`` (which integrates the Lagrange basis in exact rationals): the two meet only in the tests.
``report_mirror`` restates the step report's sums in the tile and thread order of ode_diff_reduce_kernel, in numpy float64 (every
difference, product and add rounded on its own, as the kernel's)."""
import math

import numpy as np

TILE = 32             # VV_APG_TILE
THREADS = 256


def grid64(nfe_step, sway):
    """time_grid's float64 points, restated."""
    t = np.linspace(0.0, 1.0, nfe_step, dtype=np.float64)
    return t + sway * (np.cos(np.pi / 2 * t) - 1.0 + t)


def newton_step(x, t, n, f, q):
    """One Adams-Bashforth step of order min(q, n + 1) on the grid t: the polynomial through (t_n, f_n), (t_{n-1}, f_{n-1}), ... in
    Newton form f_n + f[n, n-1] s + f[n, n-1, n-2] s (s + a), a = h_{n-1}, integrated over s in [0, h_n]: the integrals of s and of
    s (s + a) are h^2 / 2 and h^3 / 3 + a h^2 / 2.  f: the slopes so far, f[-1] = f_n."""
    h = t[n + 1] - t[n]
    k = min(q, n + 1)
    x = x + h * f[-1]
    if k >= 2:
        a = t[n] - t[n - 1]
        d1 = (f[-1] - f[-2]) / a
        x = x + (h * h / 2.0) * d1
    if k >= 3:
        b = t[n - 1] - t[n - 2]
        d1_old = (f[-2] - f[-3]) / b
        d2 = (d1 - d1_old) / (a + b)
        x = x + (h ** 3 / 3.0 + a * h * h / 2.0) * d2
    return x


def integrate_scalar(t, q, fun, x0):
    """The reference solver on a scalar problem x' = fun(t, x)."""
    x, f = float(x0), []
    for n in range(len(t) - 1):
        f.append(fun(t[n], x))
        x = newton_step(x, t, n, f, q)
    return x


def ref_multistep(orc, pre, x, q, nfe_step, g, guided=None, apg=None, keep_slopes=None):
    """The reference solver around the oracle, one item.  The slope of step n is the combined velocity at (t_n, x_n): pc + (pc - pu) g,
    pc alone where guided[n] is false (N8) or g == 0, with the projected term when apg = (eta, cap) (N11: test_apg_gpu.ref_solve_apg's
    rule).  The DiT is evaluated at the fp32 value of t_n, as the plan's tables are; the steps are the float64 grid's."""
    t = grid64(nfe_step, orc.spec.sway_coef)
    ropes = (pre["rope_cos_q"], pre["rope_sin_q"], pre["rope_cos_k"], pre["rope_sin_k"])
    f = []
    for n in range(nfe_step - 1):
        t_e = float(np.float32(t[n]))
        orc.t_grid = [t_e]
        pc = orc.dit_forward(x, pre["cat_mel_text"], ropes, 0)
        if (guided is not None and not guided[n]) or g == 0.0:
            k = pc
        else:
            pu = orc.dit_forward(x, pre["cat_mel_text_drop"], ropes, 0)
            if apg is None:
                k = pc + (pc - pu) * g
            else:
                eta, r = apg
                D = pc - pu
                d = x + (1.0 - t_e) * pc
                S1, S2, S3 = float((D * d).double().sum()), float((d * d).double().sum()), float((D * D).double().sum())
                rms = (1.0 - t_e) * math.sqrt(S3 / D.numel())
                s = r / rms if (r is not None and rms > r) else 1.0
                Cc = 0.0 if S2 == 0.0 else g * s * (eta - 1.0) * S1 / S2
                k = pc + (g * s) * D + Cc * d
        f.append(k)
        if keep_slopes is not None:
            keep_slopes.append(k)
        x = newton_step(x, t, n, f, q)
        f = f[-3:]
    return x


# ------------------------------------------------------------------------------------------------ the step report
def _tree(v):
    """The kernel's LDS tree over the 256 thread sums: red[t] += red[t + w], w = 128 ... 1."""
    v = v.copy()
    w = THREADS // 2
    while w > 0:
        v[:w] = v[:w] + v[w: 2 * w]
        w //= 2
    return v[0]


def report_mirror(f, f_prev):
    """(D2, F2) of one item as ode_diff_reduce_kernel and its finishing kernel compute them: f, f_prev float32 [frames][n_mel] (f_prev
    None = step 0: D2 = 0), n_mel a multiple of 4.  Tiles of TILE frames from frame 0; inside a tile float4 q goes to thread q % 256,
    its four elements in order, each term v = (double) a - (double) b, then v * v, then sum + that, all rounded separately; one tree
    per tile; the tiles added in ascending order from 0.0."""
    f = np.ascontiguousarray(f, dtype=np.float32)
    frames, M = f.shape if f.ndim == 2 else (0, 0)
    D2 = F2 = np.float64(0.0)
    for f0 in range(0, frames, TILE):
        a = f[f0: f0 + TILE].astype(np.float64).reshape(-1, 4)                   # float4 q of the tile = row q
        total = a.shape[0]
        rounds = -(-total // THREADS)
        pad = np.zeros((rounds * THREADS, 4))
        sq = pad.copy()
        sq[:total] = a * a
        s2 = np.zeros(THREADS)
        s1 = np.zeros(THREADS)
        if f_prev is not None:
            p = np.ascontiguousarray(f_prev, dtype=np.float32)[f0: f0 + TILE].astype(np.float64).reshape(-1, 4)
            d = a - p
            dd = pad.copy()
            dd[:total] = d * d
        for r in range(rounds):                                                   # thread t's float4s: q = t, t + 256, ...
            for j in range(4):
                s2 = s2 + sq[r * THREADS: (r + 1) * THREADS, j]                   # a thread past the tile's end adds +0.0: the same bits
                if f_prev is not None:
                    s1 = s1 + dd[r * THREADS: (r + 1) * THREADS, j]
        D2 = D2 + _tree(s1)
        F2 = F2 + _tree(s2)
    return float(D2), float(F2)


def report_plain(f, f_prev):
    """The same two sums the plain way: float64 np.sum over the whole item."""
    f = np.asarray(f, dtype=np.float64)
    d2 = 0.0 if f_prev is None else float(np.sum((f - np.asarray(f_prev, dtype=np.float64)) ** 2))
    return d2, float(np.sum(f * f))


# the item lengths tools/elementwise_host_check.py and the device test share: an empty item, one frame short of a tile, a tile, one more, two
# tiles' worth of a part; with EDGE_TILES partials per item, one more than the longest needs
EDGE_LENS = (0, TILE - 1, TILE, TILE + 1, TILE + 13)
EDGE_TILES = -(-max(EDGE_LENS) // TILE) + 1


def edge_slopes(M, seed=22):
    """-> (f, f_prev) float32 [sum(EDGE_LENS)][M], the items back to back."""
    rng = np.random.default_rng(seed + M)
    R = sum(EDGE_LENS)
    f = rng.standard_normal((R, M)).astype(np.float32)
    return f, (f + 0.25 * rng.standard_normal((R, M))).astype(np.float32)
