"""Helpers of the N21 tests (guidance reuse and its drift report), no GPU needed to import.

``reuse_column`` restates the rule of DESIGN §8 N21 for one item from its N8 column, NOT through ``model_spec.guidance_mask``: the two meet
only in the tests.  ``drift_mirror`` restates the drift report's sums in the tile and thread order of cfg_drift_reduce_kernel, in numpy
float64 (every difference, product and add rounded on its own, as the kernel's); ``drift_plain`` is the same two sums as plain loops.
``ref_solve_reuse`` is a reference solver around the fp32 oracle that keeps the guidance difference itself."""
import numpy as np

TILE = 32             # VV_APG_TILE
THREADS = 256


def reuse_column(guided, k):
    """guided: 0 / 1 per evaluation (N8's rule for one item); -> 0 / 1 / 2 per evaluation: the j-th guided evaluation is computed (1) when
    j % k == 0 and reused (2) otherwise."""
    out, j = [], 0
    for v in guided:
        if not v:
            out.append(0)
            continue
        out.append(1 if j % k == 0 else 2)
        j += 1
    return out


def _tree(v):
    """The kernel's LDS tree over the 256 thread sums: red[t] += red[t + w], w = 128 ... 1."""
    v = v.copy()
    w = THREADS // 2
    while w > 0:
        v[:w] = v[:w] + v[w: 2 * w]
        w //= 2
    return v[0]


def drift_mirror(pc, pu, d_old):
    """(E2, N2) of one computed item as cfg_drift_reduce_kernel and the finishing kernel compute them.  pc, pu: float32 [frames][n_mel],
    the item's two predictions (n_mel a multiple of 4); d_old: the stored difference, float32 [frames][n_mel], or None (the item's first
    computed evaluation of the call: E2 = 0).  D_new = pc - pu is ONE fp32 subtraction (the value the stage kernel stores); then, in
    float64, d = D_new - d_old, d * d, sum + that, each rounded on its own.  Tiles of TILE frames from frame 0; float4 q of a tile on
    thread q % 256, its four elements in order; one tree per tile; the tiles added in ascending order from 0.0."""
    dn = (np.ascontiguousarray(pc, dtype=np.float32) - np.ascontiguousarray(pu, dtype=np.float32)).astype(np.float32)
    frames = dn.shape[0]
    E2 = N2 = np.float64(0.0)
    for f0 in range(0, frames, TILE):
        a = dn[f0: f0 + TILE].astype(np.float64).reshape(-1, 4)                  # float4 q of the tile = row q
        total = a.shape[0]
        rounds = -(-total // THREADS)
        sq = np.zeros((rounds * THREADS, 4))
        sq[:total] = a * a
        dd = np.zeros((rounds * THREADS, 4))
        if d_old is not None:
            p = np.ascontiguousarray(d_old, dtype=np.float32)[f0: f0 + TILE].astype(np.float64).reshape(-1, 4)
            d = a - p
            dd[:total] = d * d
        s1, s2 = np.zeros(THREADS), np.zeros(THREADS)
        for r in range(rounds):                                                   # thread t's float4s: q = t, t + 256, ...
            for j in range(4):
                s2 = s2 + sq[r * THREADS: (r + 1) * THREADS, j]                   # a thread past the tile's end adds +0.0: the same bits
                if d_old is not None:
                    s1 = s1 + dd[r * THREADS: (r + 1) * THREADS, j]
        E2 = E2 + _tree(s1)
        N2 = N2 + _tree(s2)
    return float(E2), float(N2)


def drift_plain(pc, pu, d_old):
    """The same two sums as plain float64 loops over the item's elements (row by row, left to right)."""
    dn = (np.asarray(pc, dtype=np.float32) - np.asarray(pu, dtype=np.float32)).astype(np.float32)
    e2 = n2 = 0.0
    for r in range(dn.shape[0]):
        for c in range(dn.shape[1]):
            v = float(dn[r, c])
            n2 += v * v
            if d_old is not None:
                d = v - float(d_old[r, c])
                e2 += d * d
    return e2, n2


def check_mask(mask, e0=0, e1=None):
    """What the steps entry refuses of a mask (list of rows of 0 / 1 / 2), restated: -> None, or the reason as a short word."""
    e1 = len(mask) if e1 is None else e1
    if any(v not in (0, 1, 2) for row in mask for v in row):
        return "value"
    if any(v == 2 for row in mask for v in row) and e0 != 0:
        return "step0"
    for b in range(len(mask[0])):
        seen = False
        for e in range(e0, e1):
            if mask[e][b] == 2 and not seen:
                return "2 before 1"
            seen = seen or mask[e][b] == 1
    return None


def ref_solve_reuse(orc, pre, x, method, nfe_step, g, col, report=None):
    """The reference solver with N21's rule, one item.  col[e] in 0 / 1 / 2 per evaluation e = step * s + stage: 0 -> slope pc; 1 -> both
    predictions, D = pc - pu kept, slope pc + D g; 2 -> pc alone, slope pc + D g with the kept D.  method: a Runge-Kutta name of
    model_spec.ODE_METHODS, or "ab2" / "ab3" (tests.multistep_util.newton_step on the float64 grid).  report: a list that receives per
    evaluation (E2, N2) as float64 torch sums -- (|D - D_kept|^2, |D|^2) where computed (E2 = 0 at the first), (0, 0) elsewhere."""
    from tests.multistep_util import grid64, newton_step
    from vietvoice_tts_amd.model_spec import ODE_MULTISTEP, ode_plan
    ropes = (pre["rope_cos_q"], pre["rope_sin_q"], pre["rope_cos_k"], pre["rope_sin_k"])
    kept = [None]

    def slope(e, t_e, xi):
        orc.t_grid = [t_e]
        pc = orc.dit_forward(xi, pre["cat_mel_text"], ropes, 0)
        rep = (0.0, 0.0)
        if col[e] == 1:
            pu = orc.dit_forward(xi, pre["cat_mel_text_drop"], ropes, 0)
            D = pc - pu
            rep = (0.0 if kept[0] is None else float(((D - kept[0]).double() ** 2).sum()), float((D.double() ** 2).sum()))
            kept[0] = D
            k = pc + D * g
        elif col[e] == 2:
            k = pc + kept[0] * g
        else:
            k = pc
        if report is not None:
            report.append(rep)
        return k

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
EDGE_LENS = (0, TILE - 1, TILE, TILE + 1, TILE + 13)      # an empty item, one frame short of a tile, a tile, one more, a second tile's part
EDGE_TILES = -(-max(EDGE_LENS) // TILE) + 1               # one more than the longest item needs
EDGE_COMPUTED = (1, 1, 0, 1, 1)                           # item 2 reuses at this evaluation: no unconditional rows, sums {0, 0}
EDGE_HAS_OLD = (1, 0, 1, 1, 1)                            # item 1 has nothing stored yet: d_buf is not read for it, E2 = 0


def edge_predictions(M, seed=23):
    """-> (pc, pu, d_old) float32 [sum(EDGE_LENS)][M], the items back to back."""
    rng = np.random.default_rng(seed + M)
    R = sum(EDGE_LENS)
    pc = rng.standard_normal((R, M)).astype(np.float32)
    pu = rng.standard_normal((R, M)).astype(np.float32)
    return pc, pu, (pc - pu + 0.25 * rng.standard_normal((R, M))).astype(np.float32)


REUSE_LOAD, REUSE_STORE = 1, 2                            # include/vvtts.h: VV_REUSE_LOAD, VV_REUSE_STORE


class ReuseStageCase:
    """One launch of the reuse form of the stage kernel, the operands and the float64 reference of tests/test_cfg_reuse_gpu.py
    (test_reuse_stage_against_float64) for any shape.  subset ``mixed``: item b computes and stores (b % 4 == 0), reuses (1), computes with
    its LOAD bit set as well (2: a mapped row is computed whatever LOAD says), is not guided (3).  ``none``: no unconditional row at all,
    even items reuse (item 0 with a STORE bit that stores nothing), odd ones are not guided.  ``plain``: every row computed, no store."""

    def __init__(self, name, method, stage, lens, N, n_mel, ldp, subset, seed=0, g=2.0, h=0.07):
        self.name, self.method, self.stage, self.lens, self.N, self.n_mel, self.ldp, self.subset = name, method, stage, tuple(lens), N, n_mel, ldp, subset
        self.seed, self.g, self.h = seed, g, h

    def ops(self):
        import torch
        from vietvoice_tts_amd.model_spec import ODE_METHODS
        a_t, b_t = ODE_METHODS[self.method]
        o = type("Ops", (), {})()
        gen = torch.Generator().manual_seed(2200 + self.seed)
        B, N, M, i = len(self.lens), self.N, self.n_mel, self.stage
        o.last = i == len(b_t) - 1
        o.coef = [np.float32(self.h * float(b_t[j] if o.last else a_t[i + 1][j])) for j in range(i + 1)]
        o.row_src = torch.cat([b * N + torch.arange(n) for b, n in enumerate(self.lens)]).to(torch.int32)
        o.item = torch.cat([torch.full((n,), b) for b, n in enumerate(self.lens)])
        Rc = o.Rc = int(o.row_src.numel())
        L, S = REUSE_LOAD, REUSE_STORE
        if self.subset == "mixed":
            o.modes = [(S, L, L, 0)[b % 4] for b in range(B)]
            mapped = (o.item % 4 == 0) | (o.item % 4 == 2)
        elif self.subset == "none":
            o.modes = [((L | S) if b == 0 else L) if b % 2 == 0 else 0 for b in range(B)]
            mapped = torch.zeros(Rc, dtype=torch.bool)
        else:
            o.modes = [0] * B
            mapped = torch.ones(Rc, dtype=torch.bool)
        o.Ru = int(mapped.sum())
        o.u_row = torch.full((Rc,), -1, dtype=torch.int32)
        o.u_row[mapped] = Rc + torch.arange(o.Ru, dtype=torch.int32)
        o.x = torch.randn(B * N, M, generator=gen)
        o.pred = torch.randn(Rc + o.Ru, self.ldp, generator=gen)
        o.d_old = torch.randn(Rc, M, generator=gen)
        o.k_prev = [torch.randn(Rc, M, generator=gen) for _ in range(i)]
        return o

    def ref(self, o):
        """-> dict(k, K, acc, mag: float64; guided, has_u, stores: row masks; want_d: d_buf after the launch)."""
        import torch
        M, g, i = self.n_mel, self.g, self.stage
        Rc = o.Rc
        has_u = o.u_row >= 0
        loads = (~has_u) & torch.tensor([bool(o.modes[int(b)] & REUSE_LOAD) for b in o.item], dtype=torch.bool)
        stores = has_u & torch.tensor([bool(o.modes[int(b)] & REUSE_STORE) for b in o.item], dtype=torch.bool)
        rs = o.row_src.long()
        pc32 = o.pred[:Rc, :M]
        pu32 = torch.zeros_like(pc32)
        pu32[has_u] = o.pred[o.u_row[has_u].long(), :M]
        pc = pc32.double()
        D = torch.where(has_u[:, None], pc - pu32.double(), o.d_old.double())
        guided = has_u | loads
        k = torch.where(guided[:, None], pc + D * g, pc)
        K = torch.where(guided[:, None], pc.abs() + abs(g) * D.abs(), pc.abs())
        acc, mag = o.x[rs].double(), o.x[rs].double().abs()
        for j in range(i):
            if o.coef[j] != 0:
                acc = acc + float(o.coef[j]) * o.k_prev[j].double()
                mag = mag + abs(float(o.coef[j])) * o.k_prev[j].double().abs()
        if o.coef[i] != 0:
            acc = acc + float(o.coef[i]) * k
            mag = mag + abs(float(o.coef[i])) * K
        want_d = o.d_old.clone()
        want_d[stores] = (pc32 - pu32)[stores]               # one fp32 subtraction, stored as it is
        return dict(k=k, K=K, acc=acc, mag=mag, guided=guided, has_u=has_u, stores=stores, want_d=want_d, pc32=pc32)


def reuse_stage_cases():
    """n_mel 4 and 100, ldp tight and + 4, 1 / 3 / 86 rows, the three subsets, a first, a middle and a last stage."""
    shapes = ((4, 4, (1,), 5), (4, 8, (1, 1, 1), 5), (100, 100, (1, 1, 1), 5), (100, 104, (40, 17, 29), 40), (4, 8, (40, 17, 29), 40))
    cs, n = [], 0
    for subset in ("mixed", "none", "plain"):
        for method, stage in (("euler", 0), ("rk4", 1), ("rk4", 3), ("heun2", 1)):
            M, ldp, lens, N = shapes[n % len(shapes)]
            cs.append(ReuseStageCase(f"reuse/{subset}/{method}{stage}/M{M}_ld{ldp}_Rc{sum(lens)}", method, stage, lens, N, M, ldp, subset, seed=n))
            n += 1
    return cs
