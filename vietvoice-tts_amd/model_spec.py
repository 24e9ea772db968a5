"""Architecture constants of the synthesis hot path and the seeded synthetic weights.

The reference hides every one of these inside three ONNX graphs that are not in
the repository (reference: vietvoicetts/core/model.py:73-77, model_config.py:26);
only sample_rate=24000 / hop_length=256 / nfe_step=32 are visible
(model_config.py:29-34).  SURVEY.md section 8(a) "Model constants" fixes the
builder-chosen defaults restated here; nothing in the reference contradicts or
confirms them ("parity unpinned" against the real graphs).

Weights are synthetic: there is no network for checkpoints, so a seeded
generator produces variance-scaled tensors in torch-native layouts
(Linear [out,in], Conv1d [out,in/groups,k], ConvTranspose1d [in,out,k]).  The
HIP path and the CPU oracle consume the same dict.
"""
from __future__ import annotations

import json
import math
import numbers
from dataclasses import asdict, dataclass, field
from fractions import Fraction
from typing import Dict, NamedTuple, Optional, Tuple

import torch


@dataclass(frozen=True)
class ModelSpec:
    # mel front-end (preprocess graph)
    sample_rate: int = 24000
    n_fft: int = 1024
    win_length: int = 1024
    hop_length: int = 256
    n_mel: int = 100
    # acoustic model (transformer graph)
    dim: int = 1024
    depth: int = 22
    heads: int = 16
    head_dim: int = 64
    ff_mult: int = 2
    text_dim: int = 512
    text_layers: int = 4
    text_conv_k: int = 7
    text_ff_mult: int = 2
    vocab_size: int = 256          # text ids are 0..vocab_size-1; embedding has vocab_size+1 rows
    pos_conv_k: int = 31
    pos_conv_groups: int = 16
    time_freq_dim: int = 256
    cfg_strength: float = 2.0
    sway_coef: float = -1.0
    rope_theta: float = 10000.0
    # vocoder (decode graph)
    voc_pre_ch: int = 512
    voc_pre_k: int = 7
    voc_post_k: int = 7
    voc_up_rates: Tuple[int, ...] = (8, 8, 2, 2)
    voc_up_kernels: Tuple[int, ...] = (16, 16, 4, 4)
    voc_res_kernels: Tuple[int, ...] = (3, 7, 11)
    voc_res_dilations: Tuple[int, ...] = (1, 3, 5)
    voc_lrelu: float = 0.1
    # vocoder kind: "hifigan" (the voc_* generator above, default) or "vocos" (ConvNeXt backbone + ISTFT head)
    vocoder: str = "hifigan"
    vocos_dim: int = 512
    vocos_intermediate: int = 1536
    vocos_layers: int = 8
    vocos_embed_k: int = 7
    vocos_dw_k: int = 7
    vocos_ln_eps: float = 1e-6

    def __post_init__(self):
        assert self.heads * self.head_dim == self.dim
        assert self.head_dim == 64, "attention kernels are written for head_dim 64"
        assert self.dim // self.pos_conv_groups == 64, "pos-conv kernels assume 64 channels per group"
        prod = 1
        for r, k in zip(self.voc_up_rates, self.voc_up_kernels):
            assert k == 2 * r and r % 2 == 0
            prod *= r
        assert prod == self.hop_length
        assert self.n_mel == 100 or self.n_mel % 4 == 0
        assert self.vocoder in ("hifigan", "vocos"), self.vocoder
        if self.vocoder == "vocos":
            # the fp32 GEMMs of the backbone and the inverse DFT need N % 128 == 0 and K % 32 == 0
            assert self.vocos_dim % 128 == 0 and 0 < self.vocos_dim <= 1024 and self.vocos_intermediate % 128 == 0
            assert self.vocos_layers >= 1 and self.vocos_embed_k % 2 == 1 and self.vocos_dw_k % 2 == 1
            assert self.win_length == self.n_fft and self.n_fft % 128 == 0 and self.n_fft % self.hop_length == 0
            assert self.n_fft // self.hop_length <= 8

    def pcm_samples(self, frames: int) -> int:
        """Output samples the vocoder makes of ``frames`` mel frames: hop * T (HiFi-GAN), hop * (T - 1) (Vocos, centred ISTFT)."""
        if self.vocoder == "vocos":
            return self.hop_length * max(int(frames) - 1, 0)
        return self.hop_length * max(int(frames), 0)

    @property
    def cat_dim(self) -> int:
        return 2 * self.n_mel + self.text_dim

    @property
    def cond_dim(self) -> int:
        return self.n_mel + self.text_dim

    def voc_channels(self):
        ch = [self.voc_pre_ch]
        for _ in self.voc_up_rates:
            ch.append(ch[-1] // 2)
        return ch

    def to_json(self) -> str:
        return json.dumps(asdict(self))

    @classmethod
    def from_json(cls, s: str) -> "ModelSpec":
        d = json.loads(s)
        for k in ("voc_up_rates", "voc_up_kernels", "voc_res_kernels", "voc_res_dilations"):
            d[k] = tuple(d[k])                  # (files written before the vocoder kind existed load as HiFi-GAN specs)
        return cls(**d)

    @classmethod
    def full(cls) -> "ModelSpec":
        return cls()

    @classmethod
    def tiny(cls) -> "ModelSpec":
        """Small dims for oracle-speed parity tests; same topology, same kernels."""
        return cls(dim=128, depth=2, heads=2, text_dim=128, text_layers=2, vocab_size=64,
                   pos_conv_groups=2, voc_pre_ch=64)

    @classmethod
    def small(cls) -> "ModelSpec":
        """Mid-size config (all tile paths exercised, oracle still seconds)."""
        return cls(dim=256, depth=3, heads=4, text_dim=128, text_layers=2, vocab_size=64,
                   pos_conv_groups=4, voc_pre_ch=128)

    def with_vocos(self, dim: int = 512, intermediate: int = 1536, layers: int = 8) -> "ModelSpec":
        from dataclasses import replace
        return replace(self, vocoder="vocos", vocos_dim=dim, vocos_intermediate=intermediate, vocos_layers=layers)

    @classmethod
    def full_vocos(cls) -> "ModelSpec":
        """The full model with the Vocos decoder of charactr/vocos-mel-24khz (512 / 1536 / 8 layers, k 7)."""
        return cls.full().with_vocos()

    @classmethod
    def small_vocos(cls) -> "ModelSpec":
        return cls.small().with_vocos(256, 768, 4)

    @classmethod
    def tiny_vocos(cls) -> "ModelSpec":
        return cls.tiny().with_vocos(128, 384, 2)


def time_grid(nfe_step: int, sway_coef: float) -> Tuple[torch.Tensor, torch.Tensor]:
    """ODE time grid: nfe_step points on [0,1] with sway sampling, and the Euler deltas.

    The reference evaluates the transformer ``len(range(0, nfe_step-1, fuse_nfe))``
    times (core/tts_engine.py:157-159), i.e. nfe_step-1 = 31 Euler steps at defaults.
    Returns (t[:-1], dt) each of length nfe_step-1, float64 computed then cast to fp32.
    """
    t = torch.linspace(0.0, 1.0, nfe_step, dtype=torch.float64)
    t = t + sway_coef * (torch.cos(math.pi / 2 * t) - 1.0 + t)
    dt = t[1:] - t[:-1]
    return t[:-1].to(torch.float32), dt.to(torch.float32)


# Explicit Runge-Kutta methods of the flow-ODE sampler: name -> (a, b), a strictly lower triangular, nodes
# c_i = sum_j a[i][j].  Exact fractions; "rk4" is the 3/8 rule (torchdiffeq's fixed-grid rk4).
_F = Fraction
ODE_METHODS: Dict[str, Tuple[Tuple[Tuple[Fraction, ...], ...], Tuple[Fraction, ...]]] = {
    "euler": (((_F(0),),), (_F(1),)),
    "midpoint": (((_F(0), _F(0)), (_F(1, 2), _F(0))), (_F(0), _F(1))),
    "heun2": (((_F(0), _F(0)), (_F(1), _F(0))), (_F(1, 2), _F(1, 2))),
    "heun3": (((_F(0), _F(0), _F(0)), (_F(1, 3), _F(0), _F(0)), (_F(0), _F(2, 3), _F(0))), (_F(1, 4), _F(0), _F(3, 4))),
    "rk4": (((_F(0), _F(0), _F(0), _F(0)), (_F(1, 3), _F(0), _F(0), _F(0)), (_F(-1, 3), _F(1), _F(0), _F(0)), (_F(1), _F(-1), _F(1), _F(0))),
            (_F(1, 8), _F(3, 8), _F(3, 8), _F(1, 8))),
}
ODE_MAX_STAGES = 4
ODE_MAX_EVALS = 512


def ode_tableau(method) -> Tuple[Tuple[Tuple[float, ...], ...], Tuple[float, ...]]:
    """A method name of ODE_METHODS, or a custom tableau (a, b), as validated float64 rows: 1 to 4 stages, a square and strictly
    lower triangular, finite, |sum b - 1| < 1e-6.  ValueError otherwise."""
    if isinstance(method, str):
        if method not in ODE_METHODS:
            raise ValueError(f"ode_method must be one of {sorted(ODE_METHODS)} or a tableau (a, b), got {method!r}")
        a, b = ODE_METHODS[method]
    else:
        try:
            a, b = method
            a, b = tuple(tuple(r) for r in a), tuple(b)
        except (TypeError, ValueError):
            raise ValueError("a custom ode_method is a pair (a, b): a [s][s] strictly lower triangular, b [s]") from None
    s = len(b)
    if not 1 <= s <= ODE_MAX_STAGES or len(a) != s or any(len(r) != s for r in a):
        raise ValueError(f"an ODE tableau has 1 to {ODE_MAX_STAGES} stages, a [s][s] and b [s]")
    af = tuple(tuple(float(v) for v in r) for r in a)
    bf = tuple(float(v) for v in b)
    if not all(math.isfinite(v) for r in af for v in r) or not all(math.isfinite(v) for v in bf):
        raise ValueError("an ODE tableau must be finite")
    if any(af[i][j] != 0.0 for i in range(s) for j in range(i, s)):
        raise ValueError("an ODE tableau must be strictly lower triangular (explicit method)")
    if not abs(sum(bf) - 1.0) < 1e-6:
        raise ValueError("the weights b of an ODE tableau must sum to 1")
    return af, bf


class OdePlan(NamedTuple):
    t: torch.Tensor          # fp32 [n_steps * s]: evaluation times t_n + c_i h_n, step-major (row n * s + i)
    dt: torch.Tensor         # fp32 [n_steps]: h_n, exactly time_grid's
    a: Tuple[Tuple[float, ...], ...]
    b: Tuple[float, ...]
    s: int
    beta: Optional[Tuple[Tuple[float, ...], ...]] = None     # N20, a multistep plan only: multistep_weights' rows [n_steps][q]


# Adams-Bashforth multistep methods of the sampler: name -> q, the slopes a step combines (the fresh one and q - 1 kept
# from the steps before).  One DiT evaluation per step, as Euler.
ODE_MULTISTEP: Dict[str, int] = {"ab2": 2, "ab3": 3}


def _grid64(nfe_step: int, sway_coef: float) -> torch.Tensor:
    t = torch.linspace(0.0, 1.0, nfe_step, dtype=torch.float64)
    return t + sway_coef * (torch.cos(math.pi / 2 * t) - 1.0 + t)


def multistep_weights(t64, q: int) -> Tuple[Tuple[float, ...], ...]:
    """The variable-step Adams-Bashforth weights on the grid ``t64`` (float64 points t_0 < ... < t_n): float64 rows [n_steps][q], j = 0
    the newest slope, with x_{n+1} = x_n + h_n sum_j beta[n][j] f_{n-j}.  beta[n][j] is the integral over [t_n, t_{n+1}] of the
    Lagrange basis polynomial of node t_{n-j} among the nodes t_n, ..., t_{n-k+1}, divided by h_n, k = min(q, n + 1) the order used at
    step n (step 0 is Euler, step 1 AB2, from step 2 on AB3 when q = 3); the entries j >= k are 0.  Computed in exact rationals from the
    float64 grid and rounded once.  A uniform grid gives (1), (3/2, -1/2), (23/12, -4/3, 5/12)."""
    q = int(q)
    if not 1 <= q <= 3:
        raise ValueError("multistep_weights: q must be 1, 2 or 3")
    tq = [Fraction(float(v)) for v in t64]
    if len(tq) < 2 or any(tq[i + 1] <= tq[i] for i in range(len(tq) - 1)):
        raise ValueError("multistep_weights: the grid must have two points at least and increase strictly")
    rows = []
    for n in range(len(tq) - 1):
        k = min(q, n + 1)
        h = tq[n + 1] - tq[n]
        nodes = [tq[n - j] - tq[n] for j in range(k)]           # relative to t_n: 0, -h_{n-1}, -(h_{n-1} + h_{n-2})
        row = []
        for j in range(k):
            poly = [Fraction(1)]                                # coefficients of prod_{m != j} (s - nodes[m]), ascending powers of s
            den = Fraction(1)
            for m in range(k):
                if m == j:
                    continue
                poly = [(poly[i - 1] if i > 0 else 0) - nodes[m] * (poly[i] if i < len(poly) else 0) for i in range(len(poly) + 1)]
                den *= nodes[j] - nodes[m]
            integral = sum(cf * h ** (i + 1) / (i + 1) for i, cf in enumerate(poly))
            row.append(float(integral / den / h))
        rows.append(tuple(row + [0.0] * (q - k)))
    return tuple(rows)


def check_cfg_zero_init(k, nfe_step: int) -> int:
    """N24 zero-init (Fan et al. 2025): the number K of leading ODE steps that are skipped -- the state stays the start noise up to t_K.  An
    integer with 0 <= K <= nfe_step - 2 (one step at least is left); ValueError for a bool, a non-integer and a K outside that range."""
    if isinstance(k, bool) or not isinstance(k, numbers.Integral):
        raise ValueError("cfg_zero_init must be an integer >= 0")
    if int(k) != 0 and not 0 <= int(k) <= int(nfe_step) - 2:            # 0 is "off" on any grid
        raise ValueError(f"cfg_zero_init must satisfy 0 <= K <= nfe_step - 2 = {int(nfe_step) - 2}, got {int(k)}")
    return int(k)


def ode_plan(nfe_step: int, sway_coef: float, method="euler", skip: int = 0) -> OdePlan:
    """The sampler's plan on time_grid's grid: ``nfe_step`` points, ``nfe_step - 1`` ODE steps of ``s`` evaluations each at
    t_n + c_i h_n (float64, clamped to [0, 1], then fp32 -- like time_grid).  ``ode_plan(n, sway, "euler")`` is time_grid bit for bit.

    A name of ODE_MULTISTEP (N20, "ab2" | "ab3"): the plan of an Adams-Bashforth method -- ``t``, ``dt``, ``a``, ``b`` and ``s`` = 1 are
    Euler's bit for bit (one evaluation per step, at t_n), and ``beta`` holds multistep_weights' rows on the float64 grid.  No start-up
    step with extra evaluations is built: step 0 is an Euler step and step 1 of "ab3" an AB2 step.  With that start "ab3" has global
    order 3 on the model's own sway grid (coefficient -1: the first step is O(n^-2) long, so its O(h_0^2) error is O(n^-4)) and order
    2 on a uniform grid; "ab2" has order 2 on both.

    ``skip`` = K (N24 zero-init, check_cfg_zero_init): the plan of the steps K ... nfe_step - 2 of the same grid -- the state stays the start
    noise up to t_K.  ``t``, ``dt`` are the rows of the full plan from step K on, and ``beta`` the variable-step weights of the grid points
    from K on, so the order ramp starts at the first step that exists.  skip = 0 is the full plan bit for bit."""
    skip = check_cfg_zero_init(skip, nfe_step)
    if isinstance(method, str) and method in ODE_MULTISTEP:
        e = ode_plan(nfe_step, sway_coef, "euler", skip)
        return e._replace(beta=multistep_weights(_grid64(nfe_step, sway_coef)[skip:], ODE_MULTISTEP[method]))
    a, b = ode_tableau(method)
    s = len(b)
    t = torch.linspace(0.0, 1.0, nfe_step, dtype=torch.float64)
    t = t + sway_coef * (torch.cos(math.pi / 2 * t) - 1.0 + t)
    dt = t[1:] - t[:-1]
    c = torch.tensor([sum(r) for r in a], dtype=torch.float64)
    te = t[:-1, None] + c[None, :] * dt[:, None]
    if s > 1:
        te = te.clamp(0.0, 1.0)
    return OdePlan(te[skip:].reshape(-1).to(torch.float32), dt[skip:].to(torch.float32), a, b, s)


def check_cfg_interval(interval) -> Optional[Tuple[float, float]]:
    """A guidance interval (lo, hi) as two floats with 0 <= lo <= hi <= 1, or None (guidance everywhere); ValueError otherwise."""
    if interval is None:
        return None
    try:
        lo, hi = (float(v) for v in interval)
    except (TypeError, ValueError):
        raise ValueError("cfg_interval must be None or a pair (lo, hi)") from None
    if not (math.isfinite(lo) and math.isfinite(hi) and 0.0 <= lo <= hi <= 1.0):
        raise ValueError("cfg_interval must satisfy 0 <= lo <= hi <= 1 (finite)")
    return lo, hi


def check_cfg_reuse(v) -> Optional[int]:
    """N21 guidance reuse of one item: None, or an integer k >= 1 -- the unconditional branch runs at every k-th guided evaluation.  Returns
    the integer (1 = off, as None); ValueError for a bool, a non-integer and k < 1."""
    if v is None:
        return None
    if isinstance(v, bool) or not isinstance(v, numbers.Integral) or int(v) < 1:
        raise ValueError("cfg_reuse must be an integer >= 1 or None")
    return int(v)


def guidance_mask(plan: OdePlan, interval, strengths, reuse=None) -> Optional[torch.Tensor]:
    """N8 limited-interval guidance (Kynkaanniemi et al. 2024): uint8 [n_evals][B], row e = step * s + stage as in ``plan.t``,
    guided(b, e) = (interval is None or lo <= float(plan.t[e]) <= hi) and strengths[b] != 0 -- both edges inclusive, the fp32 time
    of the plan compared as a double.  ``interval``: None or one (lo, hi) for every item, or a sequence of B of them, one per item.
    Returns None when every item is guided at every evaluation (the unmasked call).

    ``reuse`` (N21 guidance reuse): None, one integer k >= 1 for every item, or a sequence of B of them (check_cfg_reuse); None and 1 are
    "off".  Off for every item: exactly the above.  Otherwise the mask has three values -- 0 = not guided, 1 = guided and the unconditional
    prediction COMPUTED, 2 = guided and the stored guidance difference REUSED: the guided evaluations of item b, in ascending e, are
    numbered j = 0, 1, 2, ... and evaluation j is computed when j % k_b == 0, reused otherwise.  The count runs over evaluations (the
    stages of a Runge-Kutta step count one each) and simply continues across a gap of the interval, so the first guided evaluation of an
    item is always computed."""
    g = [float(v) for v in strengths]
    B = len(g)
    one = interval is None or (len(interval) == 2 and all(isinstance(v, numbers.Real) for v in interval))
    ivals = [check_cfg_interval(interval)] * B if one else [check_cfg_interval(v) for v in interval]
    if len(ivals) != B:
        raise ValueError("guidance_mask: one interval per item")
    if reuse is None or isinstance(reuse, (bool, numbers.Number, str)):
        ks = [check_cfg_reuse(reuse)] * B
    else:
        ks = [check_cfg_reuse(v) for v in reuse]
    if len(ks) != B:
        raise ValueError("guidance_mask: one cfg_reuse per item")
    t = [float(v) for v in plan.t]
    mask = torch.zeros((len(t), B), dtype=torch.uint8)
    for b in range(B):
        if g[b] == 0.0:
            continue
        for e, te in enumerate(t):
            mask[e, b] = 1 if ivals[b] is None or ivals[b][0] <= te <= ivals[b][1] else 0
    if all(k is None or k == 1 for k in ks):
        return None if bool(mask.all()) else mask
    for b in range(B):
        k = ks[b] or 1
        j = 0
        for e in range(len(t)):
            if mask[e, b]:
                mask[e, b] = 1 if j % k == 0 else 2
                j += 1
    return mask


def check_block_cache(value, depth: int) -> Optional[Tuple[int, int, int]]:
    """N23 block caching: None, or (first, last, every) -- the span [first, last) of the ``depth`` DiT blocks and the period of the full
    evaluations -- as three integers with 0 <= first < last <= depth and every >= 1 (1 = no block is ever skipped).  A list (from JSON)
    becomes the tuple.  ValueError for anything else."""
    if value is None:
        return None
    try:
        vals = tuple(value)
    except TypeError:
        raise ValueError("block_cache must be None or (first, last, every)") from None
    if len(vals) != 3 or any(isinstance(v, bool) or not isinstance(v, numbers.Integral) for v in vals):
        raise ValueError("block_cache must be None or three integers (first, last, every)")
    first, last, every = (int(v) for v in vals)
    if not 0 <= first < last <= int(depth):
        raise ValueError(f"block_cache: the span must satisfy 0 <= first < last <= depth = {int(depth)}, got [{first}, {last})")
    if every < 1:
        raise ValueError("block_cache: every must be >= 1")
    return first, last, every


BLOCK_FULL, BLOCK_STORE, BLOCK_LIGHT = 0, 1, 2      # VV_BLOCK_* of include/vvtts.h: an evaluation's mode under block caching (N23)


def block_cache_schedule(plan: OdePlan, every: int, interval=None, report: bool = False) -> torch.Tensor:
    """N23: the mode of every evaluation of ``plan`` under block caching, uint8 [n_evals], row e = step * s + stage as in ``plan.t``.
    Evaluation e is a candidate when ``interval`` is None or lo <= float(plan.t[e]) <= hi (both edges inclusive, the fp32 time compared
    as a double, as guidance_mask does); candidate number j (in ascending e) is LIGHT (2) iff every > 1 and j % every != 0; every other
    evaluation is FULL, and a FULL evaluation STOREs (1) iff the next evaluation is LIGHT or ``report`` is on.  The first candidate is
    always full, so a LIGHT evaluation always has a store in front of it; every = 1 skips nothing."""
    if isinstance(every, bool) or not isinstance(every, numbers.Integral) or int(every) < 1:
        raise ValueError("block_cache_schedule: every must be an integer >= 1")
    every = int(every)
    iv = check_cfg_interval(interval)
    t = [float(v) for v in plan.t]
    assert all(t[e] <= t[e + 1] for e in range(len(t) - 1)), "the evaluation times of a plan do not decrease: the candidates are contiguous"
    modes = torch.zeros((len(t),), dtype=torch.uint8)
    j = 0
    for e, te in enumerate(t):
        if iv is None or iv[0] <= te <= iv[1]:
            if every > 1 and j % every != 0:
                modes[e] = BLOCK_LIGHT
            j += 1
    for e in range(len(t)):
        if modes[e] == BLOCK_FULL and (report or (e + 1 < len(t) and modes[e + 1] == BLOCK_LIGHT)):
            modes[e] = BLOCK_STORE
    return modes


def check_apg(eta, norm) -> Optional[Tuple[float, Optional[float]]]:
    """N11 projected guidance (Sadat et al. 2025) of one item: ``eta`` scales the part of the guidance difference parallel to the
    conditional data estimate (None = 1, plain CFG's), ``norm`` caps the RMS of the data-space difference (None = no cap).  Returns
    (eta, norm) as floats, or None when the pair is "off" (eta None or 1 and no cap: the plain rule).  ValueError for an eta that is
    not finite and a norm that is not finite and > 0."""
    def num(v, what):
        if isinstance(v, bool) or not isinstance(v, numbers.Real):
            raise ValueError(f"{what} must be a number or None")
        return float(v)
    e = 1.0 if eta is None else num(eta, "apg_eta")
    if not math.isfinite(e):
        raise ValueError("apg_eta must be finite or None")
    r = None if norm is None else num(norm, "apg_norm")
    if r is not None and not (math.isfinite(r) and r > 0.0):
        raise ValueError("apg_norm must be finite and > 0, or None")
    return None if (e == 1.0 and r is None) else (e, r)


def check_cfg_norm(zero_star, rescale) -> Optional[Tuple[bool, float]]:
    """N24 of one item: ``zero_star`` turns on the optimised scale s* = <p_c, p_u> / <p_u, p_u> of CFG-Zero* (Fan et al. 2025; None or False
    = off), ``rescale`` is the guidance rescale phi of Lin et al. 2024 applied to the guided velocity (None = off, else 0 < phi <= 1).
    Returns (zero_star, phi) with phi = 0.0 for "no rescale", or None when both are off (the plain rule).  ValueError for a zero_star that is
    not a bool and a rescale that is not a finite number in (0, 1]."""
    if zero_star is not None and not isinstance(zero_star, bool):
        raise ValueError("cfg_zero_star must be a bool or None")
    phi = 0.0
    if rescale is not None:
        if isinstance(rescale, bool) or not isinstance(rescale, numbers.Real):
            raise ValueError("cfg_rescale must be a number or None")
        phi = float(rescale)
        if not (math.isfinite(phi) and 0.0 < phi <= 1.0):
            raise ValueError("cfg_rescale must satisfy 0 < phi <= 1, or be None")
    return None if (not zero_star and phi == 0.0) else (bool(zero_star), phi)


def check_cfg_norm_combination(zero_star, rescale, apg_eta, apg_norm, cfg_reuse, block_cache) -> None:
    """N24: what one item's CFG-Zero* / rescale is never combined with, each refusal a sentence of its own (ModelConfig, submit and the
    engine all raise these): projected guidance, guidance reuse, block caching.  Nothing is raised for an item with both options off."""
    if check_cfg_norm(zero_star, rescale) is None:
        return
    if check_apg(apg_eta, apg_norm) is not None:
        raise ValueError("cfg_zero_star / cfg_rescale cannot be combined with apg_eta / apg_norm (both rewrite the guided slope from the same two predictions)")
    if (cfg_reuse or 1) > 1:
        raise ValueError("cfg_zero_star / cfg_rescale cannot be combined with cfg_reuse > 1 (a reused evaluation has no unconditional prediction to measure)")
    if block_cache is not None:
        raise ValueError("cfg_zero_star / cfg_rescale cannot be combined with block_cache (the block-cache entry has no guided form)")


NOISE_SOURCES = ("host", "device")      # ModelConfig.noise_source: torch.randn on the host (default) | vv_noise_fill on the device (N9)


def noise_keys(seed: int, serial: int, n_chunks: int, edit: bool = False):
    """N9: the Philox keys of one call's chunks, numpy uint64 [n_chunks][2] = {seed, stream} -- the rows vv_noise_fill reads, and the
    ONLY place the stream convention lives.  stream = (serial << 16) | chunk, bit 63 set for a speech edit: ``serial`` is the call's
    (engine) or the request's (front end) serial, 0 <= serial < 2^47, ``chunk`` the chunk's index inside the call, n_chunks <= 65536.
    ``seed``: any integer, taken modulo 2^64.  ValueError outside those ranges."""
    import numpy as np
    seed, serial, n_chunks = int(seed), int(serial), int(n_chunks)
    if not 0 <= n_chunks <= 65536:
        raise ValueError(f"noise_keys: {n_chunks} chunks do not fit the 16 chunk bits of a stream id")
    if not 0 <= serial < (1 << 47):
        raise ValueError(f"noise_keys: serial {serial} does not fit 47 bits")
    keys = np.empty((n_chunks, 2), dtype=np.uint64)
    keys[:, 0] = np.uint64(seed & ((1 << 64) - 1))
    keys[:, 1] = np.arange(n_chunks, dtype=np.uint64) | np.uint64((serial << 16) | ((1 << 63) if edit else 0))
    return keys


def mel_filterbank(spec: ModelSpec) -> torch.Tensor:
    """HTK-scale triangular mel filterbank, no norm: (n_fft//2+1, n_mel) fp32."""
    n_freqs = spec.n_fft // 2 + 1
    f_max = spec.sample_rate / 2.0
    all_freqs = torch.linspace(0, spec.sample_rate // 2, n_freqs, dtype=torch.float64)
    m_min = 2595.0 * math.log10(1.0 + 0.0 / 700.0)
    m_max = 2595.0 * math.log10(1.0 + f_max / 700.0)
    m_pts = torch.linspace(m_min, m_max, spec.n_mel + 2, dtype=torch.float64)
    f_pts = 700.0 * (10.0 ** (m_pts / 2595.0) - 1.0)
    f_diff = f_pts[1:] - f_pts[:-1]
    slopes = f_pts.unsqueeze(0) - all_freqs.unsqueeze(1)
    down = (-1.0 * slopes[:, :-2]) / f_diff[:-1]
    up = slopes[:, 2:] / f_diff[1:]
    fb = torch.clamp(torch.minimum(down, up), min=0.0)
    return fb.to(torch.float32).contiguous()


def weight_shapes(spec: ModelSpec) -> Dict[str, Tuple[Tuple[int, ...], float]]:
    """name -> (shape, std).  std==0.0 means zeros; std<0 means constant |std| (ones-like)."""
    D, Dt, M = spec.dim, spec.text_dim, spec.n_mel
    sh: Dict[str, Tuple[Tuple[int, ...], float]] = {}

    def lin(name, out_f, in_f, gain=1.0, bias_std=0.02):
        sh[name + ".weight"] = ((out_f, in_f), gain / math.sqrt(in_f))
        sh[name + ".bias"] = ((out_f,), bias_std)

    # ---- text embedding + ConvNeXtV2 blocks
    sh["text.embed.weight"] = ((spec.vocab_size + 1, Dt), 1.0)
    for i in range(spec.text_layers):
        p = f"text.blocks.{i}"
        sh[p + ".dwconv.weight"] = ((Dt, 1, spec.text_conv_k), 1.0 / math.sqrt(spec.text_conv_k))
        sh[p + ".dwconv.bias"] = ((Dt,), 0.02)
        sh[p + ".norm.weight"] = ((Dt,), -1.0)
        sh[p + ".norm.bias"] = ((Dt,), 0.02)
        lin(p + ".pwconv1", Dt * spec.text_ff_mult, Dt, gain=1.4)
        sh[p + ".grn.gamma"] = ((Dt * spec.text_ff_mult,), 0.3)
        sh[p + ".grn.beta"] = ((Dt * spec.text_ff_mult,), 0.02)
        lin(p + ".pwconv2", Dt, Dt * spec.text_ff_mult, gain=0.5)
    # ---- input embedding
    lin("input.proj", D, spec.cat_dim)
    cg = D // spec.pos_conv_groups
    for j in (1, 2):
        sh[f"input.pos_conv{j}.weight"] = ((D, cg, spec.pos_conv_k), 1.0 / math.sqrt(cg * spec.pos_conv_k))
        sh[f"input.pos_conv{j}.bias"] = ((D,), 0.02)
    # ---- time embedding
    lin("time.mlp1", D, spec.time_freq_dim)
    lin("time.mlp2", D, D)
    # ---- DiT blocks
    for i in range(spec.depth):
        p = f"blocks.{i}"
        lin(p + ".adaln", 6 * D, D, gain=0.6, bias_std=0.05)
        lin(p + ".attn.qkv", 3 * D, D)
        lin(p + ".attn.out", D, D, gain=0.7)
        lin(p + ".ff1", D * spec.ff_mult, D, gain=1.4)
        lin(p + ".ff2", D, D * spec.ff_mult, gain=0.7)
    lin("final.adaln", 2 * D, D, gain=0.6, bias_std=0.05)
    lin("final.proj", M, D, gain=1.0)
    if spec.vocoder == "vocos":
        # ---- Vocos decoder, after every acoustic tensor (the per-tensor seed index of the acoustic weights is that of the HiFi-GAN
        # spec).  Scaled so that a seeded N(0, 1) mel state gives a waveform peak of a few tenths: log-magnitudes ~ N(1.6, 0.3^2)
        V, I, n_out = spec.vocos_dim, spec.vocos_intermediate, spec.n_fft + 2
        sh["voc.embed.weight"] = ((V, M, spec.vocos_embed_k), 1.0 / math.sqrt(M * spec.vocos_embed_k))
        sh["voc.embed.bias"] = ((V,), 0.02)
        sh["voc.norm.weight"] = ((V,), -1.0)
        sh["voc.norm.bias"] = ((V,), 0.02)
        for i in range(spec.vocos_layers):
            p = f"voc.blocks.{i}"
            sh[p + ".dwconv.weight"] = ((V, 1, spec.vocos_dw_k), 1.0 / math.sqrt(spec.vocos_dw_k))
            sh[p + ".dwconv.bias"] = ((V,), 0.02)
            sh[p + ".norm.weight"] = ((V,), -1.0)
            sh[p + ".norm.bias"] = ((V,), 0.02)
            lin(p + ".pwconv1", I, V, gain=1.4)
            lin(p + ".pwconv2", V, I, gain=0.7)
            sh[p + ".gamma"] = ((V,), -1.0 / spec.vocos_layers)
        sh["voc.final_norm.weight"] = ((V,), -1.0)
        sh["voc.final_norm.bias"] = ((V,), 0.02)
        lin("voc.head", n_out, V, gain=0.3, bias_std=-1.6)
        return sh
    # ---- vocoder
    ch = spec.voc_channels()
    sh["voc.pre.weight"] = ((ch[0], M, spec.voc_pre_k), 1.0 / math.sqrt(M * spec.voc_pre_k) / 3.0)
    sh["voc.pre.bias"] = ((ch[0],), 0.02)
    for s, (r, k) in enumerate(zip(spec.voc_up_rates, spec.voc_up_kernels)):
        cin, cout = ch[s], ch[s + 1]
        # each output sample sees 2*cin taps (k = 2*stride)
        sh[f"voc.up.{s}.weight"] = ((cin, cout, k), 1.4 / math.sqrt(2 * cin))
        sh[f"voc.up.{s}.bias"] = ((cout,), 0.02)
        for a, rk in enumerate(spec.voc_res_kernels):
            for b, _d in enumerate(spec.voc_res_dilations):
                q = f"voc.res.{s}.{a}.{b}"
                sh[q + ".conv1.weight"] = ((cout, cout, rk), 1.4 / math.sqrt(cout * rk))
                sh[q + ".conv1.bias"] = ((cout,), 0.02)
                sh[q + ".conv2.weight"] = ((cout, cout, rk), 0.45 / math.sqrt(cout * rk))
                sh[q + ".conv2.bias"] = ((cout,), 0.02)
    sh["voc.post.weight"] = ((1, ch[-1], spec.voc_post_k), 0.35 / math.sqrt(ch[-1] * spec.voc_post_k))
    sh["voc.post.bias"] = ((1,), 0.0)
    return sh


def make_synthetic_weights(spec: ModelSpec, seed: int = 9527) -> Dict[str, torch.Tensor]:
    """Seeded fp32 weights (CPU).  One generator per tensor so any subset is reproducible."""
    out: Dict[str, torch.Tensor] = {}
    for idx, (name, (shape, std)) in enumerate(weight_shapes(spec).items()):
        if std < 0:
            g = torch.Generator().manual_seed(seed * 1000003 + idx)
            t = torch.full(shape, -std, dtype=torch.float32) + 0.05 * torch.randn(shape, generator=g)
        elif std == 0.0:
            t = torch.zeros(shape, dtype=torch.float32)
        else:
            g = torch.Generator().manual_seed(seed * 1000003 + idx)
            t = torch.randn(shape, generator=g, dtype=torch.float32) * std
        out[name] = t
    return out


def count_params(spec: ModelSpec) -> Dict[str, int]:
    tot = {"acoustic": 0, "vocoder": 0}
    for name, (shape, _s) in weight_shapes(spec).items():
        n = 1
        for d in shape:
            n *= d
        tot["vocoder" if name.startswith("voc.") else "acoustic"] += n
    return tot
