"""-m gpu: N23, block caching: a span of DiT blocks is skipped at chosen evaluations; its contribution to the residual
stream, stored at the full evaluation before, is added back instead.

The span kernel against torch bit for bit; all-zero and store-only schedules through the new entry against vv_transformer_steps_ex bit
for bit; fp32 runs against a reference solver written from the oracle's parts (block_cache_util.ref_solve_cached); the structure
properties bit for bit; the launches and flops the profiler counts; the report against its numpy mirror bit for bit; the refusals; the
engine level.  The model is the tiny one with FOUR blocks, built here; the shared hip_tiny engines only lend their context to the
single-kernel entries.  No test claims a quality gain or loss: the synthetic model's blocks are arbitrary."""
import ctypes as C
import dataclasses

import numpy as np
import pytest
import torch

from tests import block_cache_util as U
from tests.test_e2e_gpu import make_batch

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
LONG = "Hôm nay trời đẹp quá, chúng ta cùng nhau đi dạo quanh hồ nhé. " * 4
# three ragged items of 31, 32 and 45 frames: below, at and above a VV_APG_TILE (32-frame) boundary
RAGGED = dict(a=[256 * 12, 256 * 14 + 100, 256 * 20], t=[20, 11, 30], g=[18, 17, 24])
TOL = 1e-3            # max-abs state error in units of the reference's range: the project's bound for N7 / N8 / N20 / N21 at these run lengths
DEPTH = 4


def _rt():
    from vietvoice_tts_amd import runtime as rt
    return rt


@pytest.fixture(scope="module")
def model4():
    from vietvoice_tts_amd.model_spec import ModelSpec, make_synthetic_weights
    spec = dataclasses.replace(ModelSpec.tiny(), depth=DEPTH)
    return spec, make_synthetic_weights(spec, seed=9527)


@pytest.fixture(scope="module")
def own(model4):
    """Engines of this module's own on the four-block model, and an Oracle whose t_grid is ours to set."""
    from oracle.vv_oracle import Oracle
    from vietvoice_tts_amd.runtime import HipSynth
    spec, w = model4
    engs = {"f32": HipSynth(spec, w, acoustic_dtype="fp32", nfe_step=8), "bf16": HipSynth(spec, w, acoustic_dtype="bf16", nfe_step=8)}
    yield engs, Oracle(spec, w, nfe_step=8)
    for e in engs.values():
        e.close()


@pytest.fixture(scope="module")
def ragged(model4):
    batch = make_batch(model4[0], RAGGED["a"], RAGGED["t"], RAGGED["g"], seed=3)
    assert [int(v) for v in batch["seq_len"]] == [31, 32, 45]
    return batch


def _dev(batch):
    d = {k: (v.to(DEV) if torch.is_tensor(v) else v) for k, v in batch.items()}
    d["lens"] = [int(v) for v in batch["seq_len"]]          # on the host: nothing is read back inside a call (or a capture)
    return d


def _pre(eng, d):
    return eng.preprocess(d["audio"], d["audio_len"], d["ids"], d["text_len"], d["seq_len"], d["N"], seq_len_host=d["lens"])


def _host(d):
    return (C.c_int32 * len(d["lens"]))(*d["lens"])


def _modes(v):
    return v if torch.is_tensor(v) else torch.tensor(list(v), dtype=torch.uint8)


def _run(eng, d, pre, span=None, modes=None, cfg=None, step0=0, n=None, ws=None, x=None):
    """One call of the struct entry on a copy of the batch's noise, or on ``x`` in place.  modes None: vv_transformer_steps_ex."""
    x = d["noise"].clone() if x is None else x
    bm = None if modes is None else (span[0], span[1], _modes(modes))
    eng.transformer_steps_ex(x, pre, step0, eng.n_steps - step0 if n is None else n, _host(d), cfg, ws=ws, block_modes=bm)
    return x


def _one(spec, d, batch, b):
    """Item b of a batch as a batch of its own."""
    sl, la, lt = int(batch["seq_len"][b]), int(batch["audio_len"][b]), int(batch["text_len"][b])
    one = dict(audio=d["audio"][b: b + 1, :max(la, spec.n_fft)].contiguous(), audio_len=d["audio_len"][b: b + 1].contiguous(),
               ids=d["ids"][b: b + 1, :lt].contiguous(), text_len=d["text_len"][b: b + 1].contiguous(),
               seq_len=d["seq_len"][b: b + 1].contiguous(), N=sl, noise=d["noise"][b: b + 1, :sl].contiguous(), lens=[sl])
    return one, sl


def _moved(d, perm, extra):
    """The same items in the order ``perm`` with ``extra`` more padded frames."""
    idx = torch.tensor(perm, device=DEV)
    out = {k: d[k].index_select(0, idx).contiguous() for k in ("audio", "audio_len", "ids", "text_len", "seq_len")}
    out["N"] = d["N"] + extra
    out["noise"] = torch.nn.functional.pad(d["noise"].index_select(0, idx), (0, 0, 0, extra)).contiguous()
    out["lens"] = [d["lens"][p] for p in perm]
    return out


def _err(x, ref):
    return float((x - ref).abs().max()) / float(ref.abs().max())


# ------------------------------------------------------------------------------------------------ 1. the span kernel
def _span(eng, mode, x, d1, d2, buf, R, D, bf16=False):
    rt = _rt()
    p = lambda t: None if t is None else (t if isinstance(t, int) else t.data_ptr())
    a = rt.vv_block_span_args(mode, 1 if bf16 else 0, p(x), p(d1), p(d2), p(buf), R, D)
    return eng.lib.vv_block_span(eng.ctx, C.byref(a), torch.cuda.current_stream().cuda_stream)


@pytest.mark.parametrize("pending", U.SPAN_PENDING)
@pytest.mark.parametrize("mode", [U.MARK, U.DIFF, U.APPLY], ids=["mark", "diff", "apply"])
def test_block_span_against_torch(hip_tiny, mode, pending):
    """D 128 and 1024, 1 / 3 / 86 rows, guard rows around every buffer: the torch expression of the same single fp32 operations,
    torch.equal; what the launch does not own is untouched."""
    eng = hip_tiny["f32"]
    G = U.GUARD
    for D in U.SPAN_DIMS:
        for R in U.SPAN_ROWS:
            x, d1, d2, buf = (torch.from_numpy(a).to(DEV) for a in U.span_operands(R, D))
            if pending == "bf16":
                d1, d2 = d1.to(torch.bfloat16), d2.to(torch.bfloat16)
            if pending == "none":
                d1 = d2 = None
            x0, buf0 = x.clone(), buf.clone()
            d10, d20 = (None, None) if d1 is None else (d1.clone(), d2.clone())
            inner = lambda t: None if t is None else t[G: G + R]
            rc = _span(eng, mode, inner(x), inner(d1), inner(d2), inner(buf), R, D, bf16=pending == "bf16")
            assert rc == 0, eng.lib.vv_last_error(eng.ctx).decode()
            torch.cuda.synchronize()
            X = x0[G: G + R]
            if d1 is not None:
                X = (X + d10[G: G + R].float()) + d20[G: G + R].float()
            want_x, want_buf = x0.clone(), buf0.clone()
            if mode == U.MARK:
                want_buf[G: G + R] = X
            elif mode == U.DIFF:
                want_buf[G: G + R] = X - buf0[G: G + R]
            else:
                want_x[G: G + R] = X + buf0[G: G + R]
            assert torch.equal(x, want_x) and torch.equal(buf, want_buf), (mode, pending, D, R)
            assert d1 is None or (torch.equal(d1, d10) and torch.equal(d2, d20))
            if pending != "bf16":                      # the numpy statement the host check uses: the same bits
                nx, n1, n2, nb = U.span_operands(R, D)
                ex, eb = U.span_expected(mode, nx[G: G + R], None if d1 is None else n1[G: G + R], None if d1 is None else n2[G: G + R], nb[G: G + R])
                assert np.array_equal(x[G: G + R].cpu().numpy(), ex) and np.array_equal(buf[G: G + R].cpu().numpy(), eb)


def test_block_span_one_delta_and_refusals(hip_tiny):
    eng = hip_tiny["f32"]
    R, D = 3, 128
    x, d1, _, buf = (torch.from_numpy(a[:R]).to(DEV) for a in U.span_operands(R, D))
    x0 = x.clone()
    assert _span(eng, U.MARK, x, d1, None, buf, R, D) == 0             # one delta pending: X = x + d1
    torch.cuda.synchronize()
    assert torch.equal(buf, x0 + d1) and torch.equal(x, x0)
    flat = torch.zeros(R * D + 4, device=DEV)
    for bad in (dict(x=None), dict(buf=None), dict(x=flat[1:].data_ptr()), dict(buf=flat[1:].data_ptr()), dict(d1=flat[1:].data_ptr()),
                dict(d1=None, d2=d1), dict(mode=3), dict(R=0), dict(D=126), dict(buf=x)):
        kw = dict(mode=U.DIFF, x=x, d1=d1, d2=None, buf=buf, R=R, D=D)
        kw.update(bad)
        assert _span(eng, kw["mode"], kw["x"], kw["d1"], kw["d2"], kw["buf"], kw["R"], kw["D"]) == -22, bad
    h = flat[:R * D].view(R, D).to(torch.bfloat16)
    assert _span(eng, U.MARK, x, h.view(-1)[2:].data_ptr(), None, buf, R - 1, D, bf16=True) == -22      # a bf16 delta is 8-byte aligned
    torch.cuda.synchronize()
    assert torch.equal(buf, x0 + d1) and torch.equal(x, x0)                                              # nothing ran
    assert _span(eng, U.APPLY, x, None, None, buf, R, D) == 0
    torch.cuda.synchronize()
    assert torch.equal(x, x0 + (x0 + d1))


# ------------------------------------------------------------------------------------------------ 2. off and store-only are today's call
@pytest.mark.parametrize("dt", ["f32", "bf16"])
@pytest.mark.parametrize("name,nfe", [("euler", 8), ("rk4", 3), ("ab2", 8)])
def test_off_and_store_only_equal_ex(own, ragged, dt, name, nfe):
    from vietvoice_tts_amd.model_spec import block_cache_schedule
    rt = _rt()
    eng = own[0][dt]
    d = _dev(ragged)
    try:
        eng.set_nfe(nfe, name)
        pre = _pre(eng, d)
        E = eng.n_evals
        stores = block_cache_schedule(eng.plan, 1, None, report=True)
        assert stores.tolist() == [1] * E and block_cache_schedule(eng.plan, 1).tolist() == [0] * E
        for lanes in (1, 2):
            eng.set_option("lanes", lanes)
            plain = eng._steps_ws_bytes(eng.lib.vv_transformer_ws_bytes, 3, d["N"], _host(d))
            x0 = _run(eng, d, pre)
            x1 = _run(eng, d, pre, (1, 3), [0] * E)
            x2 = _run(eng, d, pre, (1, 3), [0] * E, ws=torch.empty((plain,), dtype=torch.uint8, device=DEV))     # ... in a block of the PLAIN size
            torch.cuda.synchronize()
            assert torch.equal(x1, x0) and torch.equal(x2, x0), (dt, name, lanes, "off")
            for span in ((1, 3), (0, DEPTH), (DEPTH - 1, DEPTH)):
                x3 = _run(eng, d, pre, span, stores)
                torch.cuda.synchronize()
                assert torch.equal(x3, x0), (dt, name, lanes, span, "store only")
        assert rt.SPAN_APPLY == 2
    finally:
        eng.set_option("lanes", 0)
        eng.set_nfe(8, "euler")


# ------------------------------------------------------------------------------------------------ 3. against a reference solver
CASES = {
    # name: (method, nfe, span, every, interval, strengths)
    "(1,3) every 2": ("euler", 8, (1, 3), 2, None, None),
    "(1,3) every 3": ("euler", 8, (1, 3), 3, None, None),
    "(0,4) every 2": ("euler", 8, (0, 4), 2, None, None),
    "(0,4) every 3": ("ab2", 8, (0, 4), 3, None, None),
    "(1,4) every 2": ("rk4", 3, (1, 4), 2, None, None),
    "(1,4) every 3": ("euler", 8, (1, 4), 3, None, None),
    "(0,1) every 2": ("euler", 8, (0, 1), 2, None, None),
    "(0,1) every 3": ("euler", 8, (0, 1), 3, None, None),
    "(1,3) every 2 in an interval": ("euler", 8, (1, 3), 2, (0.05, 0.7), None),
    "(0,4) every 2, strengths with a 0": ("euler", 8, (0, 4), 2, None, (2.0, 0.0, 3.0)),
}
APART_MIN = 1e-2      # measured on the CPU (profiles/block_cache/notes.md): the cached and uncached references are 2e-2 ... 8e-2 of the range apart
_UNCACHED = {}


@pytest.mark.parametrize("case", list(CASES))
def test_fp32_matches_reference_solver(own, model4, ragged, case):
    """The device against the test's own solver per item, within TOL of the state's range; and, on the reference side alone, the solver
    with the span rule against the solver without it: more than APART_MIN of the range, ten times the bound, for every case and item,
    so the bound would notice a device that ignored the schedule."""
    from vietvoice_tts_amd.model_spec import block_cache_schedule, ode_plan
    spec = model4[0]
    engs, orc = own
    eng = engs["f32"]
    method, nfe, span, every, interval, gs = CASES[case]
    gs = [float(spec.cfg_strength)] * 3 if gs is None else list(gs)
    plan = ode_plan(nfe, spec.sway_coef, method)
    modes = block_cache_schedule(plan, every, interval)
    want = U.schedule([float(v) for v in plan.t], every, interval)
    assert modes.tolist() == want and 2 in want
    d = _dev(ragged)
    try:
        eng.set_nfe(nfe, method)
        cfg = torch.tensor(gs, dtype=torch.float32, device=DEV)
        x = _run(eng, d, _pre(eng, d), span, modes, cfg=cfg).cpu()
        torch.cuda.synchronize()
    finally:
        eng.set_nfe(8, "euler")
    for b in range(3):
        la, lt, sl = int(ragged["audio_len"][b]), int(ragged["text_len"][b]), int(ragged["seq_len"][b])
        pre = orc.preprocess(ragged["audio"][b, :la], ragged["ids"][b, :lt], sl, ragged["noise"][b, :sl])
        ref = U.ref_solve_cached(orc, pre, pre["noise"], method, nfe, gs[b], span, want)
        key = (method, nfe, gs[b], b)
        if key not in _UNCACHED:
            _UNCACHED[key] = U.ref_solve_cached(orc, pre, pre["noise"], method, nfe, gs[b], span, [0] * len(want))
        err, apart = _err(x[b, :sl], ref), _err(_UNCACHED[key], ref)
        print(f"{case} item {b} modes {want}: err {err:.3e} of range; reference cached vs uncached {apart:.3e}")
        assert err < TOL, (case, b, err)
        assert apart > APART_MIN, (case, b, apart)


# ------------------------------------------------------------------------------------------------ 4. structure, bit for bit
@pytest.mark.parametrize("dt,name,nfe", [("f32", "rk4", 3), ("bf16", "euler", 9), ("f32", "ab2", 9)])
def test_structure_is_bit_identical(own, model4, ragged, dt, name, nfe):
    from vietvoice_tts_amd.model_spec import block_cache_schedule
    spec = model4[0]
    eng = own[0][dt]
    d = _dev(ragged)
    eng.set_nfe(nfe, name)
    assert eng.n_evals == 8
    span = (1, 3)
    modes = block_cache_schedule(eng.plan, 3)
    assert modes.tolist() == [1, 2, 2, 1, 2, 2, 1, 2]
    cfg = torch.tensor([2.0, 0.75, 3.25], dtype=torch.float32, device=DEV)
    pre = _pre(eng, d)
    try:
        eng.set_option("lanes", 1)
        x1 = _run(eng, d, pre, span, modes, cfg=cfg)
        assert not torch.equal(x1, _run(eng, d, pre, cfg=cfg))
        # the same call twice with another call's planes left in the workspace in between: a call reads nothing an earlier one left
        _run(eng, d, pre, (0, 4), block_cache_schedule(eng.plan, 2), cfg=cfg.flip(0).contiguous())
        assert torch.equal(_run(eng, d, pre, span, modes, cfg=cfg), x1), "again"
        eng.set_option("lanes", 2)
        x2 = _run(eng, d, pre, span, modes, cfg=cfg)
        torch.cuda.synchronize()
        assert torch.equal(x1, x2), "lanes"
        # each item alone: one lane, and its two branches as the lanes
        for b in range(3):
            one, sl = _one(spec, d, ragged, b)
            for lanes in (1, 2):
                eng.set_option("lanes", lanes)
                xa = _run(eng, one, _pre(eng, one), span, modes, cfg=cfg[b: b + 1].contiguous())
                torch.cuda.synchronize()
                assert torch.equal(xa[0], x1[b, :sl]), ("alone", b, lanes)
        # at another index of the batch and another N
        perm = [2, 0, 1]
        mv = _moved(d, perm, 7)
        for lanes in (1, 2):
            eng.set_option("lanes", lanes)
            xm = _run(eng, mv, _pre(eng, mv), span, modes, cfg=cfg[perm].contiguous())
            torch.cuda.synchronize()
            for i, b in enumerate(perm):
                assert torch.equal(xm[i, :d["lens"][b]], x1[b, :d["lens"][b]]), ("moved", b, lanes)
        eng.set_option("lanes", 0)
        # a caller-owned workspace of the size the library names: the same for every schedule, the plain figure plus one plane per lane
        host = _host(d)
        need, plain = eng.cached_ws_bytes(3, d["N"], d["lens"]), eng._steps_ws_bytes(eng.lib.vv_transformer_ws_bytes, 3, d["N"], host)
        plane = (2 * sum(d["lens"]) * spec.dim * 4 + 255) // 256 * 256
        assert need == plain + plane                                            # one lane here (216 packed rows: under the threshold of two)
        ws = torch.empty((need,), dtype=torch.uint8, device=DEV)
        xw = _run(eng, d, pre, span, modes, cfg=cfg, ws=ws)
        torch.cuda.synchronize()
        assert torch.equal(xw, x1), "ws"
        with pytest.raises(RuntimeError, match="too small"):
            _run(eng, d, pre, span, modes, cfg=cfg, ws=ws[:plain])
        # captured into a hipGraph: the schedule travels as launches, no synchronisation, nothing that moves
        xg = d["noise"].clone()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            _run(eng, d, pre, span, modes, cfg=cfg, ws=ws, x=xg)
        xg.copy_(d["noise"])
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(xg, x1), "graph"
        del graph
    finally:
        eng.set_option("lanes", 0)
        eng.set_nfe(8, "euler")


# ------------------------------------------------------------------------------------------------ 5. what the profiler counts
def _prof(eng, fn):
    eng.prof_enable(True)
    eng.prof_collect()
    fn()
    out = eng.prof_collect()
    eng.prof_enable(False)
    return out


@pytest.mark.parametrize("lanes", [1, 2])
def test_profiler_counts_follow_the_schedule(own, model4, ragged, lanes):
    """Per lane and evaluation: one attention launch and two LayerNorms per block run, one LayerNorm in the tail; the GEMM flops of the
    head, the blocks run and the tail on the lanes' rows.  A skipped block counts nothing."""
    from vietvoice_tts_amd.model_spec import block_cache_schedule
    spec = model4[0]
    eng = own[0]["bf16"]
    d = _dev(ragged)
    eng.set_nfe(9, "euler")
    E, R = eng.n_evals, 2 * sum(d["lens"])
    D, FF, M, CD = spec.dim, spec.dim * spec.ff_mult, spec.n_mel, spec.n_mel + spec.text_dim
    pre = _pre(eng, d)
    try:
        eng.set_option("lanes", lanes)
        for span, every in (((1, 3), 2), ((0, 4), 3), ((3, 4), 2)):
            modes = block_cache_schedule(eng.plan, every).tolist()
            run = U.blocks_run(modes, span, DEPTH)
            got = _prof(eng, lambda: _run(eng, d, pre, span, modes))
            n_blocks = sum(run)
            assert got["attention"]["launches"] == lanes * n_blocks, (span, every, lanes)
            assert got["norm"]["launches"] == lanes * (2 * n_blocks + E), (span, every, lanes)
            block = 2.0 * R * (3 * D * D + D * D + 2 * FF * D)
            want = E * (2.0 * R * D * (M + CD) + 2.0 * R * D * M) + n_blocks * block
            print(f"span {span} every {every} lanes {lanes}: blocks run {run}, GEMM flops {got['gemm']['flops']:.6e}, from the schedule {want:.6e}")
            assert abs(got["gemm"]["flops"] - want) <= 1e-9 * want
            n_store, n_light = modes.count(1), modes.count(2)
            off = _prof(eng, lambda: _run(eng, d, pre))["elementwise"]["launches"]
            assert got["elementwise"]["launches"] == off + lanes * (2 * n_store + n_light)      # MARK and DIFF, or APPLY, per lane
    finally:
        eng.prof_enable(False)
        eng.set_option("lanes", 0)
        eng.set_nfe(8, "euler")


# ------------------------------------------------------------------------------------------------ 6. the report
def _drift(eng, d_new, d_prev, lens, D, both=False, n_tiles=None):
    """vv_block_drift_reduce on host planes, the sequences back to back; both: the planes hold the sequences twice (the second copy is the
    unconditional branch).  -> (rc, report [items][2][2])."""
    rt = _rt()
    B = len(lens)
    n_seq = 2 * B if both else B
    R = max(sum(lens), 1) * (2 if both else 1)
    starts = np.concatenate([[0], np.cumsum(lens)])[:B]
    rs = list(starts) + ([int(s) + R // 2 for s in starts] if both else [])
    dn = torch.zeros(R, D)
    dp = torch.zeros(R, D)
    n = sum(lens)
    dn[:n], dp[:n] = torch.from_numpy(d_new), torch.from_numpy(d_prev if d_prev is not None else d_new)
    if both:
        dn[R // 2: R // 2 + n], dp[R // 2: R // 2 + n] = dn[:n].flip(0), dp[:n].flip(0)
    n_tiles = -(-max(lens) // U.TILE) if n_tiles is None else n_tiles
    dnd, dpd = dn.to(DEV), dp.to(DEV)
    row_start = torch.tensor(rs, dtype=torch.int32, device=DEV)
    ln = torch.tensor(list(lens) * (2 if both else 1), dtype=torch.int32, device=DEV)
    partials = torch.full((n_seq, max(n_tiles, 1), 2), float("nan"), dtype=torch.float64, device=DEV)
    report = torch.full((B, 2, 2), float("nan"), dtype=torch.float64, device=DEV)
    a = rt.vv_block_drift_args(dnd.data_ptr(), None if d_prev is None else dpd.data_ptr(), R, D, n_seq, B, 0, n_tiles, row_start.data_ptr(),
                               ln.data_ptr(), partials.data_ptr(), report.data_ptr())
    rc = eng.lib.vv_block_drift_reduce(eng.ctx, C.byref(a), torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return rc, report.cpu().numpy(), dn.numpy(), dp.numpy(), rs


@pytest.mark.parametrize("D", [128, 1024])
def test_drift_reduce_equals_the_mirror_bit_for_bit(hip_tiny, D):
    """Item lengths 0, 31, 32, 33 and 45 in one launch, one tile of partials more than the longest needs."""
    eng = hip_tiny["f32"]
    d_new, d_prev = U.edge_planes(D)
    lens = list(U.EDGE_LENS)
    off = np.concatenate([[0], np.cumsum(lens)])
    rc, got, _, _, _ = _drift(eng, d_new, d_prev, lens, D, n_tiles=U.EDGE_TILES)
    assert rc == 0, eng.lib.vv_last_error(eng.ctx).decode()
    for b in range(len(lens)):
        rows = slice(off[b], off[b + 1])
        want = U.report_mirror(d_new[rows], d_prev[rows])
        assert tuple(got[b, 0]) == want, (b, got[b, 0], want)
        assert np.isnan(got[b, 1]).all()                                      # one branch asked for: the other's place is not written
        if D == 128:
            assert np.allclose(want, U.report_plain(d_new[rows], d_prev[rows]), rtol=1e-12, atol=0.0)
    assert got[0, 0].tolist() == [0.0, 0.0]
    # the first store of a call: nothing to compare with
    rc, first, _, _, _ = _drift(eng, d_new, None, lens, D)
    assert rc == 0
    for b in range(len(lens)):
        rows = slice(off[b], off[b + 1])
        assert tuple(first[b, 0]) == U.report_mirror(d_new[rows], None) and first[b, 0, 0] == 0.0
    # both branches in one launch, as a lane runs them
    rc, both, dn, dp, rs = _drift(eng, d_new, d_prev, lens, D, both=True)
    assert rc == 0
    for b in range(len(lens)):
        for c in range(2):
            r0 = rs[c * len(lens) + b]
            assert tuple(both[b, c]) == U.report_mirror(dn[r0: r0 + lens[b]], dp[r0: r0 + lens[b]]), (b, c)
    assert _drift(eng, d_new[:, :126].copy(), d_prev[:, :126].copy(), lens, 126)[0] == -22
    assert _drift(eng, d_new, d_prev, lens, D, n_tiles=0)[0] == -22


def test_pipeline_report_equals_the_mirror(own, model4, ragged):
    """A store-only run (every = 1 under a report: every evaluation stores) stopped behind evaluation e leaves the contribution of e in a
    caller-owned workspace: the planes lie behind everything the plain call takes, the stores alternate between the two.  The report of
    the whole run equals the mirror fed those planes.  With light evaluations: E2 = 0 at the first store, {0, 0} at a light evaluation;
    the report changes nothing in the state; off, nothing is allocated or launched for it."""
    spec = model4[0]
    eng = own[0]["f32"]
    d = _dev(ragged)
    lens, N, D = d["lens"], d["N"], spec.dim
    Rc = sum(lens)
    eng.set_nfe(5, "euler")
    span = (1, 3)
    assert eng.last_block_cache_report() is None
    try:
        eng.set_option("lanes", 1)
        pre = _pre(eng, d)
        x_plain = _run(eng, d, pre)
        eng.set_block_cache_report(True)
        bm = eng.block_cache_modes((1, 3, 1))
        assert bm[2].tolist() == [1, 1, 1, 1]
        x = d["noise"].clone()
        eng.transformer_steps(x, pre, 0, eng.n_steps, seq_len_host=lens, block_cache=(1, 3, 1))
        rep = eng.last_block_cache_report()
        assert torch.equal(x, x_plain)
        assert rep.shape == (4, 3, 2, 2) and rep.dtype == np.float64
        assert not rep[0, :, :, 0].any() and (rep[:, :, :, 1] > 0).all() and (rep[1:, :, :, 0] > 0).all()
        need_on, need_off = eng.cached_ws_bytes(3, N, lens, report=True), eng.cached_ws_bytes(3, N, lens)
        plain = eng._steps_ws_bytes(eng.lib.vv_transformer_ws_bytes, 3, N, _host(d))
        plane = 2 * Rc * D * 4
        assert plane % 256 == 0 and need_off == plain + plane
        assert need_on == plain + 2 * plane + (2 * 3 * ((N + U.TILE - 1) // U.TILE) * 2 * 8 + 255) // 256 * 256
        ws = torch.zeros(need_on, dtype=torch.uint8, device=DEV)
        planes = []
        for e in range(4):
            xk = d["noise"].clone()
            _run(eng, d, pre, span, bm[2], n=e + 1, ws=ws, x=xk)
            torch.cuda.synchronize()
            part = eng.last_block_cache_report()
            assert np.array_equal(part[: e + 1], rep[: e + 1]) and not part[e + 1:].any()
            o = plain + (e % 2) * plane
            planes.append(ws[o: o + plane].view(torch.float32).reshape(2 * Rc, D).cpu().numpy().copy())
        starts = [0, lens[0], lens[0] + lens[1]]
        for e in range(4):
            for b in range(3):
                for c in range(2):
                    rows = slice(c * Rc + starts[b], c * Rc + starts[b] + lens[b])
                    want = U.report_mirror(planes[e][rows], planes[e - 1][rows] if e else None)
                    assert tuple(rep[e, b, c]) == want, (e, b, c, rep[e, b, c], want)
        print(f"sqrt(E2 / N2) per item and branch at the last evaluation: {np.sqrt(rep[3, :, :, 0] / rep[3, :, :, 1]).round(4).tolist()}")
        # lanes, and an item alone: its report rows are its own
        eng.set_option("lanes", 2)
        _run(eng, d, pre, span, bm[2])
        assert np.array_equal(eng.last_block_cache_report(), rep)
        for b in range(3):
            one, _ = _one(spec, d, ragged, b)
            for lanes in (1, 2):
                eng.set_option("lanes", lanes)
                _run(eng, one, _pre(eng, one), span, bm[2])
                assert np.array_equal(eng.last_block_cache_report()[:, 0], rep[:, b]), (b, lanes)
        eng.set_option("lanes", 1)
        # light evaluations under a report
        lm = eng.block_cache_modes((1, 3, 2))
        assert lm[2].tolist() == [1, 2, 1, 2]
        xl = _run(eng, d, pre, span, lm[2])
        rl = eng.last_block_cache_report()
        assert not rl[1].any() and not rl[3].any() and not rl[0, :, :, 0].any() and (rl[2] > 0).all()
        assert np.array_equal(rl[0], rep[0])
        eng.set_block_cache_report(False)
        assert eng.last_block_cache_report() is None
        assert eng.block_cache_modes((1, 3, 2))[2].tolist() == [1, 2, 1, 2]
        on_launches = None
        off_launches = _prof(eng, lambda: _run(eng, d, pre, span, lm[2]))["elementwise"]["launches"]
        assert torch.equal(_run(eng, d, pre, span, lm[2]), xl) and eng.last_block_cache_report() is None
        eng.set_block_cache_report(True)
        on_launches = _prof(eng, lambda: _run(eng, d, pre, span, lm[2]))["elementwise"]["launches"]
        assert on_launches == off_launches + 2 * 2 + 2                           # two launches at each store, one at each light evaluation
    finally:
        eng.set_block_cache_report(False)
        eng.set_option("lanes", 0)
        eng.set_nfe(8, "euler")


# ------------------------------------------------------------------------------------------------ 7. refusals
def test_refused_calls_leave_the_context_usable(own, ragged):
    from vietvoice_tts_amd.model_spec import block_cache_schedule
    rt = _rt()
    eng = own[0]["bf16"]
    d = _dev(ragged)
    eng.set_nfe(8, "euler")
    E = eng.n_evals
    pre = _pre(eng, d)
    modes = block_cache_schedule(eng.plan, 2).tolist()
    x0 = _run(eng, d, pre, (1, 3), modes)
    x_plain = _run(eng, d, pre)
    x = d["noise"].clone()

    def refused(m, span=(1, 3), e0=0, e1=None, why=None):
        """The library's -22; the host restatement names the same reason."""
        assert U.check_modes(m, span, DEPTH, E, e0, e1) == why
        return pytest.raises(RuntimeError, match=r"\(-22\)")
    assert U.check_modes(modes, (1, 3), DEPTH, E) is None
    three = list(modes)
    three[4] = 3
    with refused(three, why="value"):
        _run(eng, d, pre, (1, 3), three, x=x)
    early = [2] + modes[1:]
    with refused(early, why="2 before 1"):
        _run(eng, d, pre, (1, 3), early, x=x)
    after_full = [0, 2] + modes[2:]                                            # a full evaluation that does not store is no store
    with refused(after_full, why="2 before 1"):
        _run(eng, d, pre, (1, 3), after_full, x=x)
    with refused(modes, e0=2, e1=7, why="step0"):
        _run(eng, d, pre, (1, 3), modes, x=x, step0=2)
    for span in ((-1, 2), (2, 2), (3, 1), (0, DEPTH + 1)):
        with refused(modes, span=span, why="span"):
            _run(eng, d, pre, span, modes, x=x)
    for m in (modes[:-1], modes + [0]):
        with refused(m, why="n_modes"):
            _run(eng, d, pre, (1, 3), m, x=x)
    # a report of another shape
    a = rt.vv_steps_args()
    a.B, a.N, a.seq_len, a.x, a.seq_len_host = 3, d["N"], pre["seq_len"].data_ptr(), x.data_ptr(), C.cast(_host(d), C.c_void_p)
    a.cat_mel_text, a.cat_mel_text_drop, a.rope_cos_q, a.rope_sin_q, a.rope_cos_k, a.rope_sin_k = rt._pre_ptrs(pre)
    a.step0, a.n_steps = 0, eng.n_steps
    buf = torch.zeros((E, 3, 2, 2), dtype=torch.float64, device=DEV)
    mh = torch.tensor(modes, dtype=torch.uint8)
    st = torch.cuda.current_stream().cuda_stream
    for rb, re_ in ((2, E), (3, E + 1)):
        k = rt.vv_block_cache_args(1, 3, mh.data_ptr(), E, buf.data_ptr(), rb, re_)
        assert eng.lib.vv_transformer_steps_cached(eng.ctx, C.byref(a), C.byref(k), st) == -22
    try:
        eng.set_option("split_k_tail", 1)
        with pytest.raises(RuntimeError, match="split_k_tail"):
            _run(eng, d, pre, (1, 3), modes, x=x)
    finally:
        eng.set_option("split_k_tail", 0)
    need = eng.cached_ws_bytes(3, d["N"], d["lens"])
    ws = torch.empty((need,), dtype=torch.uint8, device=DEV)
    with pytest.raises(RuntimeError, match="too small"):
        _run(eng, d, pre, (1, 3), modes, x=x, ws=ws[: need - 256])
    with pytest.raises(RuntimeError, match=r"\(-22\)"):                        # whatever _ex refuses: a block without the host lengths
        eng.transformer_steps_ex(x, pre, 0, eng.n_steps, None, None, ws=ws, block_modes=(1, 3, mh))
    with pytest.raises(ValueError, match="mask"):                              # no mask and no APG on this entry
        eng.transformer_steps(x, pre, 0, eng.n_steps, guide=torch.ones((E, 3), dtype=torch.uint8), block_cache=(1, 3, 2))
    with pytest.raises(ValueError, match="depth"):
        eng.transformer_steps(x, pre, 0, eng.n_steps, block_cache=(1, DEPTH + 1, 2))
    torch.cuda.synchronize()
    assert torch.equal(x, d["noise"]) and not buf.any()                        # nothing ran
    x1, x2 = _run(eng, d, pre, (1, 3), modes, ws=ws), _run(eng, d, pre)
    torch.cuda.synchronize()
    assert torch.equal(x1, x0) and torch.equal(x2, x_plain)                    # the next cached call and the next plain call: as before
    # a schedule without a light evaluation may start anywhere
    xs, xr = d["noise"].clone(), d["noise"].clone()
    _run(eng, d, pre, x=xs, step0=2, n=3)
    _run(eng, d, pre, (1, 3), [1] * E, x=xr, step0=2, n=3)
    torch.cuda.synchronize()
    assert torch.equal(xs, xr)


# ------------------------------------------------------------------------------------------------ 8. engine level
def _engine(tmp, **kw):
    from vietvoice_tts_amd.core import ModelConfig, TTSEngine
    cfg = ModelConfig(model_cache_dir=str(tmp), synthetic_model=True, model_spec="tiny", nfe_step=8, acoustic_dtype="fp32",
                      max_chunk_duration=8.0, **kw)
    return TTSEngine(cfg)


def _lsb(a, b):
    return int(np.abs(a.astype(np.int32) - b.astype(np.int32)).max())


SPANS = [(1, 2, 2), (0, 2, 2)]


@pytest.fixture(scope="module")
def waves(tmp_path_factory):
    """The device path's audio per span and without the option (shared by the engine tests), and the reports of the first span."""
    tmp = tmp_path_factory.mktemp("block_cache")
    out = {}
    for bc in SPANS:
        e = _engine(tmp, block_cache=bc, block_cache_report=bc == SPANS[0])
        out[bc] = e.synthesize(LONG)[0]
        if bc == SPANS[0]:
            out["chunks"], out["reports"] = len(e._last_plan), e.last_block_cache_report
        e.cleanup()
    e0 = _engine(tmp)
    out[None] = e0.synthesize(LONG)[0]
    e0.cleanup()
    return tmp, out


def test_engine_device_path_report_and_off(waves, monkeypatch):
    """The <= 2 LSB figures are the N2 / N7 / N8 tolerances of the same comparisons without the option."""
    tmp, out = waves
    base = out[None]
    assert out["chunks"] > 1
    for bc in SPANS:
        assert out[bc].shape == base.shape and _lsb(base, out[bc]) > 2, bc     # another trajectory
    reports = out["reports"]
    assert len(reports) >= 1 and sum(r.shape[1] for r in reports) == out["chunks"]
    for rep in reports:
        assert rep.shape[0] == 7 and rep.shape[2:] == (2, 2) and rep.dtype == np.float64
        assert not rep[1::2].any() and not rep[0, :, :, 0].any()               # zeros at the light evaluations and for the first store's drift
        assert (rep[0::2, :, :, 1] > 0).all() and (rep[2::2, :, :, 0] > 0).all()
    e2 = _engine(tmp, block_cache=SPANS[0])                                    # the report changes nothing
    w2, _ = e2.synthesize(LONG)
    assert e2.last_block_cache_report == []
    e2.cleanup()
    assert np.array_equal(w2, out[SPANS[0]])
    # every = 1 is off, and the unset option never calls the new entry
    from vietvoice_tts_amd.runtime import HipSynth
    calls = []
    real = HipSynth.transformer_steps_ex

    def spy(self, *a, **kw):
        calls.append(kw.get("block_modes"))
        return real(self, *a, **kw)
    monkeypatch.setattr(HipSynth, "transformer_steps_ex", spy)
    e3 = _engine(tmp, block_cache=(1, 2, 1))
    w3, _ = e3.synthesize(LONG)
    lib3, n3 = e3.model_session_manager.engine.lib, len(calls)
    e3.cleanup()
    assert np.array_equal(w3, base) and all(c is None or not (c[2] == 2).any() for c in calls)
    e4 = _engine(tmp)
    eng4 = e4.model_session_manager.engine

    class Lib:                                                                 # the library with the new entry taken out
        def __getattr__(self, name):
            if name == "vv_transformer_steps_cached":
                raise AssertionError("the unset option called vv_transformer_steps_cached")
            return getattr(lib3, name)
    eng4.lib = Lib()
    w4, _ = e4.synthesize(LONG)
    eng4.lib = lib3
    e4.cleanup()
    assert np.array_equal(w4, base) and all(c is None for c in calls[n3:])
    with pytest.raises(ValueError, match="depth"):
        _engine(tmp, block_cache=(1, 3, 2))                                    # the tiny model has two blocks


@pytest.mark.parametrize("bc", SPANS)
@pytest.mark.parametrize("fuse", [1, 2])
def test_engine_session_path(waves, bc, fuse):
    tmp, out = waves
    e = _engine(tmp, block_cache=bc, fuse_nfe=fuse)
    ref, txt = e.model_session_manager.select_sample()
    ws = e._synthesize_sessions(e._prepare_inputs(ref, txt, LONG))
    got = e.audio_processor.concatenate_with_crossfade_improved(ws, e.config.cross_fade_duration, e.config.sample_rate)
    e.cleanup()
    assert got.shape == out[bc].shape and _lsb(got, out[bc]) <= 2, (bc, fuse)


@pytest.mark.parametrize("bc", SPANS)
def test_engine_stream_path(waves, bc):
    tmp, out = waves
    e = _engine(tmp, block_cache=bc)
    got = np.concatenate(list(e.synthesize_stream(LONG, chunks_per_step=1)))
    e.cleanup()
    assert got.shape == out[bc].shape and _lsb(got, out[bc]) <= 2


def test_batching_frontend_applies_it_to_every_batch(tmp_path):
    from vietvoice_tts_amd.batching import BatchingFrontend
    e = _engine(tmp_path, block_cache=SPANS[0])
    e0 = _engine(tmp_path)
    fe, fe0 = BatchingFrontend(e, max_wait_ms=300.0, max_requests=8), BatchingFrontend(e0, max_wait_ms=300.0, max_requests=8)
    text = "Xin chào các bạn, hôm nay thế nào?"
    try:
        alone = fe.submit(text, speed=1.0, serial=7).result(timeout=300)[0]
        default = fe0.submit(text, speed=1.0, serial=7).result(timeout=300)[0]
        n0 = fe.batches_run
        futs = [fe.submit("Tạm biệt và hẹn gặp lại.", speed=1.3, serial=8, gender="male", cfg_strength=3.0),
                fe.submit(text, speed=1.0, serial=7),
                fe.submit(LONG, speed=0.8, serial=9, cfg_strength=0.0)]        # a strength of 0 travels as a strength: no mask is built
        outs = [f.result(timeout=300)[0] for f in futs]
        assert fe.batches_run == n0 + 1
        assert outs[1].shape == alone.shape and _lsb(outs[1], alone) <= 2
        assert default.shape == alone.shape and _lsb(default, alone) > 2
        with pytest.raises(ValueError, match="block_cache"):
            fe.submit(text, cfg_reuse=2).result(timeout=5)
        with pytest.raises(ValueError, match="block_cache"):
            fe.submit(text, cfg_interval=(0.1, 0.9)).result(timeout=5)
        assert fe.submit(text, speed=1.0, serial=7, cfg_reuse=1).result(timeout=300)[0].shape == alone.shape      # 1 is off
    finally:
        fe.close()
        fe0.close()
        e.cleanup()
        e0.cleanup()


def test_engine_edit_speech_restores_the_kept_frames(tmp_path):
    from vietvoice_tts_amd.pack import MAX_POS
    from vietvoice_tts_amd.speech_edit import plan_edit
    e = _engine(tmp_path, block_cache=SPANS[1], block_cache_report=True)
    e0 = _engine(tmp_path)
    sr = e.config.sample_rate
    clip, _ = e0.synthesize("Xin chào các bạn, hôm nay trời đẹp quá.")
    dur = clip.size / sr
    parts, fix, text = [(0.3 * dur, 0.5 * dur)], [0.3 * dur], "Xin chào các anh, hôm nay trời đẹp quá."
    eng = e.model_session_manager.engine
    kept = {}
    real = eng.edit_restore

    def spy(x, pre, keep):                                                     # the state behind the restore, and what it was restored from
        real(x, pre, keep)
        kept["x"], kept["cat"], kept["keep"] = x.clone(), pre["cat_mel_text"].clone(), keep.clone()
    eng.edit_restore = spy
    out, _ = e.edit_speech(clip, text, parts, fix_duration=fix, seed=11)
    rep = e.last_block_cache_report
    base, _ = e0.edit_speech(clip, text, parts, fix_duration=fix, seed=11)
    plan = plan_edit(clip.size, parts, fix, sr, e.config.hop_length, e.model_session_manager.spec.n_fft, MAX_POS)
    M = e.model_session_manager.spec.n_mel
    e.cleanup()
    e0.cleanup()
    assert out.dtype == np.int16 and out.size == plan.spliced_len
    assert base.shape == out.shape and _lsb(base, out) > 2
    k = kept["keep"][0, : plan.n_frames].bool()
    assert bool(k.any()) and not bool(k.all())
    assert torch.equal(kept["x"][0, : plan.n_frames][k], kept["cat"][0, : plan.n_frames, :M][k])      # the kept frames exactly
    assert len(rep) == 1 and rep[0].shape == (7, 1, 2, 2) and not rep[0][1::2].any() and (rep[0][0::2, :, :, 1] > 0).all()
