"""-m gpu: the sampler's options in combination (tests/sampler_util.py: the factor table, its covering array, the one reference solver).

Per case of the covering array, on the four-block tiny model at 31 / 32 / 45 frames and B = 1:
  parity (fp32 engine) -- every item against the solver on the float64 oracle, err = max |x - ref64| / max |ref64| within
      4 x yardstick + 2^-23, the yardstick being the same solver on the fp32 oracle under the same metric.  Nothing is fitted to a device
      result; that every option moves the reference by more than 100 bounds is asserted on the CPU (test_sampler_matrix_cpu.py).
  twins (fp32 and bf16 engines) -- the case's own levels (lanes, split, host or device lengths, own or caller-owned workspace, reports,
      ragged / permuted / single batch) give, item by item, the bits of the same plan, strength and form at the plain levels (one lane, one
      call, host lengths, the context's workspace, reports off, the ragged batch); so does each item alone, and the call captured into a
      graph and replayed where it is capturable (host lengths, reports off).  The guard bytes behind a caller-owned workspace stay intact;
      the report rows of an item are the same bits at the case's levels and at the plain ones.
  mirrors -- at the plain levels the drift report and the block-cache report equal the numpy mirrors of the option files bit for bit, on
      every plan of one evaluation per step (a call can stop behind each of its evaluations).
  refusals -- every pair of levels ``supported`` rejects, and the option pairs of OPTION_RULES: -22 / ValueError with the rule's own message,
      nothing launched, the plan in force unchanged, and the next supported call gives the bits of a fresh engine."""
import ctypes as C
import time

import numpy as np
import pytest
import torch

from tests import sampler_util as S

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
CASES = S.cases()
GUARD = 4096          # bytes behind a caller-owned workspace
PLAIN = dict(lanes=1, call="whole", lengths="host", ws="own", reports="off", batch="ragged")
_RUNS = {}            # (engine, case id) -> (x on the host, reports)
_PLAIN = {}           # (engine, plan, strength, form, reports) -> the same of the plain levels


@pytest.fixture(scope="module")
def rig():
    """The four-block model's engines (fp32 and bf16), and the three batches on the device."""
    from vietvoice_tts_amd.runtime import HipSynth
    spec, w, batch, _, _ = S.setup()
    engs = {"f32": HipSynth(spec, w, acoustic_dtype="fp32", nfe_step=8), "bf16": HipSynth(spec, w, acoustic_dtype="bf16", nfe_step=8)}
    d = {k: (v.to(DEV) if torch.is_tensor(v) else v) for k, v in batch.items()}
    d["lens"] = [int(v) for v in batch["seq_len"]]
    data = {"ragged": d, "permuted": _moved(d, list(S.PERM), S.EXTRA)}
    for b in range(3):
        data["alone", b] = _one(spec, d, batch, b)
    data["one"] = data["alone", S.ONE]
    yield spec, engs, data
    for e in engs.values():
        e.close()


def _one(spec, d, batch, b):
    """Item b of the batch as a batch of its own."""
    sl, la, lt = int(batch["seq_len"][b]), int(batch["audio_len"][b]), int(batch["text_len"][b])
    return dict(audio=d["audio"][b: b + 1, :max(la, spec.n_fft)].contiguous(), audio_len=d["audio_len"][b: b + 1].contiguous(),
                ids=d["ids"][b: b + 1, :lt].contiguous(), text_len=d["text_len"][b: b + 1].contiguous(),
                seq_len=d["seq_len"][b: b + 1].contiguous(), N=sl, noise=d["noise"][b: b + 1, :sl].contiguous(), lens=[sl])


def _moved(d, perm, extra):
    """The same items in the order ``perm`` with ``extra`` more padded frames."""
    idx = torch.tensor(perm, device=DEV)
    out = {k: d[k].index_select(0, idx).contiguous() for k in ("audio", "audio_len", "ids", "text_len", "seq_len")}
    out["N"] = d["N"] + extra
    out["noise"] = torch.nn.functional.pad(d["noise"].index_select(0, idx), (0, 0, 0, extra)).contiguous()
    out["lens"] = [d["lens"][p] for p in perm]
    return out


def _ws_bytes(eng, B, N, lens, guide, apg, bm):
    """The size query of the entry transformer_steps_ex routes the call to, with the reports as they are switched."""
    if bm is not None:
        return eng.cached_ws_bytes(B, N, lens, report=eng.block_cache_report)
    has2 = guide is not None and bool((guide[:, :B] == 2).any())
    if guide is not None and apg is None and (eng.cfg_reuse_report or has2):
        return eng.reuse_ws_bytes(B, N, lens, report=eng.cfg_reuse_report)
    if apg is not None:
        return eng.apg_ws_bytes(B, N, lens)
    if guide is not None:
        return eng.guided_ws_bytes(B, N, lens)
    return eng._steps_ws_bytes(eng.lib.vv_transformer_ws_bytes, B, N, (C.c_int32 * B)(*lens))


class _Call:
    """One case on one engine, set up: the plan, the lanes and the reports switched, the arguments built as production builds them
    (HipSynth.guidance_mask, apg_tensors, block_cache_modes).  Use as a context: it puts the engine back."""

    def __init__(self, eng, spec, data, case, items=None, bd=None):
        self.eng, self.case = eng, case
        self.items = S.items_of(case) if items is None else items
        self.d = data[case["batch"]] if bd is None else bd
        self.opts = [S.item_options(case, b, spec) for b in self.items]

    def __enter__(self):
        try:
            return self._enter()
        except BaseException:
            self.__exit__()
            raise

    def _enter(self):
        eng, case, d = self.eng, self.case, self.d
        method, nfe = S.PLANS[case["plan"]]
        o = S.FORMS[case["form"]]
        B = len(self.items)
        eng.set_nfe(nfe, method)
        eng.set_option("lanes", case["lanes"])
        if case["reports"] == "on":
            if eng.plan.beta is not None:
                eng.set_ode_report(True)
            eng.set_cfg_reuse_report(True)
            eng.set_block_cache_report(True)
        host = case["lengths"] == "host"
        self.pre = eng.preprocess(d["audio"], d["audio_len"], d["ids"], d["text_len"], d["seq_len"], d["N"], seq_len_host=d["lens"] if host else None)
        self.host = (C.c_int32 * B)(*d["lens"]) if host else None
        gs = [p["g"] for p in self.opts]
        self.cfg = None if case["strength"] == "model" else torch.tensor(gs, dtype=torch.float32, device=DEV)
        self.guide = self.apg = self.bm = None
        if "cache" in o:
            self.bm = eng.block_cache_modes(o["cache"], o.get("cache_interval"))
        else:
            self.guide = eng.guidance_mask(o.get("interval"), gs, None if "reuse" not in o else [p["k"] for p in self.opts])
            if o.get("apg"):
                self.apg = eng.apg_tensors([p["apg"][0] for p in self.opts], [p["apg"][1] for p in self.opts])
        self.block = self.ws = None
        if case["ws"] == "caller":
            self.take_ws()
        self.calls = S.split_of(case, eng.n_steps)
        return self

    def take_ws(self):
        need = _ws_bytes(self.eng, len(self.items), self.d["N"], self.d["lens"], self.guide, self.apg, self.bm)
        assert need % 256 == 0
        self.block = torch.full((need + GUARD,), 0xA5, dtype=torch.uint8, device=DEV)
        self.ws = self.block[:need]

    def launch(self, x, calls=None):
        for step0, n in (self.calls if calls is None else calls):
            self.eng.transformer_steps_ex(x, self.pre, step0, n, self.host, self.cfg, ws=self.ws, guide=self.guide, apg=self.apg, block_modes=self.bm)

    def run(self):
        x = self.d["noise"].clone()
        self.launch(x)
        torch.cuda.synchronize()
        if self.block is not None:
            assert bool((self.block[self.ws.numel():] == 0xA5).all()), "the guard bytes behind the workspace"
        return x

    def reports(self):
        eng = self.eng
        out = {}
        if self.case["reports"] == "on":
            out = dict(ode=eng.last_ode_report() if eng.plan.beta is not None else None,
                       reuse=eng.last_cfg_reuse_report() if (self.guide is not None and self.apg is None) else None,
                       cache=eng.last_block_cache_report() if self.bm is not None else None)
        return {k: v for k, v in out.items() if v is not None}

    def __exit__(self, *exc):
        eng = self.eng
        eng.set_ode_report(False)
        eng.set_cfg_reuse_report(False)
        eng.set_block_cache_report(False)
        eng.set_option("lanes", 0)
        eng.set_nfe(8, "euler")
        return False


def _case_run(rig, dt, case):
    spec, engs, data = rig
    key = (dt, S.case_id(case))
    if key not in _RUNS:
        with _Call(engs[dt], spec, data, case) as c:
            x = c.run()
            _RUNS[key] = (x.cpu(), c.reports())
    return _RUNS[key]


def _plain_run(rig, dt, case, reports="off"):
    """The plan, strength and form of a case at the plain levels, on the ragged batch; each item alone gives the same bits."""
    spec, engs, data = rig
    key = (dt, case["plan"], case["strength"], case["form"], reports)
    if key not in _PLAIN:
        plain = dict(case, **dict(PLAIN, reports=reports))
        with _Call(engs[dt], spec, data, plain) as c:
            x = c.run().cpu()
            reps = c.reports()
        if reports == "off":
            for b in range(3):
                with _Call(engs[dt], spec, data, plain, items=(b,), bd=data["alone", b]) as c:
                    xa = c.run().cpu()
                assert torch.equal(xa[0], x[b, :data["ragged"]["lens"][b]]), (dt, S.case_id(case), "item alone", b)
        _PLAIN[key] = (x, reps)
    return _PLAIN[key]


# ------------------------------------------------------------------------------------------------ 1. parity
@pytest.mark.parametrize("case", CASES, ids=S.case_id)
def test_parity_with_float64(rig, case):
    spec, _, data = rig
    t0 = time.perf_counter()
    x, _ = _case_run(rig, "f32", case)
    t1 = time.perf_counter()
    lens = data["ragged"]["lens"]
    worst = []
    for i, b in enumerate(S.items_of(case)):
        opt = S.item_options(case, b, spec)
        r64, y, bd = S.parity_refs(case["plan"], b, opt)
        e = S.err(x[i, :lens[b]], r64)
        print(f"SAMPLER_PARITY {S.case_id(case)} item {b} err {e:.3e} yardstick {y:.3e} bound {bd:.3e} err/bound {e / bd:.3f}")
        worst.append((e / bd, b, e, bd))
    print(f"SAMPLER_TIME {S.case_id(case)} device {t1 - t0:.3f} s references {time.perf_counter() - t1:.3f} s")
    for ratio, b, e, bd in worst:
        assert e <= bd, (S.case_id(case), b, e, bd)


# ------------------------------------------------------------------------------------------------ 2. twins
def _same_reports(case, i, b, got, want, calls, s):
    """Item b's rows of every report: the case's levels against the plain ones.  Under a split the last call's report is what is left: its
    rows alone, and of the drift report N2 alone (E2 compares with what the call itself stored: a call reads nothing an earlier one left)."""
    assert set(got) == set(want), (got.keys(), want.keys())
    for name, rep in got.items():
        ref = want[name]
        if len(calls) == 1:
            assert np.array_equal(rep[:, i], ref[:, b]), (S.case_id(case), name, b)
            continue
        step0, n = calls[-1]
        per = 1 if name == "ode" else s
        rows = slice(step0 * per, (step0 + n) * per)
        assert np.array_equal(rep[rows, i][..., 1], ref[rows, b][..., 1]), (S.case_id(case), name, b, "N2 of the last call")
        assert not rep[: step0 * per, i].any(), (S.case_id(case), name, b, "rows outside the last call")


@pytest.mark.parametrize("case", CASES, ids=S.case_id)
@pytest.mark.parametrize("dt", ["f32", "bf16"])
def test_twins_are_bit_identical(rig, dt, case):
    spec, engs, data = rig
    lens = data["ragged"]["lens"]
    x, reps = _case_run(rig, dt, case)
    xp, _ = _plain_run(rig, dt, case)
    assert torch.isfinite(x).all()
    for i, b in enumerate(S.items_of(case)):
        assert torch.equal(x[i, :lens[b]], xp[b, :lens[b]]), (dt, S.case_id(case), "item", b)
    if case["reports"] == "on":
        _, want = _plain_run(rig, dt, case, reports="on")
        plan = S.plan_of(case["plan"])
        for i, b in enumerate(S.items_of(case)):
            _same_reports(case, i, b, reps, want, S.split_of(case, int(plan.dt.numel())), plan.s)
    if case["lengths"] == "host" and case["reports"] == "off":             # capturable: nothing is read back, nothing allocated
        with _Call(engs[dt], spec, data, case) as c:
            if c.ws is None:
                c.take_ws()                                                # a graph points into a block that cannot move
            xg = c.d["noise"].clone()
            c.launch(xg)                                                   # warm-up: sets kernel attributes before the capture
            torch.cuda.synchronize()
            graph = torch.cuda.CUDAGraph()
            with torch.cuda.graph(graph):
                c.launch(xg)
            xg.copy_(c.d["noise"])
            graph.replay()
            torch.cuda.synchronize()
            assert torch.equal(xg.cpu(), x), (dt, S.case_id(case), "captured and replayed")
            assert bool((c.block[c.ws.numel():] == 0xA5).all())
            del graph


@pytest.mark.parametrize("form", ["none", "interval", "apg", "reuse2", "cache13x2"])
@pytest.mark.parametrize("plan", ["ab2", "ab3"])
def test_a_workspace_of_the_named_size_serves_a_call_under_the_step_report(rig, plan, form):
    """Three levels at once, which a pairwise array need not hold: a multistep plan, the reports on, a caller-owned workspace of exactly
    the bytes the size query names.  The step report keeps one more slope and its partial sums; the queries of HipSynth name them (they
    did not: the library learns of the report only while a buffer is set, and the queries ran with none)."""
    spec, engs, data = rig
    eng = engs["f32"]
    case = dict(plan=plan, strength="item", form=form, **dict(PLAIN, ws="caller", reports="on", lanes=2))
    off = dict(case, reports="off")
    with _Call(eng, spec, data, off) as c:
        need_off = c.ws.numel()
    with _Call(eng, spec, data, case) as c:
        need_on = c.ws.numel()
        x = c.run().cpu()
        rep = c.reports()["ode"]
    assert need_on > need_off, (need_on, need_off)
    xp, want = _plain_run(rig, "f32", case, reports="on")
    assert torch.equal(x, xp) and np.array_equal(rep, want["ode"])


ONE_STAGE = [p for p in S.PLANS if S.PLANS[p][0] in ("euler", "ab2", "ab3")]


@pytest.mark.parametrize("form", ["interval", "reuse2", "reuse123iv", "cache13x2", "cache04x3iv"])
@pytest.mark.parametrize("strength", list(S.FACTORS["strength"]))
@pytest.mark.parametrize("plan", ONE_STAGE)
def test_reports_equal_their_mirrors_on_one_stage_plans(rig, plan, strength, form):
    """The drift report (N21) and the block-cache report (N23) of the plain levels -- the ones test_twins_are_bit_identical compares every
    case's report rows with -- against the numpy mirrors of the option files (cfg_reuse_util.drift_mirror, block_cache_util.report_mirror),
    bit for bit.  The mirrors are fed what the device itself computed: a call that stops behind evaluation e leaves the DiT's two
    predictions, or the stored contribution, in a caller-owned workspace.  A call cannot stop inside a Runge-Kutta step, so this covers
    the plans of one evaluation per step; the step report's mirror needs the combined slope and stays in test_multistep_gpu.py."""
    from tests import block_cache_util as BU
    from tests import cfg_reuse_util as RU
    from tests.test_cfg_reuse_gpu import _pred_offset
    spec, engs, data = rig
    eng = engs["f32"]
    case = dict(plan=plan, strength=strength, form=form, **dict(PLAIN, reports="on", ws="caller"))
    _, want = _plain_run(rig, "f32", case, reports="on")
    d = data["ragged"]
    lens, M, D = d["lens"], spec.n_mel, spec.dim
    Rc, MP, starts = sum(lens), (M + 127) // 128 * 128, [0, lens[0], lens[0] + lens[1]]
    checked = 0
    with _Call(eng, spec, data, case) as c:
        def stop_behind(e, last):
            x = d["noise"].clone()
            c.launch(x, [(0, e + 1)])
            torch.cuda.synchronize()
            part = last()
            assert np.array_equal(part[: e + 1], rep[: e + 1]) and not part[e + 1:].any(), e
        if c.bm is not None:
            rep, modes = want["cache"], c.bm[2].tolist()
            front = _ws_bytes(eng, 3, d["N"], lens, None, None, None)             # everything the call takes in front of the two planes
            plane = 2 * Rc * D * 4
            assert plane % 256 == 0 and c.ws.numel() >= front + 2 * plane
            prev, n_store = None, 0
            for e in range(eng.n_evals):
                if modes[e] != S.STORE:
                    assert not rep[e].any(), e
                    continue
                stop_behind(e, eng.last_block_cache_report)
                o = front + (n_store % 2) * plane
                cur = c.ws[o: o + plane].view(torch.float32).reshape(2 * Rc, D).cpu().numpy().copy()
                for b in range(3):
                    for br in range(2):
                        rows = slice(br * Rc + starts[b], br * Rc + starts[b] + lens[b])
                        mirror = BU.report_mirror(cur[rows], None if prev is None else prev[rows])
                        assert tuple(rep[e, b, br]) == mirror, (e, b, br, rep[e, b, br], mirror)
                        checked += 1
                prev, n_store = cur, n_store + 1
        else:
            rep, mask = want["reuse"], c.guide
            o = _pred_offset(spec, 2 * Rc)
            kept = {}
            for e in range(eng.n_evals):
                computed = [b for b in range(3) if int(mask[e, b]) == 1]
                for b in range(3):
                    assert b in computed or not rep[e, b].any(), (e, b)
                if not computed:
                    continue
                stop_behind(e, eng.last_cfg_reuse_report)
                Ru = sum(lens[b] for b in computed)                                # the unconditional rows of the items computed at e, compacted
                pred = c.ws[o: o + (Rc + Ru) * MP * 4].view(torch.float32).reshape(Rc + Ru, MP).cpu().numpy()
                u0 = Rc
                for b in computed:
                    pc, pu = pred[starts[b]: starts[b] + lens[b], :M].copy(), pred[u0: u0 + lens[b], :M].copy()
                    u0 += lens[b]
                    mirror = RU.drift_mirror(pc, pu, kept.get(b))
                    assert tuple(rep[e, b]) == mirror, (e, b, rep[e, b], mirror)
                    kept[b] = (pc - pu).astype(np.float32)
                    checked += 1
    assert checked, "no report row was compared"


# ------------------------------------------------------------------------------------------------ 3. refusals
REFUSED = S.pairs(False)


@pytest.fixture(scope="module")
def fresh(rig):
    """The plain Euler case on an engine nothing else has touched."""
    from vietvoice_tts_amd.runtime import HipSynth
    spec, _, data = rig
    w = S.setup()[1]
    case = dict(plan="euler", strength="model", form="none", **PLAIN)
    out = {}
    for dt, name in (("f32", "fp32"), ("bf16", "bf16")):
        eng = HipSynth(spec, w, acoustic_dtype=name, nfe_step=8)
        with _Call(eng, spec, data, case) as c:
            out[dt] = c.run().cpu()
        eng.close()
    return case, out


def _after_a_refusal(eng, c, x, before):
    """Nothing ran, and the plan is the one in force."""
    torch.cuda.synchronize()
    assert torch.equal(x, before), "the refused call launched something"
    method, nfe = S.PLANS[c.case["plan"]]
    assert (eng.nfe_step, eng.ode_method, eng.n_steps) == (nfe, method, int(S.plan_of(c.case["plan"]).dt.numel()))


@pytest.mark.parametrize("pair", REFUSED, ids=lambda p: f"{p[0][0]}={p[0][1]}+{p[1][0]}={p[1][1]}")
@pytest.mark.parametrize("dt", ["f32", "bf16"])
def test_refused_pairs(rig, fresh, dt, pair):
    spec, engs, data = rig
    eng = engs[dt]
    case = dict(dict(plan="euler", strength="model", form="none", **PLAIN), **dict(pair))
    ok, (where, word) = S.supported(case)
    assert not ok
    with _Call(eng, spec, data, dict(case, ws="own")) as c:               # the workspace is taken by hand: the size query itself needs host lengths
        x = c.d["noise"].clone()
        if case["ws"] == "caller":
            c.block = torch.full((1 << 24,), 0xA5, dtype=torch.uint8, device=DEV)
            c.ws = c.block[: (1 << 24) - GUARD]
        if case["call"] == "split":
            c.launch(x, c.calls[:1])                                       # the first half is a supported call
            torch.cuda.synchronize()
        before = x.clone()
        with pytest.raises(RuntimeError, match=r"\(-22\)") as info:
            c.launch(x, S.split_of(case, eng.n_steps)[-1:])
        assert word in str(info.value), (where, str(info.value))
        _after_a_refusal(eng, c, x, before)
        if c.block is not None:
            assert bool((c.block == 0xA5).all())
    plain, want = fresh
    with _Call(eng, spec, data, plain) as c:
        assert torch.equal(c.run().cpu(), want[dt]), "the next supported call"


@pytest.mark.parametrize("rule", range(len(S.OPTION_RULES)))
def test_refused_option_pairs(rig, fresh, rule):
    """What the routing refuses of the raw options (no pair of levels: a form is one level)."""
    from vietvoice_tts_amd.model_spec import block_cache_schedule
    spec, engs, data = rig
    eng = engs["f32"]
    o, where, word = S.OPTION_RULES[rule]
    plain, want = fresh
    with _Call(eng, spec, data, plain) as c:
        g = [float(spec.cfg_strength)] * 3
        guide = eng.guidance_mask(o.get("interval"), g, o.get("reuse"))
        apg = eng.apg_tensors(list(S.ETAS), list(S.CAPS)) if o.get("apg") else None
        bm = None if "cache" not in o else (o["cache"][0], o["cache"][1], block_cache_schedule(eng.plan, o["cache"][2]))
        x = c.d["noise"].clone()
        with pytest.raises(ValueError) as info:
            eng.transformer_steps_ex(x, c.pre, 0, eng.n_steps, c.host, None, guide=guide, apg=apg, block_modes=bm)
        assert word in str(info.value), (where, str(info.value))
        _after_a_refusal(eng, c, x, c.d["noise"])
        assert torch.equal(c.run().cpu(), want["f32"]), "the next supported call"
