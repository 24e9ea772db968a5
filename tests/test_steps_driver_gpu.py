"""-m gpu: the acoustic stage driver (lane plan, per-lane launches, schedule) against a recording of the build before it was taken apart.

tests/golden/steps_golden.json was written by tests/golden/make_steps_golden.py from ``steps_records`` below, on that earlier build:
ModelSpec.tiny(), fp32 and bf16, nfe_step = 8, two steps per call, over plan x lanes x batch x call form (plain with host lengths, cfg
per item, a guidance mask, APG, APG with the mask), the bf16 options that change the launches, caller-owned blocks of exactly the bytes
asked for, and the refusals of the struct entries and the size queries.  Per call: launches / flops / bytes of every profiling class
and the SHA-256 of x; per (dtype, plan, lanes, batch): the three workspace byte counts; per refusal: the code and vv_last_error.

The batches are those of tests/test_workspace_gpu.py: ``ragged`` runs as item lanes and ``one`` as branch lanes under "lanes" 2.  The
masks give every item its own window of evaluations, so the guided subset changes along a call: rk4 (8 evaluations) sees one item,
two, all, two, one, one again (no new tables), none, none; the Euler calls (2 evaluations) see all then none, and under APG a subset
and its complement.  An evaluation with none guided has no unconditional rows: branch lanes then neither fork nor join.

Engines of this module's own: it changes plans and options (the shared hip_tiny engines are never re-planned)."""
import ctypes as C
import hashlib
import json
import os

import pytest
import torch

from tests.test_workspace_gpu import DEV, LENS, _inputs, _steps_need

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "steps_golden.json")
WHICH = ("ragged", "one")
FORMS = ("plain", "cfg", "mask", "apg", "apg_mask")
CFG, ETA, NORM = [2.5, 1.0, 3.5], [0.5, 0.0, 1.0], [2.5, 0.0, 1.0]          # per item; a norm of 0 = no cap
# the window [lo, hi) of evaluations in which item b is guided, per plan and form
WINDOWS = {"rk4": {"mask": [(1, 4), (2, 6), (0, 3)], "apg_mask": [(1, 4), (2, 6), (0, 3)]},
           "euler": {"mask": [(0, 1), (0, 1), (0, 1)], "apg_mask": [(1, 2), (0, 1), (1, 2)]}}
# bf16 only, plain Euler: (name, option values, rope theta on)
BF16_EXTRA = (("split_k_tail=2", {"split_k_tail": 2}, True), ("rope_rows=1", {"rope_rows": 1}, True), ("rope_theta=0", {}, False),
              ("rope_theta=0 rope_rows=1", {"rope_rows": 1}, False), ("rope_theta=on", {}, True))


def make_engines():
    from vietvoice_tts_amd.model_spec import ModelSpec, make_synthetic_weights
    from vietvoice_tts_amd.runtime import HipSynth
    tiny = ModelSpec.tiny()
    w = make_synthetic_weights(tiny, 9527)
    return {dt: HipSynth(tiny, w, device=DEV, acoustic_dtype=name, nfe_step=8) for dt, name in (("f32", "fp32"), ("bf16", "bf16"))}


def _sha(x):
    torch.cuda.synchronize()
    return hashlib.sha256(x.cpu().numpy().tobytes()).hexdigest()


def _mask(eng, plan, form, B):
    g = torch.zeros((eng.n_evals, B), dtype=torch.uint8)
    for b, (lo, hi) in enumerate(WINDOWS[plan][form][:B]):
        g[lo:hi, b] = 1
    return g


def _form_args(eng, plan, form, B):
    f32 = lambda v: torch.tensor(v[:B], dtype=torch.float32, device=DEV)
    return {"cfg": f32(CFG) if form in ("cfg", "mask") else None,
            "guide": _mask(eng, plan, form, B) if form in ("mask", "apg_mask") else None,
            "apg": (f32(ETA), f32(NORM)) if form in ("apg", "apg_mask") else None}


def _call(eng, x, pre, lens, ws=None, **kw):
    """One two-step call through HipSynth.transformer_steps (with ws: transformer_steps_ex in that caller-owned block) -> its
    profiling account (no times) and the digest of x."""
    eng.prof_collect()
    if ws is None:
        eng.transformer_steps(x, pre, 0, 2, seq_len_host=lens, **kw)
    else:
        eng.transformer_steps_ex(x, pre, 0, 2, (C.c_int32 * len(lens))(*lens), kw["cfg"], ws=ws, guide=kw["guide"], apg=kw["apg"])
    got = eng.prof_collect()
    return {"prof": {cls: {k: v[k] for k in ("launches", "flops", "bytes")} for cls, v in got.items()}, "x": _sha(x)}


def _steps_args(eng, x, pre, host, ws=None):
    from vietvoice_tts_amd.runtime import vv_steps_args
    a = vv_steps_args()
    a.B, a.N, a.seq_len, a.x = x.shape[0], x.shape[1], pre["seq_len"].data_ptr(), x.data_ptr()
    a.seq_len_host = None if host is None else C.cast(host, C.c_void_p)
    a.cat_mel_text, a.cat_mel_text_drop = pre["cat_mel_text"].data_ptr(), pre["cat_mel_text_drop"].data_ptr()
    a.rope_cos_q, a.rope_sin_q = pre["rope_cos_q"].data_ptr(), pre["rope_sin_q"].data_ptr()
    a.rope_cos_k, a.rope_sin_k = pre["rope_cos_k"].data_ptr(), pre["rope_sin_k"].data_ptr()
    a.step0, a.n_steps = 0, 2
    if ws is not None:
        a.ws, a.ws_bytes = ws
    return a


def _refusals(eng, pre, noise, lens, N):
    """(entry: what was wrong) -> [code, vv_last_error] of the bf16 engine under Euler, on the ragged batch; x must stay as it was."""
    from vietvoice_tts_amd.runtime import vv_apg_args
    lib, ctx, B, st = eng.lib, eng.ctx, len(lens), eng._stream()
    x = noise.clone()
    host = (C.c_int32 * B)(*lens)
    guide = _mask(eng, "euler", "mask", B)
    f32 = lambda v: torch.tensor(v[:B], dtype=torch.float32, device=DEV)
    cfg, eta, norm = f32(CFG), f32(ETA), f32(NORM)
    t_host = C.cast(eng._t_host, C.c_void_p)
    apg = vv_apg_args(eta.data_ptr(), norm.data_ptr(), t_host)
    needs = {"vv_transformer_steps_ex": _steps_need(eng, lens, N), "vv_transformer_steps_guided": eng.guided_ws_bytes(B, N, lens),
             "vv_transformer_steps_apg": eng.apg_ws_bytes(B, N, lens)}
    block = torch.zeros((max(needs.values()) + 256,), dtype=torch.uint8, device=DEV)
    assert block.data_ptr() % 256 == 0
    out = {}

    def rec(key, rc):
        out[key] = [int(rc), lib.vv_last_error(ctx).decode()]

    entries = {"vv_transformer_steps_ex": lambda a: lib.vv_transformer_steps_ex(ctx, a, st),
               "vv_transformer_steps_guided": lambda a: lib.vv_transformer_steps_guided(ctx, a, guide.data_ptr(), B, st),
               "vv_transformer_steps_apg": lambda a: lib.vv_transformer_steps_apg(ctx, a, None, 0, C.byref(apg), st)}
    for name, go in entries.items():
        need = needs[name]
        rec(f"{name}: null a", go(None))
        rec(f"{name}: a block without host lengths", go(C.byref(_steps_args(eng, x, pre, None, ws=(block.data_ptr(), need)))))
        a = _steps_args(eng, x, pre, host)
        a.cfg_item = cfg.data_ptr() + 1
        rec(f"{name}: misaligned cfg_item", go(C.byref(a)))
        a = _steps_args(eng, x, pre, host)
        a.n_steps = eng.n_steps + 1
        rec(f"{name}: steps outside the time grid", go(C.byref(a)))
        bad = (C.c_int32 * B)(*lens)
        bad[1] = N + 1
        rec(f"{name}: a length above N", go(C.byref(_steps_args(eng, x, pre, bad))))
        bad[1] = 0
        rec(f"{name}: a length of 0", go(C.byref(_steps_args(eng, x, pre, bad))))
        rec(f"{name}: a block 256 bytes short", go(C.byref(_steps_args(eng, x, pre, host, ws=(block.data_ptr(), need - 256)))))
        rec(f"{name}: a block off alignment", go(C.byref(_steps_args(eng, x, pre, host, ws=(block.data_ptr() + 128, need)))))
    a = _steps_args(eng, x, pre, host)
    rec("vv_transformer_steps_guided: ld_guide < B", lib.vv_transformer_steps_guided(ctx, C.byref(a), guide.data_ptr(), B - 1, st))
    rec("vv_transformer_steps_apg: ld_guide < B", lib.vv_transformer_steps_apg(ctx, C.byref(a), guide.data_ptr(), B - 1, C.byref(apg), st))
    eng.set_option("split_k_tail", 2)
    try:
        rec("vv_transformer_steps_guided: a mask under split_k_tail", lib.vv_transformer_steps_guided(ctx, C.byref(a), guide.data_ptr(), B, st))
        rec("vv_transformer_steps_apg: a mask under split_k_tail", lib.vv_transformer_steps_apg(ctx, C.byref(a), guide.data_ptr(), B, C.byref(apg), st))
    finally:
        eng.set_option("split_k_tail", 0)
    q = vv_apg_args(eta.data_ptr(), norm.data_ptr(), None)
    rec("vv_transformer_steps_apg: no t_host", lib.vv_transformer_steps_apg(ctx, C.byref(a), None, 0, C.byref(q), st))
    q = vv_apg_args(eta.data_ptr() + 2, norm.data_ptr(), t_host)
    rec("vv_transformer_steps_apg: misaligned eta", lib.vv_transformer_steps_apg(ctx, C.byref(a), None, 0, C.byref(q), st))
    q = vv_apg_args(eta.data_ptr(), norm.data_ptr() + 1, t_host)
    rec("vv_transformer_steps_apg: misaligned norm_rms", lib.vv_transformer_steps_apg(ctx, C.byref(a), None, 0, C.byref(q), st))
    many = (C.c_int32 * 1025)(*([1] * 1025))
    nb = C.c_uint64()
    for name in ("vv_transformer_ws_bytes", "vv_transformer_guided_ws_bytes", "vv_transformer_apg_ws_bytes"):
        fn = getattr(lib, name)
        rec(f"{name}: null bytes", fn(ctx, B, N, host, None))
        rec(f"{name}: null lengths", fn(ctx, B, N, None, C.byref(nb)))
        rec(f"{name}: a length above N", fn(ctx, B, N, (C.c_int32 * B)(*[N + 1] * B), C.byref(nb)))
        if name != "vv_transformer_ws_bytes":             # VVK_GUIDE_MAX_ITEMS = 1024 bounds the calls with the mask's tables
            rec(f"{name}: 1025 items", fn(ctx, 1025, N, many, C.byref(nb)))
    assert all(v[0] != 0 for v in out.values()), out
    torch.cuda.synchronize()
    assert torch.equal(x, noise), "a refused call wrote x"
    return out


def steps_records(engs):
    """Everything the golden file pins, through entries and wrappers the library has had since projected guidance."""
    ws, calls, refusals = {}, {}, {}
    try:
        for dt, eng in engs.items():
            eng.prof_enable(True)
            ins = {which: _inputs(eng, which) for which in WHICH}
            for plan in ("euler", "rk4"):
                eng.set_nfe(8, plan)
                for lanes in (1, 2):
                    eng.set_option("lanes", lanes)
                    for which in WHICH:
                        pre, noise, lens, N, _ = ins[which]
                        B, key = len(lens), f"{dt} {plan} lanes={lanes} {which}"
                        ws[key] = [_steps_need(eng, lens, N), eng.guided_ws_bytes(B, N, lens), eng.apg_ws_bytes(B, N, lens)]
                        for form in FORMS:
                            calls[f"{key} {form}"] = _call(eng, noise.clone(), pre, lens, **_form_args(eng, plan, form, B))
                # a caller-owned block of exactly the bytes its query names: plain and APG on item lanes, the mask on branch lanes
                eng.set_option("lanes", 2)
                for which, form, k in (("ragged", "plain", 0), ("one", "mask", 1), ("ragged", "apg", 2)):
                    pre, noise, lens, N, _ = ins[which]
                    need = ws[f"{dt} {plan} lanes=2 {which}"][k]
                    block = torch.zeros((need,), dtype=torch.uint8, device=DEV)
                    assert block.data_ptr() % 256 == 0
                    calls[f"{dt} {plan} lanes=2 {which} {form} in a block"] = _call(eng, noise.clone(), pre, lens, ws=block,
                                                                                    **_form_args(eng, plan, form, len(lens)))
            eng.set_nfe(8, "euler")
            if dt != "bf16":
                continue
            for name, opts, theta_on in BF16_EXTRA:
                try:
                    eng.set_rope_theta(float(eng.spec.rope_theta) if theta_on else 0.0)
                    for k, v in opts.items():
                        eng.set_option(k, v)
                    for lanes in (1, 2):
                        eng.set_option("lanes", lanes)
                        for which in WHICH:
                            pre, noise, lens, N, _ = ins[which]
                            calls[f"{dt} euler lanes={lanes} {which} plain {name}"] = _call(eng, noise.clone(), pre, lens)
                finally:
                    for k in opts:
                        eng.set_option(k, 0)
                    eng.set_rope_theta(float(eng.spec.rope_theta))
            eng.set_option("lanes", 2)
            pre, noise, lens, N, _ = ins["ragged"]
            refusals = _refusals(eng, pre, noise, lens, N)
            calls["bf16 euler lanes=2 ragged plain after the refusals"] = _call(eng, noise.clone(), pre, lens)
    finally:
        for eng in engs.values():
            eng.prof_enable(False)
            for k in ("lanes", "split_k_tail", "rope_rows"):
                eng.set_option(k, 0)
            eng.set_rope_theta(float(eng.spec.rope_theta))
            eng.set_nfe(8, "euler")
    return {"ws_bytes": ws, "calls": calls, "refusals": refusals}


@pytest.fixture(scope="module")
def both():
    """(recorded, replayed): the golden file and the same records from this build, made once for the module."""
    with open(GOLDEN) as f:
        want = json.load(f)
    engs = make_engines()
    try:
        got = steps_records(engs)
    finally:
        for e in engs.values():
            e.close()
    return want, got


def test_the_same_records_are_made(both):
    want, got = both
    for kind in ("ws_bytes", "calls", "refusals"):
        assert got[kind].keys() == want[kind].keys(), kind
    n = len(WHICH) * 2 * 2 * 2
    assert len(want["ws_bytes"]) == n and len(want["calls"]) == n * len(FORMS) + 2 * 2 * 3 + len(BF16_EXTRA) * 4 + 1


def test_workspace_byte_counts_equal_the_recorded_ones(both):
    want, got = both
    for k, v in want["ws_bytes"].items():
        print(f"{k}: {got['ws_bytes'][k]} (recorded {v})")
    assert got["ws_bytes"] == want["ws_bytes"]


def test_profiling_accounts_equal_the_recorded_ones(both):
    want, got = both
    bad = []
    for key, w in want["calls"].items():
        g = got["calls"][key]["prof"]
        assert g.keys() == w["prof"].keys(), key
        for cls, wc in w["prof"].items():
            gc = g[cls]
            if gc["launches"] != wc["launches"]:
                bad.append((key, cls, "launches", gc["launches"], wc["launches"]))
            for k in ("flops", "bytes"):          # the same expressions over the same launches: equal up to the last bit of a sum
                if abs(gc[k] - wc[k]) > 1e-12 * max(abs(gc[k]), abs(wc[k])):
                    bad.append((key, cls, k, gc[k], wc[k]))
    assert not bad, bad[:10]


def test_results_equal_the_recorded_digests(both):
    want, got = both
    bad = [key for key, w in want["calls"].items() if got["calls"][key]["x"] != w["x"]]
    assert not bad, (len(bad), bad[:10])
    # the block is the arena's equal, and a lot of refused calls leaves the context as it was
    for key, w in want["calls"].items():
        for suffix in (" in a block", " after the refusals"):
            if key.endswith(suffix):
                assert w["x"] == want["calls"][key[:-len(suffix)]]["x"], key


def test_refusals_equal_the_recorded_ones(both):
    want, got = both
    for k, v in want["refusals"].items():
        print(f"{k}: {got['refusals'][k]}")
    assert got["refusals"] == want["refusals"]
