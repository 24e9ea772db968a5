"""The pure plans of pcm_stage.py without a GPU.  (1) For every row table of the recorded trace (tests/golden/pcm_stage_golden.*, made on
the commit before the plans existed) the matching plan, given the inputs the golden stores next to it, returns exactly that table and
the sizes the library call was given.  (2) Every refusal the GPU suites provoke through the wrappers is a ValueError of the plan."""
import json
import os
import re

import numpy as np
import pytest

from vietvoice_tts_amd import pcm_stage as P

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "pcm_stage_golden")


@pytest.fixture(scope="module")
def golden():
    with open(GOLDEN + ".json") as f:
        rec = json.load(f)
    with np.load(GOLDEN + ".npz") as z:
        rec["arrays"] = {k: z[k] for k in z.files}
    return rec


def _calls(golden, name):
    """-> per wrapper call ``name``: (its recorded inputs, the library call with tables that followed, the size queries in between)."""
    out = []
    for inp in golden["inputs"]:
        if inp["name"] == name:
            k = next(k for k in range(inp["at"], len(golden["events"])) if "tables" in golden["events"][k])
            ev = golden["events"][k]
            out.append((inp["args"], ev, [golden["arrays"][t] for t in ev["tables"]], golden["events"][inp["at"]: k]))
    assert out, name
    return out


def _n(t):
    return None if t is None or isinstance(t, str) else t["tensor"]


def _out(t):
    return t if t is None or isinstance(t, str) else t["tensor"]


def _same(table, rows, dtype=np.int64):
    return table.tobytes() == np.asarray(rows, dtype=dtype).reshape(table.shape).tobytes()


def _ws(queries, args):
    """The one size query in front of a call was asked with ``args``; -> the bytes the wrapper then allocates."""
    (q,) = [e for e in queries if e["name"].endswith("ws_bytes")]
    assert q["args"] == list(args), q
    return q["ret"] // 8 * 8 + 8


def test_join_tables(golden):
    fade, size = {}, 0                                        # the fade tables grow in the order the junction sizes first appear
    for a, ev, (rows_t, reqs_t), _q in _calls(golden, "join_chunks"):
        rows, reqs, lens, ns, total = P.plan_join(a["requests"], a["cross_fade_duration"], a["sample_rate"], n_pcm=_n(a["pcm"]), out_n=_n(a["out"]),
                                                  out_base=a["out_base"])
        for n in ns:
            if n not in fade:
                fade[n], size = size, size + 2 * n
        for r in rows:
            r[5] = fade[r[3]] if r[3] > 0 else 0
        assert _same(rows_t, rows) and _same(reqs_t, reqs) and lens == [r[3] for r in reqs]
        assert ev["args"] == [_n(a["pcm"]), len(rows), len(reqs), size, max(ns), max(r[1] for r in rows), max(total, 8)]


def test_resample_and_encode_tables(golden):
    from vietvoice_tts_amd.core.audio_processor import output_design
    for a, ev, (t,), _q in _calls(golden, "pcm_resample"):
        taps, up, down, skip = output_design(a["src"], a["dst"])
        rows, n_y, max_out = P.plan_resample(a["rows"], _n(a["x"]), a["n_y"] if a["out"] is None else _n(a["out"]), down, skip)
        assert _same(t, rows) and ev["args"] == [_n(a["x"]), len(rows), max_out, taps.size, up, down, skip, n_y]
    for a, ev, (t,), _q in _calls(golden, "pcm_encode"):
        kind, rows, n_y, max_n = P.plan_encode(a["rows"], a["encoding"], _n(a["x"]), a["n_y"])
        assert _same(t, rows) and ev["args"] == [_n(a["x"]), len(rows), max_n, kind, n_y]


def test_loudness_and_limiter_tables(golden):
    for a, ev, (t, par_t), q in _calls(golden, "pcm_loudness"):
        in_place = isinstance(a["out"], dict) and a["out"]["is_x"]
        sub, rows, par, runs, n_y = P.plan_loudness(a["rows"], a["sr"], a["targets"], a["peak_dbfs"], _n(a["x"]), _out(a["out"]), in_place)
        assert _same(t, rows) and _same(par_t, par, np.float64)
        n_y = 0 if a["out"] == "measure" else _n(a["out"]) or max(n_y, 4)
        assert ev["args"] == [_n(a["x"]), len(rows), sub, n_y, _ws(q, [runs, len(rows)])] and ev["same"] == ([[1, 9]] if in_place else [])
    tiles = {e["args"][0]: e["ret"] for e in golden["events"] if e["name"] == "vv_pcm_limit_tile"}
    for a, ev, (t, par_t), q in _calls(golden, "pcm_limit"):
        in_place = isinstance(a["out"], dict) and a["out"]["is_x"]
        L, mode, rows, par, samples, n_tiles, n_y = P.plan_limit(a["rows"], a["sr"], a["peak_dbfs"], a["mode"], a["gain"], a["targets"], a["meas"] is not None,
                                                                 a["L"], lambda L: tiles[L], _n(a["x"]), _out(a["out"]), in_place)
        assert _same(t, rows) and _same(par_t, par, np.float64)
        n_y = _n(a["out"]) or max(n_y, 4)
        assert ev["args"] == [_n(a["x"]), len(rows), L, mode, n_y, _ws(q, [samples, n_tiles, len(rows)])]
        assert (11 in ev["null"]) == (a["meas"] is None) and ev["same"] == ([[1, 12]] if in_place else [])


def test_stretch_and_prosody_tables(golden):
    for a, ev, (t,), q in _calls(golden, "pcm_stretch"):
        rows, pos_offs, n_y = P.plan_stretch(a["rows"], _n(a["x"]), _out(a["out"]), False)
        assert _same(t, rows) and ev["args"] == [_n(a["x"]), len(rows), _n(a["out"]) or max(n_y, 4), pos_offs[-1], _ws(q, [len(rows)])]
    inputs, seen = golden["inputs"], set()
    for k, inp in enumerate(inputs):
        if inp["name"] != "_prosody":
            continue
        a = inp["args"]
        new_offs, new_lens, base, size, copies, stretch, converts = P.plan_prosody(a["offs"], a["lens"], a["pitch"], a["tempo"])
        after = []
        for nxt in inputs[k + 1:]:
            if nxt["name"] not in ("pcm_stretch", "pcm_resample") or len(after) == bool(stretch) + len(converts):
                break
            after.append(nxt)
        want = ([("pcm_stretch", stretch, size)] if stretch else []) + [("pcm_resample", rows, base, p_r, q_r, from_new) for from_new, p_r, q_r, rows in converts]
        assert len(after) == len(want) and want
        for got, w in zip(after, want):
            g = got["args"]
            assert got["name"] == w[0] and g["rows"] == w[1] and g["out"]["tensor"] == w[2]
            if w[0] == "pcm_resample":
                assert (g["src"], g["dst"]) == w[3:5] and g["x"]["tensor"] == (size - base if w[5] else a["buf"]["tensor"])
                seen.add("new" if w[5] else "joined")
        assert sorted(s for s, _d, n in copies) == [o for o, p, t in zip(a["offs"], a["pitch"], a["tempo"]) if p is None and t is None]
        assert all(o % 8 == 0 for o in new_offs) and base % 8 == 0 and len(new_lens) == len(a["lens"])
    assert seen == {"new", "joined"}                          # both sources of the rate conversion are in the trace


def test_flac_tables(golden):
    for a, ev, (t,), q in _calls(golden, "pcm_flac"):
        order, rows, n_y, frames = P.plan_flac(a["rows"], _n(a["x"]), a["sample_rate"], a["lpc_order"])
        ws = _ws(q, [frames, len(rows)] + ([order] if order else []))
        assert _same(t, rows) and ev["args"] == [_n(a["x"]), len(rows), a["sample_rate"]] + ([order] if order else []) + [n_y, ws]
        assert ev["name"] == ("vv_pcm_flac_lpc" if order else "vv_pcm_flac")
    for a, ev, (t,), q in _calls(golden, "flac_index"):
        rows = P.plan_flac_index(a["rows"], _n(a["data"]))
        assert _same(t, rows) and ev["args"] == [_n(a["data"]), len(rows), _ws(q, [_n(a["data"]), len(rows)])]
    for a, ev, (clips_t, lay_t), q in _calls(golden, "flac_decode"):
        full, frames, plane = P.plan_flac_decode(a["lay"], a["index"], _n(a["pcm"]))
        assert _same(clips_t, a["index"]) and _same(lay_t, full)
        assert ev["args"][-2:] == [_n(a["pcm"]), _ws(q, [plane, frames])] and any(r[1] == 0 for r in a["lay"])      # a refused clip among them


def test_finish_output_groups(golden):
    inputs = golden["inputs"]
    starts = [k for k, inp in enumerate(inputs) if inp["name"] == "finish_output"]
    modes = set()
    last = next(k for k, inp in enumerate(inputs) if inp["name"] == "flac_index")      # behind the last finish_output: flac_clips and the streams
    for k, end in zip(starts, starts[1:] + [last]):
        a = inputs[k]["args"]
        inner = [inp for inp in inputs[k + 1: end] if inp["name"] in ("_prosody", "pcm_loudness", "pcm_limit")]
        pitch, tempo, groups = P.plan_finish(len(a["plans"]), a["loudness"], a["limiter"], a["pitch"], a["tempo"])
        want = [] if pitch is None else [("_prosody", pitch, tempo)]
        for mode, sel, tg in groups:
            modes.add(mode)
            if mode is None:
                want.append(("pcm_loudness", len(sel), tg, True))
                continue
            if any(t is not None for t in tg):
                want.append(("pcm_loudness", len(sel), tg, "measure"))
            want.append(("pcm_limit", len(sel), mode, tg if any(t is not None for t in tg) else None))
        got = []
        for inp in inner:
            g = inp["args"]
            if inp["name"] == "_prosody":
                got.append(("_prosody", g["pitch"], g["tempo"]))
            elif inp["name"] == "pcm_loudness":
                tg = g["targets"] if isinstance(g["targets"], list) else [g["targets"]] * len(g["rows"])
                got.append(("pcm_loudness", len(g["rows"]), tg, g["out"] if isinstance(g["out"], str) else g["out"]["is_x"]))
            else:
                got.append(("pcm_limit", len(g["rows"]), g["mode"], g["targets"]))
        assert got == want, a
    assert modes == {None, "sample", "true"}


def test_place():
    assert P._place([0, 700, 9610, 19600], 8) == ([0, 0, 704, 10320], 29920) and P._place([3, 0, 5]) == ([0, 3, 3], 8) and P._place([], 4) == ([], 0)


LIM = (24000, -1.0, "true", 1.0, None, False, 3, lambda L: 64, 100)       # plan_limit's arguments behind the rows, all good
CLIP = [0, 100, 1, 16, 4096, 4096, 24000, 0]                                # one good row of flac_index


def _limit(rows, **kw):
    a = dict(zip(("sr", "peak_dbfs", "mode", "gain", "targets", "has_meas", "L", "tile", "n_x"), LIM), out_n=None, in_place=False)
    a.update(kw)
    return P.plan_limit(rows, a["sr"], a["peak_dbfs"], a["mode"], a["gain"], a["targets"], a["has_meas"], a["L"], a["tile"], a["n_x"], a["out_n"], a["in_place"])


# (what is wrong, how the message starts: the entry's name, or the option's where core.audio_processor's own check speaks, as before; the call)
REFUSALS = [
    # wrong row width, no rows, too many rows
    ("resample width", "pcm_resample: rows of 6 entries", lambda: P.plan_resample([[0, 10, 0, 10, 0]], 100, None, 3, 4)),
    ("encode width", "pcm_encode: rows of 3 entries", lambda: P.plan_encode([[0, 10]], "ulaw", 100, None)),
    ("loudness width", "pcm_loudness: 1 to 65535 rows of 3 entries", lambda: P.plan_loudness([[0, 10]], 24000, -23.0, -1.0, 100)),
    ("limit width", "pcm_limit: 1 to 65535 rows of 3 entries", lambda: _limit([[0, 10]])),
    ("limit width 4", "pcm_limit: 1 to 65535 rows of 3 entries", lambda: _limit([[0, 10, 0, 0]])),
    ("stretch width", "pcm_stretch: 1 to 65535 rows of 5 entries", lambda: P.plan_stretch([[0, 10, 0, 3]], 100)),
    ("flac width", "pcm_flac: 1 to 65535 rows of 4 entries", lambda: P.plan_flac([[0, 10, 0]], 100, 24000)),
    ("flac_index width", "flac_index: 1 to 65535 rows of 8 entries", lambda: P.plan_flac_index([CLIP[:7]], 1000)),
    ("flac_decode width", "flac_decode: one row", lambda: P.plan_flac_decode([[0, 1]], [CLIP], 1000)),
    ("encode no rows", "pcm_encode: rows of 3 entries", lambda: P.plan_encode([], "ulaw", 100, None)),
    ("stretch no rows", "pcm_stretch: 1 to 65535 rows", lambda: P.plan_stretch([], 100)),
    ("flac no rows", "pcm_flac: 1 to 65535 rows", lambda: P.plan_flac([], 100, 24000)),
    ("loudness too many rows", "pcm_loudness: 1 to 65535 rows", lambda: P.plan_loudness([[0, 1, 0]] * 65536, 24000, -23.0, -1.0, 100, "measure")),
    # overlap on the output
    ("resample overlap", "pcm_resample: rows overlap on the output", lambda: P.plan_resample([[0, 30, 0, 10, 0, 0], [30, 30, 5, 10, 0, 0]], 100, None, 3, 4)),
    ("encode overlap", "pcm_encode: rows overlap on the output", lambda: P.plan_encode([[0, 10, 0], [20, 10, 5]], "ulaw", 65536, None)),
    ("loudness overlap", "pcm_loudness: rows overlap on the output", lambda: P.plan_loudness([[0, 10, 0], [20, 10, 5]], 24000, -23.0, -1.0, 100)),
    ("limit overlap", "pcm_limit: rows overlap on the output", lambda: _limit([[0, 10, 0], [20, 10, 5]])),
    ("stretch overlap", "pcm_stretch: rows overlap on the output", lambda: P.plan_stretch([[0, 10, 0, 3, 2], [20, 10, 5, 3, 2]], 100)),
    # a row past x, a row past out, a negative field
    ("resample past x", "pcm_resample: row [95, 10, 0, 4, 0, 0] does not fit", lambda: P.plan_resample([[95, 10, 0, 4, 0, 0]], 100, None, 3, 4)),
    ("resample past out", "pcm_resample: row [0, 30, 5, 10, 0, 0] does not fit", lambda: P.plan_resample([[0, 30, 5, 10, 0, 0]], 100, 14, 3, 4)),
    ("encode past x", "pcm_encode: row [65530, 10, 0] does not fit", lambda: P.plan_encode([[65530, 10, 0]], "ulaw", 65536, None)),
    ("encode past out", "pcm_encode: row [0, 10, 5] does not fit", lambda: P.plan_encode([[0, 10, 5]], "alaw", 100, 14)),
    ("encode kind", "pcm_encode: encoding is", lambda: P.plan_encode([[0, 10, 0]], "pcm16", 100, None)),
    ("loudness past x", "pcm_loudness: row [95, 10, 0] does not fit", lambda: P.plan_loudness([[95, 10, 0]], 24000, -23.0, -1.0, 100)),
    ("loudness past out", "pcm_loudness: out holds 14 samples, 15 are needed", lambda: P.plan_loudness([[0, 10, 5]], 24000, -23.0, -1.0, 100, 14)),
    ("limit past x", "pcm_limit: row [95, 10, 0, 0, 10] does not fit", lambda: _limit([[95, 10, 0]])),
    ("limit past out", "pcm_limit: out holds 14 samples, 15 are needed", lambda: _limit([[0, 10, 5]], out_n=14)),
    ("stretch past x", "pcm_stretch: row [95, 10, 0, 3, 2] does not fit", lambda: P.plan_stretch([[95, 10, 0, 3, 2]], 100)),
    ("stretch past out", "pcm_stretch: out holds 14 samples, 15 are needed", lambda: P.plan_stretch([[0, 10, 0, 3, 2]], 100, 14)),
    ("stretch negative dst_off", "pcm_stretch: row [0, 10, -1, 3, 2] does not fit", lambda: P.plan_stretch([[0, 10, -1, 3, 2]], 100)),
    ("stretch onto x", "pcm_stretch: out overlaps x", lambda: P.plan_stretch([[0, 10, 0, 3, 2]], 100, 100, True)),
    ("flac past x", "pcm_flac: row [95, 10, 0, 1] does not fit", lambda: P.plan_flac([[95, 10, 0, 1]], 100, 24000)),
    ("join past pcm", "join_chunks: chunk (150, 100) does not fit", lambda: P.plan_join([[(150, 100)]], 0.1, 24000, n_pcm=200)),
    ("join past out", "join_chunks: out holds 99 samples, 100 are needed", lambda: P.plan_join([[(0, 100)]], 0.1, 24000, n_pcm=200, out_n=99)),
    ("join out_base", "join_chunks: out_base must be", lambda: P.plan_join([[(0, 100)]], 0.1, 24000, out_base=4)),
    ("join empty chunk", "join_chunks: an empty chunk", lambda: P.plan_join([[(0, 100), (100, 0)]], 0.1, 24000, n_pcm=200)),
    ("join junction", "join_chunks: a junction of 36000 samples, more than", lambda: P.plan_join([[(0, 60000), (60000, 60000)]], 1.5, 24000, n_pcm=120000)),
    # in place with shifted offsets
    ("loudness in place", "pcm_loudness: in place needs dst_off == src_off", lambda: P.plan_loudness([[0, 10, 20]], 24000, -23.0, -1.0, 100, 100, True)),
    ("limit in place", "pcm_limit: in place needs dst_off == src_off + out_lo", lambda: _limit([[0, 10, 1, 0, 5]], out_n=100, in_place=True)),
    # out_lo + out_n > n; a target without meas; the gain; the mode; the look-ahead; the ceiling; the rate; the target
    ("limit window", "pcm_limit: row [0, 10, 0, 5, 6] does not fit", lambda: _limit([[0, 10, 0, 5, 6]])),
    ("limit target without meas", "pcm_limit: a loudness target needs meas", lambda: _limit([[0, 10, 0]], targets=-23.0)),
    ("limit gain 0", "pcm_limit: the gain must be", lambda: _limit([[0, 10, 0]], gain=0.0)),
    ("limit gain -1", "pcm_limit: the gain must be", lambda: _limit([[0, 10, 0]], gain=[-1.0])),
    ("limit gain inf", "pcm_limit: the gain must be", lambda: _limit([[0, 10, 0]], gain=float("inf"))),
    ("limit gains", "pcm_limit: one target and one gain per row", lambda: _limit([[0, 10, 0]], gain=[1.0, 1.0])),
    ("limit mode None", "pcm_limit: a mode is needed", lambda: _limit([[0, 10, 0]], mode=None)),
    ("limit mode peak", "output_limiter must be", lambda: _limit([[0, 10, 0]], mode="peak")),
    ("limit L 0", "limiter: the look-ahead", lambda: _limit([[0, 10, 0]], L=0)),
    ("limit L 1025", "limiter: the look-ahead", lambda: _limit([[0, 10, 0]], L=1025)),
    ("limit rate", "limiter: a look-ahead of 0.005 s at 400000 Hz is 2000 samples", lambda: _limit([[0, 10, 0]], sr=400000, L=None)),
    ("limit ceiling", "output_peak_dbfs", lambda: _limit([[0, 10, 0]], peak_dbfs=1.0)),
    ("loudness rate 1000", "pcm_loudness: the sample rate must be", lambda: P.plan_loudness([[0, 10, 0]], 1000, -23.0, -1.0, 100)),
    ("loudness rate 22055", "pcm_loudness: the sample rate must be", lambda: P.plan_loudness([[0, 10, 0]], 22055, -23.0, -1.0, 100)),
    ("loudness targets", "pcm_loudness: one target per row", lambda: P.plan_loudness([[0, 10, 0]], 24000, [-23.0, -16.0], -1.0, 100)),
    ("loudness target -70", "output_loudness", lambda: P.plan_loudness([[0, 10, 0]], 24000, -70.0, -1.0, 100)),
    ("loudness ceiling", "output_peak_dbfs", lambda: P.plan_loudness([[0, 10, 0]], 24000, -23.0, 1.0, 100)),
    # bad p / q
    ("stretch p == q", "time_stretch: p and q in", lambda: P.plan_stretch([[0, 10, 0, 5, 5]], 100)),
    ("stretch p / q > 4", "time_stretch: p and q in", lambda: P.plan_stretch([[0, 10, 0, 9, 2]], 100)),
    ("stretch p / q < 1 / 4", "time_stretch: p and q in", lambda: P.plan_stretch([[0, 10, 0, 1, 5]], 100)),
    ("stretch q = 0", "time_stretch: p and q in", lambda: P.plan_stretch([[0, 10, 0, 3, 0]], 100)),
    ("stretch p > 2048", "time_stretch: p and q in", lambda: P.plan_stretch([[0, 10, 0, 4096, 2048]], 100)),
    # last = 0 with a ragged block; an empty row; the frame numbers; last; the rate; the order
    ("flac ragged", "pcm_flac: row [0, 5000, 0, 0] does not fit", lambda: P.plan_flac([[0, 5000, 0, 0]], 10000, 24000)),
    ("flac ragged 10", "pcm_flac: row [0, 10, 0, 0] does not fit", lambda: P.plan_flac([[0, 10, 0, 0]], 100, 24000)),
    ("flac empty", "pcm_flac: row [0, 0, 0, 1] does not fit", lambda: P.plan_flac([[0, 0, 0, 1]], 100, 24000)),
    ("flac frame0 2^31", "pcm_flac: row [0, 10, 2147483648, 1] does not fit", lambda: P.plan_flac([[0, 10, 1 << 31, 1]], 100, 24000)),
    ("flac frame0 -1", "pcm_flac: row [0, 10, -1, 1] does not fit", lambda: P.plan_flac([[0, 10, -1, 1]], 100, 24000)),
    ("flac last 2", "pcm_flac: row [0, 10, 0, 2] does not fit", lambda: P.plan_flac([[0, 10, 0, 2]], 100, 24000)),
    ("flac rate 8000.5", "pcm_flac: a sample rate in", lambda: P.plan_flac([[0, 10, 0, 1]], 100, 8000.5)),
    ("flac rate 0", "pcm_flac: a sample rate in", lambda: P.plan_flac([[0, 10, 0, 1]], 100, 0)),
    ("flac rate 655351", "pcm_flac: a sample rate in", lambda: P.plan_flac([[0, 10, 0, 1]], 100, 655351)),
    ("flac order 13", "flac_lpc_order", lambda: P.plan_flac([[0, 10, 0, 1]], 100, 24000, 13)),
    ("flac order -1", "flac_lpc_order", lambda: P.plan_flac([[0, 10, 0, 1]], 100, 24000, -1)),
    ("flac order 2.0", "flac_lpc_order", lambda: P.plan_flac([[0, 10, 0, 1]], 100, 24000, 2.0)),
    ("flac order True", "flac_lpc_order", lambda: P.plan_flac([[0, 10, 0, 1]], 100, 24000, True)),
    # descending FLAC clip offsets, a clip into the padding, a layout past pcm or out of order
    ("flac_index descending", "flac_index: row [0, 100, 1, 16, 4096, 4096, 24000, 0] does not fit", lambda: P.plan_flac_index([[100] + CLIP[1:], CLIP], 1000)),
    ("flac_index padding", "flac_index: row [0, 996,", lambda: P.plan_flac_index([[0, 996] + CLIP[2:]], 1000)),
    ("flac_index bits", "flac_index: row [0, 100, 1, 12,", lambda: P.plan_flac_index([CLIP[:3] + [12] + CLIP[4:]], 1000)),
    ("flac_index data", "flac_index: 8 ... 2^31 - 64 bytes of data", lambda: P.plan_flac_index([[0, 0] + CLIP[2:]], 4)),
    ("flac_index alignment", "flac_index: 8 ... 2^31 - 64 bytes of data, 8-byte aligned", lambda: P.plan_flac_index([CLIP], 1000, False)),
    ("flac_decode past pcm", "flac_decode: row [0, 1, 600] does not fit", lambda: P.plan_flac_decode([[0, 1, 600]], [CLIP], 1000)),
    ("flac_decode descending", "flac_decode: row [0, 1, 10] does not fit", lambda: P.plan_flac_decode([[100, 1, 10], [0, 1, 10]], [CLIP] * 2, 1000)),
    # finish_output: one entry per request
    ("finish loudness", "finish_output: one loudness entry per request", lambda: P.plan_finish(2, loudness=[-23.0])),
    ("finish limiter", "finish_output: one limiter entry per request", lambda: P.plan_finish(2, limiter=["true"])),
    ("finish limiter mode", "output_limiter must be", lambda: P.plan_finish(2, limiter="loud")),
    ("finish pitch", "finish_output: one pitch and one tempo entry per request", lambda: P.plan_finish(2, pitch=[1.0, None, None])),
]


@pytest.mark.parametrize("case", range(len(REFUSALS)), ids=[r[0].replace(" ", "_") for r in REFUSALS])
def test_refusals(case):
    _what, starts, call = REFUSALS[case]
    with pytest.raises(ValueError, match="^" + re.escape(starts)):
        call()


def test_good_rows_next_to_the_refused_ones_pass():
    assert _limit([[0, 10, 1, 1, 5]], out_n=100, in_place=True)[2] == [[0, 10, 1, 1, 5]]
    assert P.plan_loudness([[0, 10, 0]], 24000, None, -1.0, 100, 100, True)[4] == 10
    assert P.plan_stretch([[0, 10, 0, 3, 2]], 100, "positions", True)[1] == [0, 2]
    assert P.plan_flac([[0, 8192, 7, 0]], 10000, 24000)[3] == 2
    assert P.plan_join([[(0, 100), (100, 100)]], 10 / 24000 + 1e-12, 24000, n_pcm=200)[2] == [190]
