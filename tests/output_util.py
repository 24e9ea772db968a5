"""Shared helpers of the output-stage tests (tests/test_output_cpu.py, tests/test_output_gpu.py)."""
import json
import os

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
_cache = {}


def golden():
    """(meta, arrays) of tests/golden/output_golden.{json,npz}, loaded once."""
    if "g" not in _cache:
        with open(os.path.join(HERE, "golden", "output_golden.json"), encoding="utf-8") as f:
            meta = json.load(f)
        z = np.load(os.path.join(HERE, "golden", "output_golden.npz"))
        _cache["g"] = (meta, {k: z[k] for k in z.files})
    return _cache["g"]


def join_cases():
    """[(name, sample_rate, cross_fade_duration, [chunks], expected)] from the fixture."""
    meta, arr = golden()
    return [(m["name"], m["sample_rate"], m["cross_fade_duration"], [arr[f"j{i}_in_{k}"] for k in range(m["n_chunks"])], arr[f"j{i}_out"])
            for i, m in enumerate(meta["join"])]


def pack_requests(chunk_sets, gap=5):
    """Chunks of several requests laid into one int16 plane with ``gap`` junk samples between them (odd source offsets):
    -> (plane, requests = per request [(src_off, len)])."""
    parts, reqs, pos = [], [], 0
    for chunks in chunk_sets:
        spans = []
        for c in chunks:
            c = np.asarray(c).reshape(-1)
            parts.append(np.full(gap, 32767, np.int16))          # junk that must never be read as part of a chunk
            pos += gap
            parts.append(c)
            spans.append((pos, c.size))
            pos += c.size
        reqs.append(spans)
    parts.append(np.full(gap, 32767, np.int16))
    return np.concatenate(parts), reqs


def emulate_join(plane, requests, cross_fade_duration, sample_rate, plan_join, ring=None):
    """The device algorithm of vv_join_chunks in numpy, from plan_join's rows: flag pass, a walk per request over a position-indexed
    ring, the body pass -- with a write counter per output sample.  -> (out, counts, offsets, lengths)."""
    rows, reqs, lens, ns, total = plan_join(requests, cross_fade_duration, sample_rate)
    C = max(max(ns, default=0), 8) if ring is None else ring
    out = np.full(total, -12345, np.int16)
    cnt = np.zeros(total, np.int32)
    flags = [int(r[6] and (plane[r[0]: r[0] + r[1]] == 32767).any()) for r in rows]
    gains = [np.float32(1)] * len(rows)

    def rep(x, fl):
        return (x * (26214.0 / 32767)).astype(np.int16) if fl else x

    def gained(x, g):
        return (x.astype(np.float32) * g).astype(np.int32).astype(np.int16)

    for c0, nc, oo, jl in reqs:
        if nc < 2:
            continue
        S = np.zeros(C, np.int16)
        r = rows[c0]
        total_ = r[1]
        p = np.arange(max(0, total_ - C), total_)
        S[p % C] = rep(plane[r[0] + p], flags[c0])
        for k in range(1, nc):
            so, ln, P, n, fin, _t, _r, _q = rows[c0 + k]
            fl = flags[c0 + k]
            g = np.float32(1)
            src = rep(plane[so: so + ln], fl)
            if n > 0:
                idx = (P + np.arange(n)) % C
                tail = S[idx]
                rp = np.sqrt(np.mean(tail.astype(np.float32) ** 2))
                rn = np.sqrt(np.mean(src[:n].astype(np.float32) ** 2))
                if rp > 100 and rn > 100:
                    g = np.float32(np.clip(rp / rn, np.float32(0.7), np.float32(1.5)))
                th = np.linspace(0, np.pi / 2, n)
                mixed = (tail.astype(np.float64) * np.cos(th) ** 2 + gained(src[:n], g).astype(np.float64) * np.sin(th) ** 2).astype(np.int16)
                S[idx] = mixed
                pos = P + np.arange(n)
                ok = (pos < fin) & (pos < jl)
                out[oo + pos[ok]] = mixed[ok]
                cnt[oo + pos[ok]] += 1
            gains[c0 + k] = g
            total_new = P + ln
            p = np.arange(max(P + n, total_new - C), total_new)
            S[p % C] = gained(src[p - P], g)
    for ci, (so, ln, P, n, fin, _t, _r, q) in enumerate(rows):
        oo, jl = reqs[q][2], reqs[q][3]
        b = min(P + ln, fin, jl)
        pos = np.arange(P + n, b)
        if pos.size:
            out[oo + pos] = gained(rep(plane[so + pos - P], flags[ci]), gains[ci])
            cnt[oo + pos] += 1
    return out, cnt, [r[2] for r in reqs], lens


def scipy_resample(x, up, down):
    from scipy.signal import resample_poly
    return np.clip(np.rint(resample_poly(np.asarray(x).astype(np.float64), up, down)), -32768, 32767).astype(np.int64)


def lsb_condition(got, want):
    """The issue's condition against scipy: no difference above 1 LSB, at most 1 sample in 10^4 differing.  -> differing samples."""
    got, want = np.asarray(got).astype(np.int64), np.asarray(want).astype(np.int64)
    assert got.shape == want.shape, (got.shape, want.shape)
    d = np.abs(got - want)
    n_diff = int((d > 0).sum())
    assert d.max(initial=0) <= 1, f"difference of {int(d.max())} LSB"
    assert n_diff * 10000 <= max(got.size, 1), f"{n_diff} of {got.size} samples differ"
    return n_diff
