#!/usr/bin/env python3
"""The look-ahead limiter in the output stage: what `limiter=` costs between the end of vv_decode (int16 chunks in
HBM) and the final bytes on the host.

  plain     HipSynth.finish_output at 24 kHz pcm16 (join, one copy)
  limited   the same call with limiter="true": join -> vv_pcm_limit in place -> one copy
  loud      the same call with loudness=-16 and limiter="true": join -> vv_pcm_loudness (measure) -> vv_pcm_limit -> one copy
  mirror    audio_processor.limit_peaks on the same joined PCM, on the host (what a caller without the kernel would run after the copy)

on three workloads at full size: B = 1 and B = 32 one-chunk requests of the headline length (~11 s), and one 5-minute request of 30
chunks.  The paths are alternated inside every repetition, each timed by a host clock around work that ends with the bytes on the
host; medians of --reps windows.  The call alone is timed with device events around one vv_pcm_limit call on the joined buffer, in both
modes and measuring only (no apply pass); these include the upload of the descriptor rows.  The four launches of one call are not timed
one by one here; they come from a kernel trace of this program:
    rocprofv3 --kernel-trace --stats -- python tools/limiter_bench.py --reps 5
Before timing, the device result is checked against the mirror (equal, bit for bit).

    python tools/limiter_bench.py [--reps 21] [--out profiles/limiter/limiter_bench.json]

Prints one JSON line.  There is nothing to measure without a HIP device."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402

from vietvoice_tts_amd import runtime as rt  # noqa: E402
from vietvoice_tts_amd.core.audio_processor import limit_peaks  # noqa: E402
from vietvoice_tts_amd.model_spec import ModelSpec, make_synthetic_weights  # noqa: E402

SR, CF, HOP, TARGET, PEAK = 24000, 0.1, 256, -16.0, -1.0


def workload(name, dev):
    """-> (plane int16 [B][ld] on the device, host lengths, requests as lists of rows): seeded noise under a slow envelope whose crests
    pass the ceiling, so that the limiter has work in part of every request and none in the rest."""
    rng = np.random.default_rng(5)
    if name == "b1":
        frames, reqs = [1031], [[0]]                    # 11 s
    elif name == "b32":
        frames, reqs = [int(v) for v in rng.integers(900, 1100, size=32)], [[i] for i in range(32)]
    else:
        frames, reqs = [int(v) for v in rng.integers(920, 960, size=30)], [list(range(30))]      # ~5 minutes in one request
    lens = [f * HOP for f in frames]
    plane = np.zeros((len(lens), max(lens)), np.int16)
    for i, n in enumerate(lens):
        env = 0.55 + 0.45 * np.cos(2 * np.pi * 0.7 * np.arange(n) / SR + i)
        plane[i, :n] = np.clip(rng.standard_normal(n) * 9000 * env, -32768, 32767).astype(np.int16)
    return torch.from_numpy(plane).to(dev), lens, reqs


def events_ms(fn, reps):
    ts = []
    for _ in range(reps + 2):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ts.append(a.elapsed_time(b))
    return float(np.median(ts[2:]))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=21)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "limiter_bench times the GPU path; there is nothing to measure without a HIP device"
    spec = ModelSpec.tiny()                   # the kernels under the clock take their sizes as arguments; the context can be small
    eng = rt.HipSynth(spec, make_synthetic_weights(spec), acoustic_dtype="bf16", nfe_step=4)
    res = {"metric": "output_limiter", "reps": a.reps, "sample_rate": SR, "peak_dbfs": PEAK, "lookahead": 120}
    for name in ("b1", "b32", "longform5min"):
        plane, lens, reqs = workload(name, eng.device)
        ld = plane.shape[1]
        plans = [[(i * ld, lens[i]) for i in r] for r in reqs]
        paths = {"plain": lambda: eng.finish_output(plane, plans, CF, SR),
                 "limited": lambda: eng.finish_output(plane, plans, CF, SR, peak_dbfs=PEAK, limiter="true"),
                 "loud": lambda: eng.finish_output(plane, plans, CF, SR, loudness=TARGET, peak_dbfs=PEAK, limiter="true")}
        joined, got = paths["plain"](), paths["limited"]()
        mirror_ts, limited_share = [], 0.0
        for _ in range(3):                     # the first pass builds the tables and warms numpy: not timed
            t0 = time.perf_counter()
            want = [limit_peaks(j, SR, PEAK, "true") for j in joined]
            mirror_ts.append((time.perf_counter() - t0) * 1e3)
        mirror_ms = float(np.median(mirror_ts[1:]))
        assert all(np.array_equal(w[0], g) for w, g in zip(want, got)), "the device result differs from the host mirror"
        limited_share = sum(w[1]["n_limited"] for w in want) / max(1, sum(j.size for j in joined))
        ts = {k: [] for k in paths}
        for i in range(a.reps + 2):
            for k, fn in paths.items():        # alternated: the paths see the same box at the same time
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                fn()
                if i >= 2:
                    ts[k].append((time.perf_counter() - t0) * 1e3)
        buf, offs, ns = eng.join_chunks(plane.reshape(-1), plans, CF, SR)
        rows = [[o, n, o] for o, n in zip(offs, ns)]
        out = torch.empty_like(buf)
        med = {k: float(np.median(v)) for k, v in ts.items()}
        res[name] = {
            "requests": len(reqs), "chunks": len(lens), "audio_s": round(sum(j.size for j in joined) / SR, 1),
            "samples_limited_share": round(limited_share, 4),
            "plain_ms": round(med["plain"], 3), "limited_ms": round(med["limited"], 3), "loud_ms": round(med["loud"], 3),
            "added_ms": round(med["limited"] - med["plain"], 3), "added_over_plain": round(med["limited"] / med["plain"] - 1, 3),
            "mirror_ms": round(mirror_ms, 1),
            "call_true_ms": round(events_ms(lambda: eng.pcm_limit(buf, rows, SR, PEAK, "true", out=out), a.reps), 4),
            "call_sample_ms": round(events_ms(lambda: eng.pcm_limit(buf, rows, SR, PEAK, "sample", out=out), a.reps), 4),
            "measure_only_ms": round(events_ms(lambda: eng.pcm_limit(buf, rows, SR, PEAK, "true", out="measure"), a.reps), 4),
            "spread_ms": {k: [round(min(v), 3), round(max(v), 3)] for k, v in ts.items()},
        }
    eng.close()
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
