#!/usr/bin/env python3
"""Pitch and tempo in the output stage: what `tempo=` and `pitch=` cost between the end of vv_decode (int16 chunks in
HBM) and the final bytes on the host.

  plain     HipSynth.finish_output at 24 kHz pcm16 (join, one copy)
  tempo     the same call with tempo=2/3 (the stretch by 3/2 alone): join -> vv_pcm_stretch -> one copy
  pitch     the same call with pitch=3 (stretch by 25/21, then vv_pcm_resample 25 -> 21): join -> stretch -> rate conversion -> one copy
  mirror    audio_processor.time_stretch on the same joined PCM, on the host

on three workloads at full size: B = 1 and B = 32 one-chunk requests of the headline length (~11 s), and one 5-minute request of 30
chunks.  The paths are alternated inside every repetition, each timed by a host clock around work that ends with the bytes on the
host; medians of --reps windows.  The search pass alone (vv_pcm_stretch with y = NULL: the frame positions, no sample) and the whole
call are timed with device events on the joined buffer; both include the upload of the descriptor rows.  One workgroup walks a
request's frames in order, so the search time follows the LONGEST request of a call, not the sum.
Before timing, the device result is checked against the mirror (equal, bit for bit).

    python tools/prosody_bench.py [--reps 11] [--out profiles/prosody/prosody_bench.json]

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
from vietvoice_tts_amd.core.audio_processor import WSOLA_HS, prosody_plan, time_stretch  # noqa: E402
from vietvoice_tts_amd.model_spec import ModelSpec, make_synthetic_weights  # noqa: E402

SR, CF, HOP, TEMPO, PITCH = 24000, 0.1, 256, 2.0 / 3.0, 3


def workload(name, dev):
    """-> (plane int16 [B][ld] on the device, host lengths, requests as lists of rows): a harmonic signal with a wandering pitch under
    seeded noise, so that the search has a periodicity to find."""
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
        t = np.arange(n) / SR
        phase = 2 * np.pi * np.cumsum(110.0 + 30.0 * np.sin(2 * np.pi * 0.8 * t + i)) / SR
        v = 7000 * np.sin(phase) + 3000 * np.sin(3 * phase + 1.0) + 1200 * rng.standard_normal(n)
        plane[i, :n] = np.clip(v, -32768, 32767).astype(np.int16)
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
    ap.add_argument("--reps", type=int, default=11)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "prosody_bench times the GPU path; there is nothing to measure without a HIP device"
    spec = ModelSpec.tiny()                   # the kernels under the clock take their sizes as arguments; the context can be small
    eng = rt.HipSynth(spec, make_synthetic_weights(spec), acoustic_dtype="bf16", nfe_step=4)
    plan = prosody_plan(1000, None, TEMPO)
    res = {"metric": "output_prosody", "reps": a.reps, "sample_rate": SR, "tempo": TEMPO, "stretch": [plan.p, plan.q], "pitch": PITCH}
    for name in ("b1", "b32", "longform5min"):
        plane, lens, reqs = workload(name, eng.device)
        ld = plane.shape[1]
        plans = [[(i * ld, lens[i]) for i in r] for r in reqs]
        paths = {"plain": lambda: eng.finish_output(plane, plans, CF, SR),
                 "tempo": lambda: eng.finish_output(plane, plans, CF, SR, tempo=TEMPO),
                 "pitch": lambda: eng.finish_output(plane, plans, CF, SR, pitch=PITCH)}
        joined, got = paths["plain"](), paths["tempo"]()
        t0 = time.perf_counter()
        want = [time_stretch(j, plan.p, plan.q)[0] for j in joined]
        mirror_ms = (time.perf_counter() - t0) * 1e3
        assert all(np.array_equal(w, g) for w, g in zip(want, got)), "the device result differs from the host mirror"
        ts = {k: [] for k in paths}
        for i in range(a.reps + 2):
            for k, fn in paths.items():        # alternated: the paths see the same box at the same time
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                fn()
                if i >= 2:
                    ts[k].append((time.perf_counter() - t0) * 1e3)
        buf, offs, ns = eng.join_chunks(plane.reshape(-1), plans, CF, SR)
        rows, dst = [], 0
        for o, n in zip(offs, ns):
            rows.append([o, n, dst, plan.p, plan.q])
            dst = -(-(dst + -(-n * plan.p // plan.q)) // 8) * 8
        out = torch.empty((max(dst, 8),), dtype=torch.int16, device=eng.device)
        frames = [-(-(-(-n * plan.p // plan.q)) // WSOLA_HS) for n in ns]
        med = {k: float(np.median(v)) for k, v in ts.items()}
        search_ms = events_ms(lambda: eng.pcm_stretch(buf, rows, out="positions"), a.reps)
        res[name] = {
            "requests": len(reqs), "chunks": len(lens), "audio_s": round(sum(j.size for j in joined) / SR, 1),
            "frames_total": int(sum(frames)), "frames_longest_request": int(max(frames)),
            "plain_ms": round(med["plain"], 3), "tempo_ms": round(med["tempo"], 3), "pitch_ms": round(med["pitch"], 3),
            "tempo_added_ms": round(med["tempo"] - med["plain"], 3), "pitch_added_ms": round(med["pitch"] - med["plain"], 3),
            "mirror_ms": round(mirror_ms, 1),
            "search_alone_ms": round(search_ms, 4), "search_us_per_frame_of_longest": round(1e3 * search_ms / max(frames), 3),
            "call_ms": round(events_ms(lambda: eng.pcm_stretch(buf, rows, out=out), a.reps), 4),
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
