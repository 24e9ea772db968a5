#!/usr/bin/env python3
"""Formant-preserving pitch shift in the output stage: what `formants="keep"` costs on top of `pitch=` between the end of
vv_decode (int16 chunks in HBM) and the final bytes on the host.

  plain     HipSynth.finish_output at 24 kHz pcm16 (join, one copy)
  shift     the same call with pitch=4 (stretch by 34/27, then vv_pcm_resample 34 -> 27): today's pitch, the envelope moves
  keep      the same call with pitch=4, formants="keep": ... -> vv_pcm_formant -> one copy

on two workloads at full size: B = 1 and B = 32 one-chunk requests of the headline length (~11 s).  The paths are alternated inside every
repetition, each timed by a host clock around work that ends with the bytes on the host; medians of --reps windows.  vv_pcm_formant alone
(the wrapper call on the joined and the shifted buffer, descriptor upload and workspace allocation included) is timed with device events.
The operations of the tap sums are counted from the shapes: 4 L per output sample (two filters, one multiply and one add per tap, never
fused), against the chip's vector float64 rate for separate multiplies and adds (half the fused peak).  The three kernels' own times come
from a profiler run of this same tool (see profiles/formant/notes.md), not from here.
Before timing, the device result on a 1 s request is checked against the mirror (equal, bit for bit).

    python tools/formant_bench.py [--reps 11] [--workloads b1,b32] [--out profiles/formant/formant_bench.json]
    rocprofv3 --kernel-trace --stats -d <dir> -o formant -- python tools/formant_bench.py --reps 3 --workloads b32     (the three kernels)

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
from vietvoice_tts_amd.core.audio_processor import FORMANT_H, FORMANT_L, FORMANT_P, keep_formants, prosody_plan  # noqa: E402
from vietvoice_tts_amd.model_spec import ModelSpec, make_synthetic_weights  # noqa: E402

SR, CF, HOP, PITCH = 24000, 0.1, 256, 4
FP64_VECTOR_PEAK = 78.6e12          # fused multiply-adds counted as two; separate multiplies and adds reach half of it at most


def workload(name, dev):
    """-> (plane int16 [B][ld] on the device, host lengths): a harmonic signal with a wandering pitch under seeded noise."""
    rng = np.random.default_rng(5)
    frames = [1031] if name == "b1" else [94] if name == "check" else [int(v) for v in rng.integers(900, 1100, size=32)]
    lens = [f * HOP for f in frames]
    plane = np.zeros((len(lens), max(lens)), np.int16)
    for i, n in enumerate(lens):
        t = np.arange(n) / SR
        phase = 2 * np.pi * np.cumsum(110.0 + 30.0 * np.sin(2 * np.pi * 0.8 * t + i)) / SR
        v = 7000 * np.sin(phase) + 3000 * np.sin(3 * phase + 1.0) + 1200 * rng.standard_normal(n)
        plane[i, :n] = np.clip(v, -32768, 32767).astype(np.int16)
    return torch.from_numpy(plane).to(dev), lens


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
    ap.add_argument("--workloads", default="b1,b32")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "formant_bench times the GPU path; there is nothing to measure without a HIP device"
    spec = ModelSpec.tiny()                   # the kernels under the clock take their sizes as arguments; the context can be small
    eng = rt.HipSynth(spec, make_synthetic_weights(spec), acoustic_dtype="bf16", nfe_step=4)
    plan = prosody_plan(1000, PITCH, None)
    res = {"metric": "output_formants", "reps": a.reps, "sample_rate": SR, "pitch": PITCH, "pitch_ratio": [plan.p_r, plan.q_r],
           "order": FORMANT_P, "taps": FORMANT_L, "hop": FORMANT_H}
    plane, lens = workload("check", eng.device)
    plans = [[(0, lens[0])]]
    joined = eng.finish_output(plane, plans, CF, SR)[0]
    shifted = eng.finish_output(plane, plans, CF, SR, pitch=PITCH)[0]
    kept = eng.finish_output(plane, plans, CF, SR, pitch=PITCH, formants="keep")[0]
    assert np.array_equal(kept, keep_formants(joined, shifted, 1, 1)), "the device result differs from the host mirror"
    res["checked_against_mirror_s"] = round(lens[0] / SR, 2)
    for name in a.workloads.split(","):
        plane, lens = workload(name, eng.device)
        ld = plane.shape[1]
        plans = [[(i * ld, n)] for i, n in enumerate(lens)]
        paths = {"plain": lambda: eng.finish_output(plane, plans, CF, SR),
                 "shift": lambda: eng.finish_output(plane, plans, CF, SR, pitch=PITCH),
                 "keep": lambda: eng.finish_output(plane, plans, CF, SR, pitch=PITCH, formants="keep")}
        ts = {k: [] for k in paths}
        for i in range(a.reps + 2):
            for k, fn in paths.items():        # alternated: the paths see the same box at the same time
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                fn()
                if i >= 2:
                    ts[k].append((time.perf_counter() - t0) * 1e3)
        buf, offs, ns = eng.join_chunks(plane.reshape(-1), plans, CF, SR)
        new, new_offs, new_lens = eng._prosody(buf, offs, ns, [PITCH] * len(ns), [None] * len(ns))
        rows = [[o, n, no, nn, no, 1, 1] for o, n, no, nn in zip(offs, ns, new_offs, new_lens)]
        out = torch.empty_like(new)
        frames = [-(-n // FORMANT_H) + 1 for n in new_lens]
        call_ms = events_ms(lambda: eng.pcm_formant(buf, new, rows, out=out), a.reps)
        flop = 4.0 * FORMANT_L * sum(new_lens)
        med = {k: float(np.median(v)) for k, v in ts.items()}
        res[name] = {
            "requests": len(lens), "audio_s": round(sum(ns) / SR, 1), "frames_total": int(sum(frames)),
            "plain_ms": round(med["plain"], 3), "shift_ms": round(med["shift"], 3), "keep_ms": round(med["keep"], 3),
            "keep_added_ms": round(med["keep"] - med["shift"], 3),
            "formant_call_ms": round(call_ms, 4),
            "tap_sum_gflop": round(flop / 1e9, 2),
            "tap_sum_tflops_over_whole_call": round(flop / (call_ms * 1e-3) / 1e12, 2),
            "share_of_unfused_fp64_roof_over_whole_call": round(flop / (call_ms * 1e-3) / (FP64_VECTOR_PEAK / 2), 3),
            "workspace_mb": round(int(eng.lib.vv_pcm_formant_ws_bytes(sum(frames), len(lens))) / 2 ** 20, 1),
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
