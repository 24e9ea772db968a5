#!/usr/bin/env python3
"""Projected guidance at full size, bf16, Euler on the 32-point grid: HipSynth.transformer_steps of the headline shape
(B = 32, 256 tokens, N = 1600 frames per item) and of B = 1 under three configurations -- (a) plain CFG, the path without projected
guidance; (b) eta = 0 without a cap; (c) eta = 0 with a cap of 0.3.  (a) is run first AND last: the two bracket what the run itself
drifts by.  Per configuration: ms per batch, ms per evaluation and the time over the first (a); and, from a profiled call of each
configuration (vv_prof_enable: one event pair per launch), the launches and the time of the "elementwise" class, whose difference to
(a)'s is the three kernels' own time (the reduction, the coefficients, and what the stage kernel costs beyond vvk_cfg_euler).  Host
clock around calls that end in a device synchronise; one warm-up call, then median (and min / max) of --reps.

    python tools/apg_bench.py [--reps 3] [--out profiles/apg/apg_bench.json]

Seeded synthetic weights and inputs: this measures COST only.  Prints one JSON line."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402

from vietvoice_tts_amd.model_spec import ModelSpec, make_synthetic_weights  # noqa: E402
from vietvoice_tts_amd.runtime import HipSynth  # noqa: E402

SEED, REF_S, TOK, FRAMES = 9527, 6.0, 256, 1600            # the headline unit of bench.py: 6 s reference clip, 256 tokens, N = 1600 frames
CAP = 0.3
CONFIGS = ["plain", "eta0", "eta0_cap", "plain"]


def timed(fn, reps):
    fn()                                   # warm-up: every shape of the timed calls
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ts.append((time.perf_counter() - t0) * 1e3)
    return ts


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--batches", default="32,1")
    ap.add_argument("--frames", type=int, default=FRAMES)
    ap.add_argument("--nfe", type=int, default=32)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "apg_bench times the GPU path; there is nothing to measure without a HIP device"
    spec = ModelSpec.full()
    eng = HipSynth(spec, make_synthetic_weights(spec, SEED), acoustic_dtype="bf16", nfe_step=a.nfe)
    dev, N = eng.device, a.frames
    g = torch.Generator().manual_seed(SEED)
    R = int(REF_S * spec.sample_rate)
    res = {"metric": "apg_steps_ms", "spec": "full", "dtype": "bf16", "method": "euler", "nfe_step": a.nfe, "frames": N, "tokens": TOK,
           "reps": a.reps, "cap": CAP}
    for B in [int(v) for v in a.batches.split(",")]:
        audio = (torch.randn((B, R), generator=g) * 3000).to(torch.int16).to(dev)
        ids = torch.randint(0, spec.vocab_size, (B, TOK), generator=g, dtype=torch.int32).to(dev)
        i32 = lambda v: torch.full((B,), v, dtype=torch.int32, device=dev)
        pre = eng.preprocess(audio, i32(R), ids, i32(TOK), i32(N), N, seq_len_host=[N] * B, audio_len_host=[R] * B)
        noise = torch.randn((B, N, spec.n_mel), generator=g).to(dev)
        x = torch.empty_like(noise)
        apgs = {"plain": None, "eta0": eng.apg_tensors([0.0] * B, [None] * B), "eta0_cap": eng.apg_tensors([0.0] * B, [CAP] * B)}
        rows, base = [], None
        for name in CONFIGS:
            apg = apgs[name]

            def run():
                x.copy_(noise)
                eng.transformer_steps(x, pre, 0, eng.n_steps, apg=apg)
            ts = timed(run, a.reps)
            med = float(np.median(ts))
            eng.prof_enable(True)          # one more call with an event pair around every launch: the class's launches and device time
            eng.prof_collect()
            run()
            torch.cuda.synchronize()
            ew = eng.prof_collect()["elementwise"]
            eng.prof_enable(False)
            row = {"config": name, "evaluations": eng.n_evals, "ms": round(med, 2), "ms_min": round(min(ts), 2), "ms_max": round(max(ts), 2),
                   "ms_per_eval": round(med / eng.n_evals, 4), "ms_per_eval_min": round(min(ts) / eng.n_evals, 4),
                   "ms_per_eval_max": round(max(ts) / eng.n_evals, 4), "elementwise_launches": int(ew["launches"]),
                   "elementwise_ms": round(ew["ms"], 3), "elementwise_ms_per_eval": round(ew["ms"] / eng.n_evals, 5),
                   "finite": bool(torch.isfinite(x).all())}
            if base is None:
                base = med
            row["over_plain"] = round(med / base, 4)
            rows.append(row)
            print(f"B={B} {name}: {row['ms']} ms, {row['ms_per_eval']} ms per evaluation, {row['over_plain']} of plain; elementwise "
                  f"{row['elementwise_launches']} launches, {row['elementwise_ms']} ms", file=sys.stderr, flush=True)
        res[f"b{B}"] = rows
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")
    eng.close()


if __name__ == "__main__":
    main()
