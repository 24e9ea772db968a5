#!/usr/bin/env python3
"""The ODE solvers at full size, bf16: HipSynth.transformer_steps of the headline shape (B = 32, 256 tokens, N = 1600
frames per item) and of B = 1, for every built-in method on a 32-point grid, for midpoint / rk4 on 17 and 9 points and (N20) for the
multistep methods ab2 on 32 and 17 points and ab3 on 17.  ``method:nfe:report`` times a multistep method with its step report on.  Per configuration:
ms per batch, DiT evaluations, and ms per evaluation NEXT TO Euler's ms per evaluation from the same run.  Host clock around calls
that end in a device synchronise; one warm-up call, then median (and min / max) of --reps.

    python tools/ode_bench.py [--reps 3] [--out profiles/ode/ode_bench.json]
    rocprofv3 --kernel-trace --stats -d <dir> -o ode -- python3 tools/ode_bench.py --reps 1 --batches 32 --configs euler:32,midpoint:17,rk4:9
    python3 tools/rocpd_kernel_stats.py <dir>/.../ode_results.db ode_kernel_stats.csv                  (the stage kernel's share)

Seeded synthetic weights and inputs: this measures COST only.  What a solver of higher order buys in integration error cannot be
shown on synthetic weights (their velocity field is too rough to show a solver's order).  Prints one JSON line."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402

from vietvoice_tts_amd.model_spec import ODE_METHODS, ODE_MULTISTEP, ModelSpec, make_synthetic_weights  # noqa: E402
from vietvoice_tts_amd.runtime import HipSynth  # noqa: E402

SEED, REF_S, TOK, FRAMES = 9527, 6.0, 256, 1600            # the headline unit of bench.py: 6 s reference clip, 256 tokens, N = 1600 frames
# Euler on the 32-point grid comes first (the figure every row stands next to) AND last: the two bracket what the run itself drifts by
CONFIGS = [(m, 32) for m in ("euler", "midpoint", "heun2", "heun3", "rk4")] + [("midpoint", 17), ("rk4", 17), ("midpoint", 9), ("rk4", 9),
                                                                              ("ab2", 32), ("ab2", 17), ("ab3", 17), ("euler", 32)]


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
    ap.add_argument("--configs", default="", help="method:nfe_step,... instead of the default list (start with euler:32)")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "ode_bench times the GPU path; there is nothing to measure without a HIP device"
    spec = ModelSpec.full()
    eng = HipSynth(spec, make_synthetic_weights(spec, SEED), acoustic_dtype="bf16", nfe_step=32)
    dev, N = eng.device, a.frames
    g = torch.Generator().manual_seed(SEED)
    R = int(REF_S * spec.sample_rate)
    # (method, nfe_step, report): a third field "report" turns the step report of a multistep method on
    configs = [(c.split(":")[0], int(c.split(":")[1]), c.split(":")[2:] == ["report"]) for c in a.configs.split(",")] if a.configs else \
        [(m, n, False) for m, n in CONFIGS]
    assert configs[0] == ("euler", 32, False), "the first configuration is the Euler figure the others stand next to"
    res = {"metric": "ode_steps_ms", "spec": "full", "dtype": "bf16", "frames": N, "tokens": TOK, "reps": a.reps}
    for B in [int(v) for v in a.batches.split(",")]:
        audio = (torch.randn((B, R), generator=g) * 3000).to(torch.int16).to(dev)
        ids = torch.randint(0, spec.vocab_size, (B, TOK), generator=g, dtype=torch.int32).to(dev)
        i32 = lambda v: torch.full((B,), v, dtype=torch.int32, device=dev)
        pre = eng.preprocess(audio, i32(R), ids, i32(TOK), i32(N), N, seq_len_host=[N] * B, audio_len_host=[R] * B)
        noise = torch.randn((B, N, spec.n_mel), generator=g).to(dev)
        x = torch.empty_like(noise)

        def run():
            x.copy_(noise)
            eng.transformer_steps(x, pre, 0, eng.n_steps)
        rows, euler_pe = [], None
        for method, nfe, report in configs:
            eng.set_ode_report(False)
            eng.set_nfe(nfe, method)
            eng.set_ode_report(report)
            ts = timed(run, a.reps)
            med = float(np.median(ts))
            row = {"method": method, "nfe_step": nfe, "stages": 1 if method in ODE_MULTISTEP else len(ODE_METHODS[method][1]),
                   "report": report, "evaluations": eng.n_evals,
                   "ms": round(med, 2), "ms_min": round(min(ts), 2), "ms_max": round(max(ts), 2),
                   "ms_per_eval": round(med / eng.n_evals, 4), "ms_per_eval_min": round(min(ts) / eng.n_evals, 4),
                   "ms_per_eval_max": round(max(ts) / eng.n_evals, 4), "finite": bool(torch.isfinite(x).all())}
            if euler_pe is None:
                euler_pe = med / eng.n_evals                       # the list starts with Euler on the 32-point grid
            row["euler_ms_per_eval"] = round(euler_pe, 4)
            row["per_eval_over_euler"] = round(med / eng.n_evals / euler_pe, 4)
            rows.append(row)
            print(f"B={B} {method} nfe_step={nfe}{' +report' if report else ''}: {row['ms']} ms, {row['ms_per_eval']} ms per evaluation", file=sys.stderr, flush=True)
        eng.set_ode_report(False)
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
