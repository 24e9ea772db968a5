#!/usr/bin/env python3
"""The guidance interval at full size, bf16, Euler on the 32-point grid: HipSynth.transformer_steps of the headline
shape (B = 32, 256 tokens, N = 1600 frames per item) and of B = 1 under four configurations -- (a) unmasked, the path without a
mask; (b) an all-ones mask (the same rows through the masked path); (c) an all-zero mask (no unconditional row anywhere); (d) the
interval (0.25, 0.75); and guidance reuse -- (e) reuse k = 2, 3, 4 over the whole grid, the unconditional branch at every
k-th evaluation; (f) k = 2 inside the interval (0.25, 0.75); and CFG-Zero* / guidance rescale / zero-init
 -- (g) the optimised scale, the rescale at phi = 0.7 and both for every item (two small launches per evaluation in front of
the combine: the row also gives the time over the all-ones mask of the same run, the plain guided call, and the bytes the two launches
read per evaluation, 2 Rc n_mel 4); (h) cfg_zero_init = 1 and 2 (the plan without its first K steps: the row also gives the expected
(n - 1 - K) / (n - 1) and the deviation from it), closed by one more unmasked run.  (a) is run first AND last: the two bracket what the run itself drifts by.  Per configuration: ms per batch,
ms per evaluation, the rows launched over the unmasked rows, and the time over the first (a).  Host clock around calls that end in
a device synchronise; one warm-up call, then median (and min / max) of --reps.

    python tools/guidance_bench.py [--reps 3] [--out profiles/guidance/guidance_bench.json]
    rocprofv3 --kernel-trace --stats -d <dir> -o guidance -- python3 tools/guidance_bench.py --reps 1 --batches 32 --configs unmasked,zeros
    python3 tools/rocpd_kernel_stats.py <dir>/.../guidance_results.db guidance_kernel_stats.csv

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
INTERVAL = (0.25, 0.75)
CONFIGS = ["unmasked", "ones", "zeros", "interval", "reuse2", "reuse3", "reuse4", "interval_reuse2", "unmasked",
           "zero_star", "rescale", "zero_star_rescale", "zero_init1", "zero_init2", "unmasked"]
RESCALE = 0.7
NORMS = {"zero_star": (True, None), "rescale": (False, RESCALE), "zero_star_rescale": (True, RESCALE)}      # N24: (cfg_zero_star, cfg_rescale) of every item
ZERO_INIT = {"zero_init1": 1, "zero_init2": 2}


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
    ap.add_argument("--configs", default="", help="unmasked,ones,zeros,interval,reuse2,reuse3,reuse4,interval_reuse2,zero_star,rescale,zero_star_rescale,zero_init1,zero_init2 in any order instead of the default list (start with unmasked)")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "guidance_bench times the GPU path; there is nothing to measure without a HIP device"
    spec = ModelSpec.full()
    eng = HipSynth(spec, make_synthetic_weights(spec, SEED), acoustic_dtype="bf16", nfe_step=a.nfe)
    dev, N = eng.device, a.frames
    g = torch.Generator().manual_seed(SEED)
    R = int(REF_S * spec.sample_rate)
    configs = a.configs.split(",") if a.configs else CONFIGS
    assert configs[0] == "unmasked", "the first configuration is the unmasked figure the others stand next to"
    res = {"metric": "guidance_steps_ms", "spec": "full", "dtype": "bf16", "method": "euler", "nfe_step": a.nfe, "frames": N, "tokens": TOK,
           "reps": a.reps, "interval": list(INTERVAL)}
    for B in [int(v) for v in a.batches.split(",")]:
        audio = (torch.randn((B, R), generator=g) * 3000).to(torch.int16).to(dev)
        ids = torch.randint(0, spec.vocab_size, (B, TOK), generator=g, dtype=torch.int32).to(dev)
        i32 = lambda v: torch.full((B,), v, dtype=torch.int32, device=dev)
        pre = eng.preprocess(audio, i32(R), ids, i32(TOK), i32(N), N, seq_len_host=[N] * B, audio_len_host=[R] * B)
        noise = torch.randn((B, N, spec.n_mel), generator=g).to(dev)
        x = torch.empty_like(noise)
        masks = {"unmasked": None, "ones": torch.ones((eng.n_evals, B), dtype=torch.uint8), "zeros": torch.zeros((eng.n_evals, B), dtype=torch.uint8),
                 "interval": eng.guidance_mask(INTERVAL, [None] * B), "reuse2": eng.guidance_mask(None, [None] * B, 2),
                 "reuse3": eng.guidance_mask(None, [None] * B, 3), "reuse4": eng.guidance_mask(None, [None] * B, 4),
                 "interval_reuse2": eng.guidance_mask(INTERVAL, [None] * B, 2)}
        rows, base, ones_ms = [], None, None
        full_evals = eng.n_evals
        for name in configs:
            guide = masks.get(name)
            norm = eng.cfg_norm_tensors([NORMS[name][0]] * B, [NORMS[name][1]] * B) if name in NORMS else None
            if name in ZERO_INIT:                       # N24 zero-init: the plan without its first K steps (no mask: the unmasked path)
                eng.set_nfe(a.nfe, "euler", ZERO_INIT[name])

            def run():
                x.copy_(noise)
                eng.transformer_steps(x, pre, 0, eng.n_steps, guide=guide, cfg_norm=norm)
            ts = timed(run, a.reps)
            med = float(np.median(ts))
            guided = eng.n_evals if guide is None else int((guide[:, 0] == 1).sum())      # evaluations with unconditional rows (a 2 reuses: none)
            row = {"config": name, "evaluations": eng.n_evals, "guided_evaluations": guided,
                   "rows_over_unmasked": round((eng.n_evals + guided) / (2.0 * eng.n_evals), 4),
                   "ms": round(med, 2), "ms_min": round(min(ts), 2), "ms_max": round(max(ts), 2), "ms_per_eval": round(med / eng.n_evals, 4),
                   "ms_per_eval_min": round(min(ts) / eng.n_evals, 4), "ms_per_eval_max": round(max(ts) / eng.n_evals, 4),
                   "finite": bool(torch.isfinite(x).all())}
            if base is None:
                base = med
            row["over_unmasked"] = round(med / base, 4)
            if name == "ones":
                ones_ms = med
            if name in NORMS:                           # N24: against the plain guided call of the same run; what the two launches read
                row["over_guided"] = None if ones_ms is None else round(med / ones_ms, 4)
                row["norm_read_bytes_per_eval"] = 2 * B * N * spec.n_mel * 4
                row["norm_extra_ms_per_eval"] = None if ones_ms is None else round((med - ones_ms) / eng.n_evals, 4)
            if name in ZERO_INIT:
                want = eng.n_evals / full_evals
                row["zero_init"], row["expected_over_unmasked"] = ZERO_INIT[name], round(want, 4)
                row["deviation"] = round(med / base - want, 4)
                eng.set_nfe(a.nfe, "euler")
            rows.append(row)
            print(f"B={B} {name}: {row['ms']} ms, {row['ms_per_eval']} ms per evaluation, {row['over_unmasked']} of unmasked", file=sys.stderr, flush=True)
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
