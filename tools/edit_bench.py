#!/usr/bin/env python3
"""Speech editing at full size, bf16: a 10 s source with one 1.0 s span regenerated as 1.5 s (10.5 s spliced,
985 frames), B = 1 and B = 8 edits per HipSynth.edit_batch call, next to HipSynth.synthesize_batch at the same frame count
(a 3 s reference clip + 703 generated frames).  Host clock around calls that end in a device synchronise; median of --reps.

    python tools/edit_bench.py [--reps 5] [--out profiles/speech_edit/edit_bench.json]
    rocprofv3 --kernel-trace --stats -d <dir> -- python tools/edit_bench.py --reps 1     (the share of the edit kernels)

Seeded synthetic weights and inputs; prints one JSON line."""
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
from vietvoice_tts_amd.pack import MAX_POS  # noqa: E402
from vietvoice_tts_amd.runtime import HipSynth  # noqa: E402
from vietvoice_tts_amd.speech_edit import plan_edit  # noqa: E402

SEED, SRC_S, SPAN, NEW_S, REF_S, TOK = 9527, 10.0, (4.0, 5.0), 1.5, 3.0, 160


def timed(fn, reps):
    fn()                                   # warm-up: every shape of the timed calls
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ts.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(ts)), ts


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--nfe", type=int, default=32)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "edit_bench times the GPU path; there is nothing to measure without a HIP device"
    spec = ModelSpec.full()
    eng = HipSynth(spec, make_synthetic_weights(spec, SEED), acoustic_dtype="bf16", nfe_step=a.nfe)
    sr, hop, dev = spec.sample_rate, spec.hop_length, eng.device
    g = torch.Generator().manual_seed(SEED)
    S = int(SRC_S * sr)
    plan = plan_edit(S, [SPAN], [NEW_S], sr, hop, spec.n_fft, MAX_POS)
    N = plan.n_frames
    res = {"metric": "speech_edit_ms", "spec": "full", "dtype": "bf16", "n_steps": eng.n_steps, "source_s": SRC_S, "span_s": list(SPAN),
           "new_span_s": NEW_S, "spliced_samples": plan.spliced_len, "frames": N, "reps": a.reps}
    for B in (1, 8):
        src = (torch.randn(B * S, generator=g) * 3000).to(torch.int16).to(dev)
        rows = [r for b in range(B) for r in plan.rows(b, b * S)]
        ids = torch.randint(0, spec.vocab_size, (B, TOK), generator=g, dtype=torch.int32).to(dev)
        tl = torch.full((B,), TOK, dtype=torch.int32, device=dev)
        keep = torch.from_numpy(np.tile(plan.keep, (B, 1))).to(dev)
        noise = torch.randn((B, N, spec.n_mel), generator=g).to(dev)
        edit_ms, edit_all = timed(lambda: eng.edit_batch(src, rows, [plan.spliced_len] * B, ids, tl, keep, noise), a.reps)
        # synthesis of the same frame count: reference clip + generated frames = N, every generated frame vocoded
        R = int(REF_S * sr)
        gen = N - (R // hop + 1)
        audio = (torch.randn((B, R), generator=g) * 3000).to(torch.int16).to(dev)
        i32 = lambda v: torch.full((B,), v, dtype=torch.int32, device=dev)
        syn_ms, syn_all = timed(lambda: eng.synthesize_batch(audio, i32(R), ids, tl, i32(N), N, noise, gen, seq_len_host=[N] * B,
                                                             audio_len_host=[R] * B), a.reps)
        res[f"b{B}"] = {"edit_ms": round(edit_ms, 2), "synth_ms": round(syn_ms, 2), "edit_over_synth": round(edit_ms / syn_ms, 4),
                        "synth_generated_frames": gen, "edit_ms_all": [round(t, 2) for t in edit_all],
                        "synth_ms_all": [round(t, 2) for t in syn_all]}
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")
    eng.close()


if __name__ == "__main__":
    main()
