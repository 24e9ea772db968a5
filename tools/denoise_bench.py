#!/usr/bin/env python3
"""The vocoder-bias denoiser in the output stage: what `denoise=` costs between the end of vv_decode (int16 chunks in HBM)
and the final bytes on the host.

  plain     HipSynth.finish_output at 24 kHz pcm16 (join, one copy)
  denoise   the same call with denoise=1.0 against a given bias profile: join -> vv_pcm_denoise -> one copy

on two workloads at full size: B = 1 and B = 32 one-chunk requests of the headline length (~11 s).  The paths are alternated inside every
repetition, each timed by a host clock around work that ends with the bytes on the host.  vv_pcm_denoise alone (the wrapper call on the
joined buffer, descriptor upload and workspace allocation included) is timed with device events, and so is vv_pcm_formant on the same
buffers in the same run, as the yardstick among the stage's float64 links.  Medians of --reps (default 3) after a warm-up.  The butterfly
operations are counted from the shapes: per hop four frames, two transforms each, ten stages of 512 butterflies of ten operations.
Before timing, the device result on a 1 s request is checked against the mirror (equal, bit for bit).

    python tools/denoise_bench.py [--reps 3] [--workloads b1,b32] [--out profiles/denoise/denoise_bench.json]
    rocprofv3 --kernel-trace --stats -d <dir> -o denoise -- python tools/denoise_bench.py --workloads b32      (the kernels' own times)

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

from tools.formant_bench import events_ms, workload  # noqa: E402
from vietvoice_tts_amd import runtime as rt  # noqa: E402
from vietvoice_tts_amd.core.audio_processor import DENOISE_BINS, DENOISE_H, DENOISE_N, denoise_bias, denoise_pcm  # noqa: E402
from vietvoice_tts_amd.model_spec import ModelSpec, make_synthetic_weights  # noqa: E402

SR, CF, STRENGTH, PITCH = 24000, 0.1, 1.0, 4
FLOP_PER_HOP = 4 * 2 * 10 * 512 * 10.0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default="")
    ap.add_argument("--workloads", default="b1,b32")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "denoise_bench times the GPU path; there is nothing to measure without a HIP device"
    spec = ModelSpec.tiny()                   # the kernels under the clock take their sizes as arguments; the context can be small
    eng = rt.HipSynth(spec, make_synthetic_weights(spec), acoustic_dtype="bf16", nfe_step=4)
    res = {"metric": "output_denoise", "reps": a.reps, "sample_rate": SR, "strength": STRENGTH, "n": DENOISE_N, "hop": DENOISE_H}
    plane, lens = workload("check", eng.device)
    plans = [[(0, lens[0])]]
    joined = eng.finish_output(plane, plans, CF, SR)[0]
    bias = denoise_bias(joined) * 0.25                                  # a profile of the size of the signal's own floor: bins clamp, others do not
    assert bias.shape == (DENOISE_BINS,)
    got = eng.finish_output(plane, plans, CF, SR, denoise=STRENGTH, denoise_bias=bias)[0]
    assert np.array_equal(got, denoise_pcm(joined, bias, STRENGTH)), "the device result differs from the host mirror"
    assert np.array_equal(eng.pcm_denoise_bias(plane.reshape(-1), [[0, lens[0]]]).cpu().numpy()[0], denoise_bias(joined))
    res["checked_against_mirror_s"] = round(lens[0] / SR, 2)
    bias_d = torch.from_numpy(bias).to(eng.device)
    for name in a.workloads.split(","):
        plane, lens = workload(name, eng.device)
        ld = plane.shape[1]
        plans = [[(i * ld, n)] for i, n in enumerate(lens)]
        paths = {"plain": lambda: eng.finish_output(plane, plans, CF, SR),
                 "denoise": lambda: eng.finish_output(plane, plans, CF, SR, denoise=STRENGTH, denoise_bias=bias_d)}
        ts = {k: [] for k in paths}
        for i in range(a.reps + 2):
            for k, fn in paths.items():        # alternated: the paths see the same box at the same time
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                fn()
                if i >= 2:
                    ts[k].append((time.perf_counter() - t0) * 1e3)
        buf, offs, ns = eng.join_chunks(plane.reshape(-1), plans, CF, SR)
        out = torch.empty_like(buf)
        rows = [[o, n, o, 0] for o, n in zip(offs, ns)]
        call_ms = events_ms(lambda: eng.pcm_denoise(buf, rows, STRENGTH, bias_d, out=out), a.reps)
        bias_ms = events_ms(lambda: eng.pcm_denoise_bias(buf, [[offs[0], min(ns[0], 88 * 256)]]), a.reps)
        new, new_offs, new_lens = eng._prosody(buf, offs, ns, [PITCH] * len(ns), [None] * len(ns))      # the yardstick: pcm_formant, same run
        frows = [[o, n, no, nn, no, 1, 1] for o, n, no, nn in zip(offs, ns, new_offs, new_lens)]
        fout = torch.empty_like(new)
        formant_ms = events_ms(lambda: eng.pcm_formant(buf, new, frows, out=fout), a.reps)
        hops = sum(-(-n // DENOISE_H) for n in ns)
        med = {k: float(np.median(v)) for k, v in ts.items()}
        res[name] = {
            "requests": len(lens), "audio_s": round(sum(ns) / SR, 1), "hops_total": int(hops),
            "plain_ms": round(med["plain"], 3), "denoise_ms": round(med["denoise"], 3), "denoise_added_ms": round(med["denoise"] - med["plain"], 3),
            "denoise_call_ms": round(call_ms, 4), "formant_call_ms": round(formant_ms, 4), "bias_call_88_frames_ms": round(bias_ms, 4),
            "butterfly_gflop": round(hops * FLOP_PER_HOP / 1e9, 2),
            "butterfly_tflops_over_whole_call": round(hops * FLOP_PER_HOP / (call_ms * 1e-3) / 1e12, 2),
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
