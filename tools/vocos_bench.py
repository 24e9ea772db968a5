#!/usr/bin/env python3
"""N6 measurement: the decode stage with the HiFi-GAN generator vs the Vocos decoder at full size (1037 generated frames per item),
B = 1 and B = 32, and one bf16 synthesis batch (B = 32, 31 Euler steps) with each vocoder in audio seconds per second.

    python tools/vocos_bench.py --out vocos_bench.json
    rocprofv3 --kernel-trace --stats -d prof -o vocos -- python3 tools/vocos_bench.py --trace      (per-kernel times, a run of its own)

Decode: one warm-up call, then the median of --reps calls, each timed by a pair of HIP events on the launch stream.  Synthesis:
host clock around synthesize_batch (which ends in a device synchronise through the PCM read), median of --synth-reps after a warm-up."""
import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

from vietvoice_tts_amd.model_spec import ModelSpec, make_synthetic_weights
from vietvoice_tts_amd.runtime import HipSynth

DEV = "cuda:0"
T_GEN, REF = 1037, 563            # bench.py's headline shape: a 3 s reference clip (563 frames) + 1037 generated frames


def decode_ms(eng, B, reps):
    N = REF + T_GEN
    x = torch.randn(B, N, eng.spec.n_mel, generator=torch.Generator().manual_seed(0)).to(DEV)
    pre = {"ref_signal_len": torch.full((B,), REF, dtype=torch.int32, device=DEV), "seq_len": torch.full((B,), N, dtype=torch.int32, device=DEV)}
    eng.decode(x, pre, T_GEN)
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        pcm, n = eng.decode(x, pre, T_GEN)
        b.record()
        torch.cuda.synchronize()
        ts.append(a.elapsed_time(b))
    eng.prof_enable(True)
    eng.decode(x, pre, T_GEN)
    p = eng.prof_collect()
    eng.prof_enable(False)
    cls = {k: {"ms": round(v["ms"], 3), "launches": v["launches"]} for k, v in p.items()
           if k in ("voc_conv", "voc_post", "elementwise", "gemm") and v["launches"]}
    return {"B": B, "median_ms": round(statistics.median(ts), 3), "min_ms": round(min(ts), 3), "reps": reps, "samples_per_item": int(n[0]),
            "prof_classes": cls}


def synth(eng, B, reps):
    s = eng.spec
    g = torch.Generator().manual_seed(1)
    S = REF * s.hop_length - s.hop_length // 2          # 563 reference frames
    N = S // s.hop_length + 1 + T_GEN
    audio = (torch.randn(B, S, generator=g) * 3000).to(torch.int16).to(DEV)
    ids = torch.randint(0, s.vocab_size, (B, 120), generator=g, dtype=torch.int32).to(DEV)
    i32 = lambda v: torch.full((B,), v, dtype=torch.int32, device=DEV)
    noise = torch.randn(B, N, s.n_mel, generator=g).to(DEV)
    run = lambda: eng.synthesize_batch(audio, i32(S), ids, i32(120), i32(N), N, noise, T_GEN, seq_len_host=[N] * B, audio_len_host=[S] * B)
    _x, pcm, n, _pre = run()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        _x, pcm, n, _pre = run()
        n_host = n.cpu()
        ts.append(time.perf_counter() - t0)
    audio_s = float(n_host.sum()) / s.sample_rate
    med = statistics.median(ts)
    return {"B": B, "median_s": round(med, 4), "reps": reps, "audio_s": round(audio_s, 3), "audio_s_per_s": round(audio_s / med, 2),
            "checksum": int(pcm.int().abs().sum())}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--synth-reps", type=int, default=3)
    ap.add_argument("--out", default="")
    ap.add_argument("--trace", action="store_true", help="decode-only run for a kernel trace: both vocoders, B = 32, 3 calls each")
    a = ap.parse_args()
    assert torch.cuda.is_available()
    full = ModelSpec.full()
    w = make_synthetic_weights(full)
    w_v = make_synthetic_weights(ModelSpec.full_vocos())
    res = {"device": torch.cuda.get_device_name(0), "t_gen": T_GEN, "ref_frames": REF, "decode": {}, "synthesis_bf16": {}}
    for kind, spec, weights in (("hifigan", full, w), ("vocos", ModelSpec.full_vocos(), w_v)):
        eng = HipSynth(spec, weights, device=DEV, acoustic_dtype="bf16", nfe_step=32)
        if a.trace:
            decode_ms(eng, 32, 3)
            eng.close()
            continue
        res["decode"][kind] = [decode_ms(eng, B, a.reps) for B in (1, 32)]
        res["synthesis_bf16"][kind] = synth(eng, 32, a.synth_reps)
        print(kind, json.dumps(res["decode"][kind]), json.dumps(res["synthesis_bf16"][kind]), flush=True)
        eng.close()
        torch.cuda.empty_cache()
    if a.trace:
        return
    res["decode_speedup_vocos_over_hifigan"] = {str(d["B"]): round(h["median_ms"] / d["median_ms"], 2)
                                                for h, d in zip(res["decode"]["hifigan"], res["decode"]["vocos"])}
    print(json.dumps(res))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
