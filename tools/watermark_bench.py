#!/usr/bin/env python3
"""The keyed audio watermark of the output stage: what embedding and detecting cost on the device, and the null pool the
detection threshold comes from.

  --null-pool   CPU only, the host mirror: the largest score over all 256 alignments on unmarked stand-in signals (speechlike, speechy and
                noise of 1, 4 and 11 s, 16 seeds each: tests/watermark_util.null_pool) and on their marked versions under a wrong key.
                WATERMARK_THRESHOLD is 1.3 x the maximum it prints.
  (default)     on a HIP device: vv_pcm_watermark and vv_pcm_watermark_detect (the wrapper calls on a joined buffer, descriptor upload
                and workspace allocation included) timed with device events on B = 1 and B = 32 requests of the headline length (~11 s),
                beside vv_pcm_denoise on the same buffers in the same run.  Medians of --reps after a warm-up.  Before timing, the device
                results on a 1 s request are checked against the mirror (PCM and statistic equal, bit for bit).

    python tools/watermark_bench.py --null-pool [--out profiles/watermark/null_pool.json]
    python tools/watermark_bench.py [--reps 5] [--workloads b1,b32] [--out profiles/watermark/watermark_bench.json]

Prints one JSON line."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402

from vietvoice_tts_amd.core.audio_processor import (DENOISE_H, WATERMARK_THRESHOLD, watermark_decide, watermark_embed,  # noqa: E402
                                                    watermark_stats)

SR, CF, KEY, PAYLOAD, STRENGTH = 24000, 0.1, 0x0123456789ABCDEF, 0x1234, 0.2


def null_pool():
    from tests.watermark_util import KEY as K0, WRONG_KEY, null_pool as pool
    res, worst = {"metric": "watermark_null_pool", "signals": 0, "hypotheses": 0}, (0.0, "")
    by_kind = {}
    for name, x in pool():
        for tag, sig, key in (("unmarked", x, K0), ("wrong_key", watermark_embed(x, K0, PAYLOAD, STRENGTH), WRONG_KEY)):
            s = watermark_decide(watermark_stats(sig, key)).score
            k = f"{name.rsplit('-', 1)[0]}-{tag}"
            by_kind[k] = max(by_kind.get(k, 0.0), s)
            worst = max(worst, (s, f"{name}-{tag}"))
            res["signals"] += 1
            res["hypotheses"] += 256
    res.update(max_score=round(worst[0], 4), max_at=worst[1], threshold_1p3x=round(1.3 * worst[0], 4), threshold_in_code=WATERMARK_THRESHOLD,
               max_by_kind={k: round(v, 4) for k, v in sorted(by_kind.items())})
    return res


def device(a):
    import torch
    from tools.formant_bench import events_ms, workload
    from vietvoice_tts_amd import runtime as rt
    from vietvoice_tts_amd.core.audio_processor import denoise_bias
    from vietvoice_tts_amd.model_spec import ModelSpec, make_synthetic_weights
    assert torch.cuda.is_available(), "watermark_bench times the GPU path; use --null-pool without a HIP device"
    spec = ModelSpec.tiny()                   # the kernels under the clock take their sizes as arguments; the context can be small
    eng = rt.HipSynth(spec, make_synthetic_weights(spec), acoustic_dtype="bf16", nfe_step=4)
    res = {"metric": "output_watermark", "reps": a.reps, "sample_rate": SR, "strength": STRENGTH}
    plane, lens = workload("check", eng.device)
    joined = eng.finish_output(plane, [[(0, lens[0])]], CF, SR)[0]
    got = eng.finish_output(plane, [[(0, lens[0])]], CF, SR, watermark=PAYLOAD, watermark_key=KEY, watermark_strength=STRENGTH)[0]
    assert np.array_equal(got, watermark_embed(joined, KEY, PAYLOAD, STRENGTH)), "the device PCM differs from the host mirror"
    stats = eng.pcm_watermark_detect(torch.from_numpy(got).to(eng.device), [[0, got.size]], KEY).cpu().numpy()
    assert np.array_equal(stats[0], watermark_stats(got, KEY)), "the device statistic differs from the host mirror"
    assert watermark_decide(stats[0]).payload == PAYLOAD
    res["checked_against_mirror_s"] = round(lens[0] / SR, 2)
    bias_d = torch.from_numpy(denoise_bias(joined) * 0.25).to(eng.device)
    for name in a.workloads.split(","):
        plane, lens = workload(name, eng.device)
        ld = plane.shape[1]
        plans = [[(i * ld, n)] for i, n in enumerate(lens)]
        buf, offs, ns = eng.join_chunks(plane.reshape(-1), plans, CF, SR)
        out = torch.empty_like(buf)
        embed_ms = events_ms(lambda: eng.pcm_watermark(buf, [[o, n, o] for o, n in zip(offs, ns)], KEY, PAYLOAD, STRENGTH, out=out), a.reps)
        detect_ms = events_ms(lambda: eng.pcm_watermark_detect(out, [[o, n] for o, n in zip(offs, ns)], KEY), a.reps)
        denoise_ms = events_ms(lambda: eng.pcm_denoise(buf, [[o, n, o, 0] for o, n in zip(offs, ns)], 1.0, bias_d, out=out), a.reps)
        res[name] = {"requests": len(lens), "audio_s": round(sum(ns) / SR, 1), "hops_total": int(sum(-(-n // DENOISE_H) for n in ns)),
                     "embed_call_ms": round(embed_ms, 4), "detect_call_ms": round(detect_ms, 4), "denoise_call_ms": round(denoise_ms, 4)}
    eng.close()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default="")
    ap.add_argument("--workloads", default="b1,b32")
    ap.add_argument("--null-pool", action="store_true")
    a = ap.parse_args()
    line = json.dumps(null_pool() if a.null_pool else device(a))
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
