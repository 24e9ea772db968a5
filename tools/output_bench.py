#!/usr/bin/env python3
"""The output stage, host path against device stage: the time from the end of vv_decode (int16 chunks in HBM) to the
final bytes on the host, and the bytes that cross PCIe, for

  host      the default path: one device-to-host copy of the vocoder plane (and of pcm_len) per chunk group, then
            AudioProcessor.concatenate_with_crossfade_improved per request in numpy
  device    HipSynth.finish_output at 24 kHz pcm16: vv_join_chunks in HBM, one copy of the joined samples
  device8u  HipSynth.finish_output at 8 kHz mu-law: join -> vv_pcm_resample -> vv_pcm_encode, one copy of the G.711 bytes

on two workloads: a long-form text of 25 chunks (one request, one chunk group) and a front-end batch of 32 one-chunk requests.
The planes are seeded noise of speech-like level in the vocoder's layout ([B][ld] int16, every chunk ~ 10 s); the three paths are
alternated inside every repetition and each timing is a host clock around work that ends with the bytes on the host; medians of --reps
windows.  Before timing, the device stage's samples are checked against the host path's (equal, bit for bit).

    python tools/output_bench.py [--reps 21] [--out profiles/output/output_bench.json]

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
from vietvoice_tts_amd.core import AudioProcessor  # noqa: E402
from vietvoice_tts_amd.model_spec import ModelSpec, make_synthetic_weights  # noqa: E402

SR, CF, HOP = 24000, 0.1, 256


def workload(name, dev):
    """-> (plane int16 [B][ld] on the device, pcm_len int32 [B] on the device, host lengths, requests as lists of rows)."""
    rng = np.random.default_rng(5)
    if name == "longform25":
        frames = rng.integers(850, 1000, size=25)
        reqs = [list(range(25))]
    else:
        frames = rng.integers(700, 1000, size=32)
        reqs = [[i] for i in range(32)]
    lens = [int(f) * HOP for f in frames]
    ld = max(lens)
    plane = np.zeros((len(lens), ld), np.int16)
    for i, n in enumerate(lens):
        plane[i, :n] = np.clip(rng.standard_normal(n) * 3000, -32768, 32767).astype(np.int16)
    return torch.from_numpy(plane).to(dev), torch.tensor(lens, dtype=torch.int32, device=dev), lens, reqs


def host_path(plane, pcm_len, reqs):
    pcm, n = plane.cpu().numpy(), pcm_len.cpu().numpy()
    waves = [pcm[i, : n[i]].reshape(1, 1, -1) for i in range(pcm.shape[0])]
    return [AudioProcessor.concatenate_with_crossfade_improved([waves[i] for i in r], CF, SR) for r in reqs]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=21)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "output_bench times the GPU path; there is nothing to measure without a HIP device"
    spec = ModelSpec.tiny()                   # the kernels under the clock take their sizes as arguments; the context can be small
    eng = rt.HipSynth(spec, make_synthetic_weights(spec), acoustic_dtype="bf16", nfe_step=4)
    res = {"metric": "output_stage", "reps": a.reps, "sample_rate": SR, "cross_fade_duration": CF}
    for name in ("longform25", "batch32"):
        plane, pcm_len, lens, reqs = workload(name, eng.device)
        ld = plane.shape[1]
        plans = [[(i * ld, lens[i]) for i in r] for r in reqs]
        paths = {
            "host": lambda: host_path(plane, pcm_len, reqs),
            "device": lambda: eng.finish_output(plane, plans, CF, SR),
            "device8u": lambda: eng.finish_output(plane, plans, CF, SR, 8000, "ulaw"),
        }
        want, got = paths["host"](), paths["device"]()
        assert all(np.array_equal(w, g) for w, g in zip(want, got)), "the device stage differs from the host path"
        out8 = paths["device8u"]()
        ts = {k: [] for k in paths}
        for i in range(a.reps + 2):
            for k, fn in paths.items():        # alternated: the three see the same box at the same time
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                fn()
                if i >= 2:
                    ts[k].append((time.perf_counter() - t0) * 1e3)
        res[name] = {
            "chunks": len(lens), "requests": len(reqs), "audio_s": round(sum(w.size for w in want) / SR, 1),
            "host_ms": round(float(np.median(ts["host"])), 3), "host_bytes": int(plane.numel() * 2 + 4 * len(lens)),
            "device_ms": round(float(np.median(ts["device"])), 3), "device_bytes": int(sum(g.nbytes for g in got)),
            "device8u_ms": round(float(np.median(ts["device8u"])), 3), "device8u_bytes": int(sum(g.nbytes for g in out8)),
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
