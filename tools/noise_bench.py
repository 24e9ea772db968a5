#!/usr/bin/env python3
"""The start noise of the flow ODE, host source against device source, at full size (N = 1600 frames, n_mel = 100):

  host    the draw as TTSEngine._synthesize_device does it: torch.randn per item from one generator, a zero-padded [B][N][n_mel] host
          tensor, one pageable H2D copy (timed as a whole and the copy alone); host clock, the copy ends in a device synchronise
  fill    vv_noise_fill alone, HIP events around windows of --launches launches, median of --reps windows, at B = 32 and B = 1;
          bytes/s = the 4 B N n_mel bytes it stores over that time, next to the LayerNorm class's rate measured in the same run
          (vv_layernorm at 102,400 x 1,024 with two bf16 deltas: the project's measured HBM yardstick)
  engine  B = 1 TTSEngine.synthesize wall time (full model, bf16, 32 grid points) under both sources, the two engines alternated

    python tools/noise_bench.py [--reps 21] [--out profiles/noise/noise_bench.json]

Seeded synthetic weights; prints one JSON line.  There is nothing to measure without a HIP device."""
import argparse
import ctypes as C
import json
import os
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402

from vietvoice_tts_amd import runtime as rt  # noqa: E402
from vietvoice_tts_amd.model_spec import ModelSpec, make_synthetic_weights, noise_keys  # noqa: E402

N, N_MEL, SEED = 1600, 100, 9527
TEXT = "Hôm nay trời đẹp quá, chúng ta cùng nhau đi dạo quanh hồ nhé."


def med(ts):
    return float(np.median(ts))


def host_draw(B, dev, reps):
    """-> (draw + pad + copy ms, copy alone ms): medians; the generator runs on, as the engine's does."""
    gen = torch.Generator().manual_seed(SEED)
    whole, copy = [], []
    for i in range(reps + 2):
        t0 = time.perf_counter()
        blocks = [torch.randn((N, N_MEL), generator=gen, dtype=torch.float32) for _ in range(B)]
        noise = torch.zeros((B, N, N_MEL), dtype=torch.float32)
        for b in range(B):
            noise[b, :N] = blocks[b]
        t1 = time.perf_counter()
        x = noise.to(dev)
        torch.cuda.synchronize()
        t2 = time.perf_counter()
        del x
        if i >= 2:                           # two warm-up rounds
            whole.append((t2 - t0) * 1e3)
            copy.append((t2 - t1) * 1e3)
    return med(whole), med(copy)


def fill_alone(eng, B, launches, reps):
    kd = eng.noise_keys_device(noise_keys(SEED, 0, B))
    seq = torch.full((B,), N, dtype=torch.int32, device=eng.device)
    out = torch.empty((B, N, N_MEL), dtype=torch.float32, device=eng.device)
    st = torch.cuda.current_stream().cuda_stream
    call = lambda: eng.lib.vv_noise_fill(eng.ctx, B, N, N_MEL, out.data_ptr(), seq.data_ptr(), kd.data_ptr(), 0, st)
    for _ in range(10):
        assert call() == 0
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(launches):
            call()
        e1.record()
        torch.cuda.synchronize()
        ts.append(e0.elapsed_time(e1) / launches)
    ms = med(ts)
    return {"us": round(ms * 1e3, 2), "bytes": 4 * B * N * N_MEL, "GBps": round(4 * B * N * N_MEL / ms / 1e6, 1),
            "us_min": round(min(ts) * 1e3, 2), "us_max": round(max(ts) * 1e3, 2)}


def layernorm_rate(eng, launches, reps):
    R, D = 102400, 1024
    dev = eng.device
    x = torch.randn(R, D, device=dev)
    d1, d2 = torch.randn(R, D, device=dev).bfloat16(), torch.randn(R, D, device=dev).bfloat16()
    y = torch.zeros(R, D, device=dev, dtype=torch.bfloat16)
    w, b = torch.randn(D, device=dev), torch.randn(D, device=dev)
    a = rt.vv_ln_args()
    a.out_dtype = rt.VV_BF16
    a.x, a.ldx, a.y, a.ldy, a.R, a.D, a.w, a.b, a.add_one, a.eps = x.data_ptr(), D, y.data_ptr(), D, R, D, w.data_ptr(), b.data_ptr(), 1, 1e-6
    a.delta, a.delta_dtype, a.ld_delta, a.delta2 = d1.data_ptr(), rt.VV_BF16, D, d2.data_ptr()
    st = torch.cuda.current_stream().cuda_stream
    for _ in range(3):
        assert eng.lib.vv_layernorm(eng.ctx, C.byref(a), st) == 0
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(launches):
            eng.lib.vv_layernorm(eng.ctx, C.byref(a), st)
        e1.record()
        torch.cuda.synchronize()
        ts.append(e0.elapsed_time(e1) / launches)
    byt = R * D * (4 + 2 + 2 + 4 + 2)        # fp32 stream read and rewritten, two bf16 deltas read, bf16 output written
    return {"us": round(med(ts) * 1e3, 1), "bytes": byt, "GBps": round(byt / med(ts) / 1e6, 1)}


def engine_b1(cache, reps):
    from vietvoice_tts_amd.core import ModelConfig, TTSEngine
    engines = {src: TTSEngine(ModelConfig(model_cache_dir=cache, synthetic_model=True, model_spec="full", acoustic_dtype="bf16", nfe_step=32,
                                          noise_source=src)) for src in ("host", "device")}
    ts = {"host": [], "device": []}
    frames = None
    for i in range(reps + 2):
        for src, e in engines.items():        # alternated: both see the same box at the same time
            t0 = time.perf_counter()
            wave, _ = e.synthesize(TEXT)
            dt = (time.perf_counter() - t0) * 1e3
            frames = list(e._last_plan)
            if i >= 2:
                ts[src].append(dt)
    for e in engines.values():
        e.cleanup()
    return {"frames": frames, "audio_s": round(wave.size / 24000.0, 2), "host_ms": round(med(ts["host"]), 2), "device_ms": round(med(ts["device"]), 2),
            "host_ms_all": [round(t, 2) for t in ts["host"]], "device_ms_all": [round(t, 2) for t in ts["device"]]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=21)
    ap.add_argument("--launches", type=int, default=50)
    ap.add_argument("--engine-reps", type=int, default=9)
    ap.add_argument("--cache", default="")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "noise_bench times the GPU path; there is nothing to measure without a HIP device"
    spec = ModelSpec.tiny()                   # the kernels under the clock take their sizes as arguments; the context can be small
    eng = rt.HipSynth(spec, make_synthetic_weights(spec), acoustic_dtype="bf16", nfe_step=4)
    res = {"metric": "start_noise", "N": N, "n_mel": N_MEL, "reps": a.reps, "launches_per_window": a.launches}
    res["layernorm_yardstick"] = layernorm_rate(eng, 20, a.reps)
    for B in (32, 1):
        whole, copy = host_draw(B, eng.device, a.reps)
        res[f"b{B}"] = {"host_draw_pad_h2d_ms": round(whole, 3), "h2d_alone_ms": round(copy, 3), "fill": fill_alone(eng, B, a.launches, a.reps)}
    eng.close()
    cache = a.cache or tempfile.mkdtemp(prefix="noise_bench_")
    res["engine_b1"] = engine_b1(cache, a.engine_reps)
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
