#!/usr/bin/env python3
"""FLAC in the output stage: what `output_encoding="flac"` costs between the final int16 PCM in HBM and the bytes on the
host, at the bench's shape: 32 requests of about 11 s at 24 kHz.

  flac      vv_pcm_flac over the 32 requests (plan, analyse, scan, pack), device events
  ulaw      vv_pcm_encode (mu-law) over the same buffer: the plain streaming baseline of the stage, device events
  copies    the two device-to-host copies FLAC needs (24 (R + 1) bytes of info, which synchronises, then exactly info[R][0] bytes)
            against the one copy of the PCM they replace, host clock around work that ends with the bytes on the host

on two inputs: a seeded speech-like signal (a harmonic series with a wandering pitch under a slow envelope, plus a little noise), and -- with
--pcm-dir -- the PCM the synthetic model made in `bench.py --dump-outputs DIR` (random weights: noise-like, so expect it to compress
badly).  Reports bytes out over bytes in, and -- with --bench-json, the line bench.py printed in the same session on the same box --
the FLAC call as a share of the timed synthesis step.  Before timing, the device bytes of two requests are checked against the mirror.
The split between the kernels comes from a kernel trace of this tool in a run of its own (profiles/flac/notes.md).

--lpc-order 8,12 adds, per order, vv_pcm_flac_lpc over the same requests: its bytes (two requests checked against the
mirror with that order) and its call time, alternated with vv_pcm_flac so that both see the same box at the same time.

    python tools/flac_bench.py [--reps 21] [--pcm-dir DIR] [--bench-json FILE] [--lpc-order 8,12] [--out profiles/flac/flac_bench.json]

Prints one JSON line.  There is nothing to measure without a HIP device."""
import argparse
import json
import os
import socket
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402

from vietvoice_tts_amd import runtime as rt  # noqa: E402
from vietvoice_tts_amd.core.audio_processor import FLAC_BLOCK, FLAC_MAX_LPC_ORDER, flac_encode_frames, flac_frame_bound  # noqa: E402
from vietvoice_tts_amd.model_spec import ModelSpec, make_synthetic_weights  # noqa: E402

SR, HOP, B = 24000, 256, 32


def speechlike(n, seed):
    """A seeded voiced-speech stand-in: a harmonic series with a wandering pitch under a slow envelope, plus a little noise."""
    rng = np.random.default_rng(seed)
    t = np.arange(n) / SR
    f0 = 120 + 30 * np.sin(2 * np.pi * 0.7 * t) + 10 * np.sin(2 * np.pi * 2.3 * t)
    phase = 2 * np.pi * np.cumsum(f0) / SR
    x = sum(np.sin(h * phase) / h for h in range(1, 12))
    env = 0.55 + 0.45 * np.sin(2 * np.pi * 1.7 * t + 1.0)
    return np.clip(np.rint(6000 * env * x + rng.normal(0, 40, n)), -32768, 32767).astype(np.int16)


def device_identity():
    """What the box says about itself: host name, device name, architecture, compute units and, where the runtime gives one, the
    device's unique id -- so that a figure can be set against the boxes other notes name."""
    props = torch.cuda.get_device_properties(0)
    ident = {"box": socket.gethostname(), "device": props.name, "arch": getattr(props, "gcnArchName", ""),
             "compute_units": props.multi_processor_count, "memory_gib": round(props.total_memory / 2 ** 30, 1)}
    uuid = getattr(props, "uuid", None)
    if uuid is not None:
        ident["uuid"] = str(uuid)
    ident["torch"], ident["hip"] = torch.__version__, str(torch.version.hip)
    return ident


def speech_input():
    rng = np.random.default_rng(5)
    return [speechlike(int(f) * HOP, 100 + i) for i, f in enumerate(rng.integers(900, 1100, size=B))]


def model_input(dirname):
    pcm, lens = np.load(os.path.join(dirname, "pcm.npy")), np.load(os.path.join(dirname, "pcm_len.npy"))
    return [pcm[i, : int(lens[i])].astype(np.int16) for i in range(pcm.shape[0])]


def events_ms(fn, reps, warmup=3):
    ts = []
    for _ in range(reps + warmup):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ts.append(a.elapsed_time(b))
    return ts[warmup:]


def host_ms(fn, reps, warmup=3):
    ts = []
    for _ in range(reps + warmup):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        ts.append((time.perf_counter() - t0) * 1e3)
    return ts[warmup:]


def stats(ts):
    return {"median_ms": round(float(np.median(ts)), 4), "min_ms": round(min(ts), 4), "max_ms": round(max(ts), 4)}


def measure(eng, signals, reps, lpc_orders=()):
    lib, dev = eng.lib, eng.device
    offs, at = [], 0
    for s in signals:
        offs.append(at)
        at += -(-s.size // 8) * 8
    plane = np.zeros(at, np.int16)
    for o, s in zip(offs, signals):
        plane[o: o + s.size] = s
    x = torch.from_numpy(plane).to(dev)
    R, n_in = len(signals), sum(s.size for s in signals)
    rows = [[o, s.size, 0, 1] for o, s in zip(offs, signals)]
    frames = sum(-(-s.size // FLAC_BLOCK) for s in signals)
    n_y = sum((s.size // FLAC_BLOCK) * flac_frame_bound(FLAC_BLOCK) + flac_frame_bound(s.size % FLAC_BLOCK) for s in signals)
    rows_h = torch.tensor(rows, dtype=torch.int64)
    rows_d = rows_h.to(dev)
    y = torch.empty((n_y,), dtype=torch.uint8, device=dev)
    info = torch.empty((R + 1, 3), dtype=torch.int64, device=dev)
    ws = torch.empty((int(lib.vv_pcm_flac_ws_bytes(frames, R)) // 8 + 1,), dtype=torch.int64, device=dev)
    stream = torch.cuda.current_stream().cuda_stream

    def flac():
        rc = lib.vv_pcm_flac(eng.ctx, x.data_ptr(), x.numel(), rows_d.data_ptr(), rows_h.data_ptr(), R, SR, y.data_ptr(), n_y, info.data_ptr(),
                             ws.data_ptr(), ws.numel() * 8, stream)
        assert rc == 0, lib.vv_last_error(eng.ctx)

    flac()
    torch.cuda.synchronize()
    hinfo = info.cpu().numpy()
    total = int(hinfo[R, 0])
    host = y[:total].cpu().numpy()
    for r in (0, R - 1):                                       # the device bytes against the mirror, before any timing
        want = flac_encode_frames(signals[r], SR)[0]
        assert np.array_equal(host[int(hinfo[r, 0]): int(hinfo[r + 1, 0])], want), "the device bytes differ from the host mirror"
    u_rows = torch.tensor([[o, s.size, o] for o, s in zip(offs, signals)], dtype=torch.int64).to(dev)
    u_y = torch.empty((x.numel() + 8,), dtype=torch.uint8, device=dev)
    max_n = max(s.size for s in signals)

    def ulaw():
        rc = lib.vv_pcm_encode(eng.ctx, x.data_ptr(), x.numel(), u_rows.data_ptr(), R, max_n, 1, u_y.data_ptr(), x.numel(), stream)
        assert rc == 0, lib.vv_last_error(eng.ctx)

    def flac_copies():
        n = int(info.cpu()[R, 0])
        return y[:n].cpu()

    t_flac, t_ulaw = [], []
    for _ in range(3):                                         # alternated: both see the same box at the same time
        t_flac += events_ms(flac, reps // 3 + 1)
        t_ulaw += events_ms(ulaw, reps // 3 + 1)
    t_two, t_one = [], []
    for _ in range(3):
        t_two += host_ms(flac_copies, reps // 3 + 1)
        t_one += host_ms(lambda: x.cpu(), reps // 3 + 1)
    res = {"requests": R, "audio_s": round(n_in / SR, 1), "frames": frames, "bytes_in": 2 * n_in, "bytes_out": total,
           "ratio_out_over_in": round(total / (2 * n_in), 4), "flac_call": stats(t_flac), "ulaw_call": stats(t_ulaw),
           "flac_two_copies": stats(t_two), "pcm_one_copy": stats(t_one),
           "flac_gb_per_s_of_pcm": round(2 * n_in / (np.median(t_flac) * 1e-3) / 1e9, 2)}
    if lpc_orders:                                             # N16: vv_pcm_flac_lpc per order, alternated with vv_pcm_flac
        ws_l = torch.empty((int(lib.vv_pcm_flac_lpc_ws_bytes(frames, R, max(lpc_orders))) // 8 + 1,), dtype=torch.int64, device=dev)

        def lpc(order):
            rc = lib.vv_pcm_flac_lpc(eng.ctx, x.data_ptr(), x.numel(), rows_d.data_ptr(), rows_h.data_ptr(), R, SR, order, y.data_ptr(), n_y,
                                     info.data_ptr(), ws_l.data_ptr(), ws_l.numel() * 8, stream)
            assert rc == 0, lib.vv_last_error(eng.ctx)

        sizes = {}
        for order in lpc_orders:
            lpc(order)
            torch.cuda.synchronize()
            hinfo = info.cpu().numpy()
            sizes[order] = int(hinfo[R, 0])
            host = y[: sizes[order]].cpu().numpy()
            for r in (0, R - 1):
                want = flac_encode_frames(signals[r], SR, lpc_order=order)[0]
                assert np.array_equal(host[int(hinfo[r, 0]): int(hinfo[r + 1, 0])], want), "the device bytes differ from the host mirror"
        t_plain, t_lpc = [], {order: [] for order in lpc_orders}
        for _ in range(3):
            t_plain += events_ms(flac, reps // 3 + 1)
            for order in lpc_orders:
                t_lpc[order] += events_ms(lambda: lpc(order), reps // 3 + 1)
        res["flac_call_beside_lpc"] = stats(t_plain)
        res["lpc"] = {str(order): {"bytes_out": sizes[order], "ratio_out_over_in": round(sizes[order] / (2 * n_in), 4),
                                   "bytes_over_fixed_only": round(sizes[order] / total, 4), "call": stats(t_lpc[order]),
                                   "call_over_flac_call": round(float(np.median(t_lpc[order]) / np.median(t_plain)), 2)} for order in lpc_orders}
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=21)
    ap.add_argument("--pcm-dir", default="", help="bench.py --dump-outputs DIR of the same session: the synthetic model's PCM")
    ap.add_argument("--bench-json", default="", help="a file with the JSON line bench.py printed in the same session on the same box")
    ap.add_argument("--lpc-order", default="", help="comma-separated LPC orders (1 ... 12) to measure vv_pcm_flac_lpc at, e.g. 8,12")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "flac_bench times the GPU path; there is nothing to measure without a HIP device"
    spec = ModelSpec.tiny()                   # the kernels under the clock take their sizes as arguments; the context can be small
    eng = rt.HipSynth(spec, make_synthetic_weights(spec), acoustic_dtype="bf16", nfe_step=4)
    res = {"metric": "output_flac", "reps": a.reps, "sample_rate": SR, **device_identity()}
    orders = tuple(int(v) for v in a.lpc_order.split(",") if v)
    assert all(1 <= p <= FLAC_MAX_LPC_ORDER for p in orders), f"--lpc-order: orders in 1 ... {FLAC_MAX_LPC_ORDER}"
    res["speechlike"] = measure(eng, speech_input(), a.reps, orders)
    if a.pcm_dir:
        res["synthetic_model_pcm"] = measure(eng, model_input(a.pcm_dir), a.reps, orders)
    if a.bench_json:
        with open(a.bench_json) as f:
            line = [ln for ln in f.read().splitlines() if ln.startswith("{")][-1]
        step = json.loads(line)
        res["bench_step_median_ms"] = step["median_ms_per_step"]
        for key in ("speechlike", "synthetic_model_pcm"):
            if key in res:
                res[key]["flac_share_of_step"] = round(res[key]["flac_call"]["median_ms"] / step["median_ms_per_step"], 5)
    eng.close()
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
