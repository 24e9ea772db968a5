#!/usr/bin/env python3
"""Block caching at full size, bf16, Euler on the 32-point grid: HipSynth.transformer_steps of the headline shape
(B = 32, 256 tokens, N = 1600 frames per item) and of B = 1 -- (a) off, the path without the option; (b) a few spans and periods
(first, last, every).  (a) is run first AND last: the distance between the two bounds what a ratio of this run can mean.  Per
configuration: ms per batch and per evaluation, the blocks run over the blocks of the uncached run, the time over the first (a), and the
bytes of the stored planes (the cached workspace figure less the plain one).  Device events around each call on the caller's stream (the
side stream is joined to it inside the call); one warm-up call, then median (and min / max) of --reps.

    python tools/block_cache_bench.py [--reps 3] [--out profiles/block_cache/block_cache_bench.json] [--notes profiles/block_cache/notes.md]

--notes: the table is written between the `<!-- bench -->` marks of that file (the file is created when it does not exist; the text
around the marks is kept).  Seeded synthetic weights and inputs: this measures COST only.  Prints one JSON line."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402

from vietvoice_tts_amd.model_spec import ModelSpec, block_cache_schedule, make_synthetic_weights  # noqa: E402
from vietvoice_tts_amd.runtime import HipSynth, _host_lens  # noqa: E402

SEED, REF_S, TOK, FRAMES = 9527, 6.0, 256, 1600            # the headline unit of bench.py: 6 s reference clip, 256 tokens, N = 1600 frames
CONFIGS = ["off", "4,20,2", "4,20,3", "2,22,2", "off"]
MARK = "<!-- bench -->"


def timed(fn, reps):
    fn()                                   # warm-up: every shape of the timed calls
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        ts.append(a.elapsed_time(b))
    return ts


def table(res):
    out = [f"Measured by `tools/block_cache_bench.py --reps {res['reps']}`: {res['spec']} size, {res['dtype']}, {res['method']} on {res['nfe_step']} points "
           f"({res['evaluations']} evaluations), {res['frames']} frames per item, device events, median of {res['reps']}.", ""]
    for key in [k for k in res if k.startswith("b") and k[1:].isdigit()]:
        rows = res[key]
        offs = [r["ms_per_eval"] for r in rows if r["config"] == "off"]
        spread = (max(offs) - min(offs)) / offs[0] if len(offs) > 1 else float("nan")
        out += [f"B = {key[1:]} (the two uncached runs lie {spread:.4f} of the first apart):", "",
                "| block_cache | ms per batch (min ... max) | ms per evaluation | time / first off | blocks run / all | plane bytes | faster than the slower off by more than that distance |",
                "|---|---|---|---|---|---|---|"]
        for r in rows:
            verdict = "" if r["config"] == "off" else ("yes" if r["ms_per_eval"] < max(offs) - (max(offs) - min(offs)) else "NO")
            out.append(f"| {r['config']} | {r['ms']} ({r['ms_min']} ... {r['ms_max']}) | {r['ms_per_eval']} | {r['over_off']} | {r['blocks_over_all']} | "
                       f"{r['plane_bytes']} | {verdict} |")
        out.append("")
    return "\n".join(out)


def write_notes(path, text):
    body = f"{MARK}\n{text}\n{MARK}\n"
    if os.path.exists(path):
        old = open(path).read()
        if old.count(MARK) == 2:
            head, _, tail = old.split(MARK)
            body = head + body.rstrip("\n") + tail
        else:
            body = old.rstrip("\n") + "\n\n" + body
    else:
        body = "# Block caching (N23)\n\n" + body
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    with open(path, "w") as f:
        f.write(body)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--batches", default="32,1")
    ap.add_argument("--frames", type=int, default=FRAMES)
    ap.add_argument("--nfe", type=int, default=32)
    ap.add_argument("--configs", default="", help="off or first,last,every, separated by ';', instead of the default list (start with off)")
    ap.add_argument("--out", default="")
    ap.add_argument("--notes", default="")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "block_cache_bench times the GPU path; there is nothing to measure without a HIP device"
    spec = ModelSpec.full()
    eng = HipSynth(spec, make_synthetic_weights(spec, SEED), acoustic_dtype="bf16", nfe_step=a.nfe)
    dev, N = eng.device, a.frames
    g = torch.Generator().manual_seed(SEED)
    R = int(REF_S * spec.sample_rate)
    configs = a.configs.split(";") if a.configs else CONFIGS
    assert configs[0] == "off", "the first configuration is the uncached figure the others stand next to"
    res = {"metric": "block_cache_steps_ms", "spec": "full", "dtype": "bf16", "method": "euler", "nfe_step": a.nfe, "evaluations": eng.n_evals,
           "frames": N, "tokens": TOK, "reps": a.reps, "depth": spec.depth}
    for B in [int(v) for v in a.batches.split(",")]:
        audio = (torch.randn((B, R), generator=g) * 3000).to(torch.int16).to(dev)
        ids = torch.randint(0, spec.vocab_size, (B, TOK), generator=g, dtype=torch.int32).to(dev)
        i32 = lambda v: torch.full((B,), v, dtype=torch.int32, device=dev)
        pre = eng.preprocess(audio, i32(R), ids, i32(TOK), i32(N), N, seq_len_host=[N] * B, audio_len_host=[R] * B)
        noise = torch.randn((B, N, spec.n_mel), generator=g).to(dev)
        x = torch.empty_like(noise)
        planes = eng.cached_ws_bytes(B, N, [N] * B) - eng._steps_ws_bytes(eng.lib.vv_transformer_ws_bytes, B, N, _host_lens(B, [N] * B))
        rows, base = [], None
        for name in configs:
            bc = None if name == "off" else tuple(int(v) for v in name.split(","))

            def run():
                x.copy_(noise)
                eng.transformer_steps(x, pre, 0, eng.n_steps, block_cache=bc)
            ts = timed(run, a.reps)
            med = float(np.median(ts))
            modes = [0] * eng.n_evals if bc is None else block_cache_schedule(eng.plan, bc[2]).tolist()
            blocks = sum(spec.depth - (bc[1] - bc[0]) if m == 2 else spec.depth for m in modes)
            row = {"config": name, "evaluations": eng.n_evals, "light_evaluations": modes.count(2), "store_evaluations": modes.count(1),
                   "blocks_run": blocks, "blocks_over_all": round(blocks / (spec.depth * eng.n_evals), 4), "plane_bytes": 0 if bc is None else planes,
                   "ms": round(med, 2), "ms_min": round(min(ts), 2), "ms_max": round(max(ts), 2), "ms_per_eval": round(med / eng.n_evals, 4),
                   "ms_per_eval_min": round(min(ts) / eng.n_evals, 4), "ms_per_eval_max": round(max(ts) / eng.n_evals, 4),
                   "finite": bool(torch.isfinite(x).all())}
            if base is None:
                base = med
            row["over_off"] = round(med / base, 4)
            rows.append(row)
            print(f"B={B} {name}: {row['ms']} ms, {row['ms_per_eval']} ms per evaluation, {row['over_off']} of off, blocks {row['blocks_over_all']}",
                  file=sys.stderr, flush=True)
        res[f"b{B}"] = rows
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")
    if a.notes:
        write_notes(a.notes, table(res))
    eng.close()


if __name__ == "__main__":
    main()
