"""Generates tests/golden/output_golden.json + output_golden.npz for the device output stage.

Run in the build container only (the reference is mounted read-only and never travels to the GPU box):
    python tests/golden/make_output_golden.py

(a) join     : cases produced by RUNNING the reference's AudioProcessor.concatenate_with_crossfade_improved (loaded by file path with
               make_host_golden.load_reference()); inputs and outputs are stored, no source text.
(b) G.711    : the two 65,536-byte tables of stdlib audioop.lin2ulaw / lin2alaw at width 2 over every int16 value.
(c) polyphase: inputs only; the expected values come from scipy.signal.resample_poly in the tests.

The long cases use periodic signals (a random period of 997 samples): they compress well, and the float32 summation order still decides
their RMS values.
"""
import json
import os
import sys

import numpy as np

OUT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, OUT)
from make_host_golden import load_reference  # noqa: E402

JUNCTIONS = (1, 7, 8, 9, 127, 128, 129, 2400, 8192, 8193, 21600)


def duration_for(n, sr):
    """A cross_fade_duration with int(duration * sr) == n."""
    d = n / sr
    for _ in range(4):
        if int(d * sr) == n:
            return d
        d = np.nextafter(d, np.inf) if int(d * sr) < n else np.nextafter(d, -np.inf)
    raise AssertionError((n, sr))


def noise(rng, n, amp):
    return np.clip(rng.standard_normal(n) * amp, -32000, 32000).astype(np.int16)


def periodic(rng, n, amp):
    return np.resize(noise(rng, 997, amp), n)


def build_cases():
    rng = np.random.default_rng(20251018)
    cases = []          # (name, sr, duration, [chunks])
    for n in JUNCTIONS:
        sr = 24000 if n >= 2400 else (8000, 16000, 24000)[n % 3]
        d = duration_for(n, sr)
        lens = sorted({v for v in (1, n - 1, n, n + 1, 2 * n - 1, 2 * n, 2 * n + 1) if v > 0})
        if n <= 129:
            sets = [[2 * n + 1, 1, n - 1, n, n + 1, 2 * n - 1], [2 * n, n + 1, 1, 1, 2 * n + 1], [n, n], [1, 2 * n, n - 1, n + 1], lens[::-1][:6]]
            make = noise
        elif n == 2400:
            sets = [[2 * n + 1, n - 1, n, n + 1, 2 * n - 1, 2 * n], [1, 2 * n, 1, n + 1]]
            make = periodic
        else:
            sets = [[n + 1, 2 * n - 1], [2 * n + 1, n, 2 * n]] if n < 21600 else [[2 * n + 1, 2 * n - 1]]
            make = periodic
        for j, s in enumerate(sets):
            s = [v for v in s if v > 0]
            if len(s) < 2:
                s = [1, 1]
            cases.append((f"n{n}_set{j}", sr, d, [make(rng, v, (1500, 4000, 900)[k % 3]) for k, v in enumerate(s)]))
    d128, d2400 = duration_for(128, 16000), duration_for(2400, 24000)
    a = noise(rng, 300, 3000)
    a[17] = 32767
    cases.append(("clip_32767", 16000, d128, [noise(rng, 260, 2000), a, noise(rng, 257, 2500)]))
    b = noise(rng, 300, 3000)
    b[5] = -32768
    cases.append(("neg_32768_only", 16000, d128, [b, noise(rng, 200, 2000)]))
    cases.append(("rms_below_100", 16000, d128, [noise(rng, 300, 30), noise(rng, 300, 40), noise(rng, 129, 3000)]))
    cases.append(("gain_0.7", 16000, d128, [noise(rng, 300, 500), noise(rng, 300, 5000)]))
    cases.append(("gain_1.5", 16000, d128, [noise(rng, 300, 5000), noise(rng, 300, 500)]))
    cases.append(("gain_between", 16000, d128, [noise(rng, 300, 1000), noise(rng, 300, 1100), noise(rng, 300, 950)]))
    rise = (rng.standard_normal(7200) * np.concatenate([np.full(2400, 300.0), np.linspace(300.0, 30000.0, 4800)]))
    cases.append(("wrap", 24000, d2400, [noise(rng, 3000, 600), np.clip(rise, -32000, 32000).astype(np.int16)]))
    cases.append(("no_crossfade", 24000, 0.0, [a.copy(), noise(rng, 100, 2000), b.copy()]))
    c = noise(rng, 500, 3000)
    c[499] = 32767
    cases.append(("single_chunk_32767", 24000, d2400, [c]))
    cases.append(("shape_1_1_n", 24000, duration_for(129, 24000), [noise(rng, 400, 2000).reshape(1, 1, -1), noise(rng, 130, 2500).reshape(1, 1, -1)]))
    return cases


def main():
    import audioop
    ap = load_reference()["audio_processor"].AudioProcessor
    arrays, meta = {}, []
    for i, (name, sr, d, chunks) in enumerate(build_cases()):
        out = np.asarray(ap.concatenate_with_crossfade_improved([c.copy() for c in chunks], d, sr))
        assert out.dtype == np.int16, (name, out.dtype)
        for k, c in enumerate(chunks):
            arrays[f"j{i}_in_{k}"] = c
        arrays[f"j{i}_out"] = out
        meta.append({"name": name, "sample_rate": sr, "cross_fade_duration": float(d), "n_chunks": len(chunks), "n": int(d * sr),
                     "lens": [int(c.size) for c in chunks]})
    wrap = next(m for m in meta if m["name"] == "wrap")
    i_w = meta.index(wrap)
    tail_in, tail_out = arrays[f"j{i_w}_in_1"][-2400:].astype(np.int64), arrays[f"j{i_w}_out"][-2400:].astype(np.int64)
    wrap["sign_flips_last_2400"] = int(((tail_in * tail_out) < 0).sum())
    every = np.arange(-32768, 32768, dtype=np.int16)
    arrays["g711_ulaw"] = np.frombuffer(audioop.lin2ulaw(every.tobytes(), 2), dtype=np.uint8)
    arrays["g711_alaw"] = np.frombuffer(audioop.lin2alaw(every.tobytes(), 2), dtype=np.uint8)
    rng = np.random.default_rng(4242)
    x = np.clip(rng.standard_normal(6007) * 9000, -32768, 32767).astype(np.int16)
    x[1000:1040], x[3000:3030] = 32767, -32768            # samples at the clamp
    arrays["poly_x"] = x
    with open(os.path.join(OUT, "output_golden.json"), "w", encoding="utf-8") as f:
        json.dump({"join": meta, "g711_order": "index k = sample k - 32768", "poly": {"src": 24000, "rates": [8000, 16000, 22050, 44100, 48000]}},
                  f, indent=1)
    np.savez_compressed(os.path.join(OUT, "output_golden.npz"), **arrays)
    print("wrote", len(meta), "join cases,", len(arrays), "arrays,", os.path.getsize(os.path.join(OUT, "output_golden.npz")), "bytes; wrap flips",
          wrap["sign_flips_last_2400"])


if __name__ == "__main__":
    main()
