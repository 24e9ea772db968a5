#!/usr/bin/env python3
"""FLAC in the ingest stage: what a reference clip stored as FLAC costs against the Python mirror and against the same
clip stored as WAV.  The clips are made by the product's own encoder on the device (vv_pcm_flac: Fixed; vv_pcm_flac_lpc order 8) from a
seeded speech-like signal, 10 s at 24 kHz, mono, 16 bits.

  mirror    core.audio_processor.flac_decode of ONE clip, host clock (pure Python: seconds; measured once per encoder setting)
  device    HipSynth.flac_clips over 1 and over 32 clips: the whole call (container parsing, upload of the frame bytes, vv_flac_index, the
            readback of info, vv_flac_decode, the readback of info2), host clock around work that ends with info2 on the host; and the
            two C calls alone by device events.  The decoded PCM is checked against the encoder's input before anything is timed
  ingest    VoiceBank.ingest_many of the 32 clips as FLAC against the same 32 clips as WAV, fresh banks, alternated, host clock (the
            call ends with the entries' host copies)

The split between the kernels comes from a kernel trace of this tool in a run of its own (profiles/flac_decode/notes.md).  The capability
did not exist before, so there is no earlier figure to compare with, and nothing here asserts a threshold.

    python tools/flac_decode_bench.py [--reps 11] [--out profiles/flac_decode/flac_decode_bench.json]

Prints one JSON line.  There is nothing to measure without a HIP device."""
import argparse
import json
import os
import socket
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402

from vietvoice_tts_amd import runtime as rt  # noqa: E402
from vietvoice_tts_amd.core.audio_processor import AudioProcessor, flac_decode, flac_stream_header  # noqa: E402
from vietvoice_tts_amd.model_spec import ModelSpec, make_synthetic_weights  # noqa: E402
from vietvoice_tts_amd.voice_bank import VoiceBank  # noqa: E402

SR, SECONDS, B = 24000, 10, 32


def speechlike(n, seed):
    """A seeded voiced-speech stand-in: a harmonic series with a wandering pitch under a slow envelope, plus a little noise."""
    rng = np.random.default_rng(seed)
    t = np.arange(n) / SR
    f0 = 120 + 30 * np.sin(2 * np.pi * 0.7 * t) + 10 * np.sin(2 * np.pi * 2.3 * t) + 3 * seed
    phase = 2 * np.pi * np.cumsum(f0) / SR
    x = sum(np.sin(h * phase) / h for h in range(1, 12))
    env = 0.55 + 0.45 * np.sin(2 * np.pi * 1.7 * t + 1.0)
    return np.clip(np.rint(6000 * env * x + rng.normal(0, 40, n)), -32768, 32767).astype(np.int16)


def encode(eng, clips, lpc_order):
    """The clips as complete FLAC files, by the device encoder."""
    x = torch.from_numpy(np.concatenate(clips)).to(eng.device)
    offs = np.concatenate([[0], np.cumsum([len(c) for c in clips])])
    y, info = eng.pcm_flac(x, [[int(offs[j]), len(c), 0, 1] for j, c in enumerate(clips)], SR, lpc_order)
    info, y = info.cpu().numpy(), y.cpu().numpy()
    files = []
    for j, c in enumerate(clips):
        end = int(info[j + 1, 0]) if j + 1 < len(clips) else int(info[len(clips), 0])
        files.append(flac_stream_header(SR, len(c), int(info[j, 1]), int(info[j, 2])) + y[int(info[j, 0]): end].tobytes())
    return files


def host_ms(fn, reps):
    out = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        out.append((time.perf_counter() - t0) * 1e3)
    return {"median_ms": round(statistics.median(out), 4), "min_ms": round(min(out), 4), "max_ms": round(max(out), 4), "reps": reps}


def stages_ms(eng, files, reps):
    """vv_flac_index and vv_flac_decode alone, by device events (the buffers made ahead; the layout from one earlier readback)."""
    from vietvoice_tts_amd.core.audio_processor import flac_container
    infos = [flac_container(f) for f in files]
    parts, rows, pos = [], [], 0
    for f, fi in zip(files, infos):
        body = f[fi.start:]
        rows.append([pos, len(body), fi.channels, fi.bits, fi.min_block, fi.max_block, fi.rate, fi.total])
        parts.append(body + b"\0" * (-len(body) % 4))
        pos += len(parts[-1])
    buf = torch.frombuffer(bytearray(b"".join(parts) + b"\0" * (-pos % 8 + 8)), dtype=torch.uint8).to(eng.device)
    info, index = eng.flac_index(buf, rows)
    info = info.cpu().tolist()
    lay, at = [], 0
    for st, _b, frames, samples in info:
        assert st == 0
        lay.append([at, frames, samples])
        at += samples * 2
    pcm = torch.empty((at,), dtype=torch.uint8, device=eng.device)
    res = {}
    for name, fn in (("vv_flac_index", lambda: eng.flac_index(buf, rows)), ("vv_flac_decode", lambda: eng.flac_decode(buf, index, lay, pcm))):
        fn()
        times = []
        for _ in range(reps):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            b.record()
            b.synchronize()
            times.append(a.elapsed_time(b))
        res[name] = {"median_ms": round(statistics.median(times), 4), "min_ms": round(min(times), 4), "max_ms": round(max(times), 4), "reps": reps}
    res["frame_bytes"] = pos
    res["pcm_bytes"] = at
    return res


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--reps", type=int, default=11)
    p.add_argument("--out", default="")
    a = p.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("no HIP device: nothing to measure")
    spec = ModelSpec.tiny()
    eng = rt.HipSynth(spec, make_synthetic_weights(spec, seed=9527), acoustic_dtype="fp32", nfe_step=8)
    clips = [speechlike(SR * SECONDS, s) for s in range(B)]
    props = torch.cuda.get_device_properties(0)
    out = {"box": socket.gethostname(), "device": props.name, "arch": getattr(props, "gcnArchName", ""), "clips": B, "seconds": SECONDS, "rate": SR}
    wavs = [AudioProcessor.to_wav_bytes(c, SR) for c in clips]
    for label, order in (("fixed", 0), ("lpc8", 8)):
        files = encode(eng, clips, order)
        pcm, res = eng.flac_clips(files)
        host = pcm.cpu().numpy()
        for c, r in zip(clips, res):                                          # right before fast
            assert not isinstance(r, Exception) and np.array_equal(host[r[0]: r[0] + 2 * r[1]].view(np.int16), c)
        t0 = time.perf_counter()
        got = flac_decode(files[0])
        mirror_s = time.perf_counter() - t0
        assert np.array_equal(got[0][:, 0], clips[0])
        sec = {"flac_bytes_over_pcm_bytes": round(sum(map(len, files)) / (2.0 * sum(map(len, clips))), 4),
               "mirror_one_clip_s": round(mirror_s, 3),
               "device_one_clip": dict(whole_call=host_ms(lambda: eng.flac_clips(files[:1]), a.reps), **stages_ms(eng, files[:1], a.reps)),
               "device_32_clips": dict(whole_call=host_ms(lambda: eng.flac_clips(files), a.reps), **stages_ms(eng, files, a.reps))}
        flac_t, wav_t = [], []
        for _ in range(a.reps):                                               # alternated: both see the same box at the same time
            for items, sink in ((files, flac_t), (wavs, wav_t)):
                bank = VoiceBank(eng, SR)
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                bank.ingest_many(items)
                torch.cuda.synchronize()
                sink.append((time.perf_counter() - t0) * 1e3)
        sec["ingest_32_flac_ms"] = {"median": round(statistics.median(flac_t), 3), "min": round(min(flac_t), 3), "max": round(max(flac_t), 3)}
        sec["ingest_32_wav_ms"] = {"median": round(statistics.median(wav_t), 3), "min": round(min(wav_t), 3), "max": round(max(wav_t), 3)}
        e_f, e_w = VoiceBank(eng, SR).ingest_many(files), VoiceBank(eng, SR).ingest_many(wavs)
        assert all(np.array_equal(x.pcm_host, y.pcm_host) for x, y in zip(e_f, e_w))
        out[label] = sec
    line = json.dumps(out)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
