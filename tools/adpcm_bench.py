#!/usr/bin/env python3
"""IMA ADPCM in the output stage and ADPCM / G.711 clips in the ingest stage: what they cost on the device, at the bench's
shape (32 requests of about 11 s at 24 kHz) and at one request.

  adpcm     vv_pcm_adpcm over the requests (89 quantiser passes per block, one more for the codes), device events
  ulaw      vv_pcm_encode (mu-law) over the same buffer: the plain streaming baseline of the stage
  flac      vv_pcm_flac over the same buffer: the stage's other compressed encoding
            -- the three alternated in rounds, so that all see the same box at the same time; the drift is the spread of the rounds' medians
  wav_clips the device encoder's own ADPCM files back through wav_clips (container parse, one upload, vv_wav_decode, 16 R bytes of status),
            and their mu-law form, against flac_clips of the FLAC files of the same PCM: host clock around work that ends with the PCM on
            the device
  quality   on the host mirror, 2 s of the stand-in (47 blocks of 1017): the SNR of the per-block search, of the carried-state encoder
            (block 0 from index 0, every next block from the index the previous one ended with) and of every block starting at index 0

Before timing, the device bytes of two requests are checked against the mirror, and a decoded clip against the mirror's samples.

    python tools/adpcm_bench.py [--reps 21] [--out profiles/adpcm/adpcm_bench.json]

Prints one JSON line.  There is nothing to measure without a HIP device."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import numpy as np  # noqa: E402
import torch  # noqa: E402

from flac_bench import device_identity, events_ms, host_ms, speech_input, speechlike, stats  # noqa: E402
from vietvoice_tts_amd import runtime as rt  # noqa: E402
from vietvoice_tts_amd.core import audio_processor as ap  # noqa: E402
from vietvoice_tts_amd.model_spec import ModelSpec, make_synthetic_weights  # noqa: E402

SR = 24000
SPB = ap.adpcm_samples_per_block(ap.adpcm_block_align(SR))
BA = ap.adpcm_block_align(SR)


def quality():
    x = speechlike(47 * SPB, 5)
    blocks, best, err = ap.adpcm_choose(x, SPB)
    body, s0, real = blocks[:, 1:], blocks[:, :1], np.full((blocks.shape[0], 1), SPB - 1)
    zero = ap._adpcm_quantise(body, s0, np.zeros((blocks.shape[0], 1), np.int64), real, False)[0][:, 0]
    carried, idx = [], 0
    for b in range(blocks.shape[0]):                           # the chain: each block from the index the one before ended with
        e, codes = ap._adpcm_quantise(body[b: b + 1], s0[b: b + 1], np.array([[idx]]), real[b: b + 1], True)
        carried.append(int(e[0, 0]))
        for c in codes[0, 0]:
            idx = min(88, max(0, idx + int(ap.ADPCM_INDEX[c])))
    p = float((x.astype(np.float64) ** 2).sum())
    snr = lambda e: round(float(10 * np.log10(p / float(np.sum(e)))), 2)  # noqa: E731
    assert all(e <= c for e, c in zip(err, carried))
    return {"blocks": int(blocks.shape[0]), "snr_db_search": snr(err), "snr_db_carried": snr(carried), "snr_db_index0": snr(zero)}


def measure(eng, signals, reps):
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
    stream = torch.cuda.current_stream().cuda_stream
    # ---- the three encoders on the same PCM
    a_rows, at = [], 0
    for o, s in zip(offs, signals):
        a_rows.append([o, s.size, at])
        at += -(-s.size // SPB) * BA
    a_h = torch.tensor(a_rows, dtype=torch.int64)
    a_d, a_y = a_h.to(dev), torch.empty((at,), dtype=torch.uint8, device=dev)

    def adpcm():
        rc = lib.vv_pcm_adpcm(eng.ctx, x.data_ptr(), x.numel(), a_d.data_ptr(), a_h.data_ptr(), R, SPB, a_y.data_ptr(), a_y.numel(), stream)
        assert rc == 0, lib.vv_last_error(eng.ctx)

    adpcm()
    host = a_y.cpu().numpy()
    for r in (0, R - 1):                                       # the device bytes against the mirror, before any timing
        want = ap.adpcm_encode_blocks(signals[r], SPB)
        assert np.array_equal(host[a_rows[r][2]: a_rows[r][2] + want.size], want), "the device bytes differ from the host mirror"
    u_rows = torch.tensor([[o, s.size, o] for o, s in zip(offs, signals)], dtype=torch.int64).to(dev)
    u_y = torch.empty((x.numel() + 8,), dtype=torch.uint8, device=dev)
    max_n = max(s.size for s in signals)

    def ulaw():
        rc = lib.vv_pcm_encode(eng.ctx, x.data_ptr(), x.numel(), u_rows.data_ptr(), R, max_n, 1, u_y.data_ptr(), x.numel(), stream)
        assert rc == 0, lib.vv_last_error(eng.ctx)

    frames = sum(-(-s.size // ap.FLAC_BLOCK) for s in signals)
    f_h = torch.tensor([[o, s.size, 0, 1] for o, s in zip(offs, signals)], dtype=torch.int64)
    f_d = f_h.to(dev)
    n_y = sum((s.size // ap.FLAC_BLOCK) * ap.flac_frame_bound(ap.FLAC_BLOCK) + ap.flac_frame_bound(s.size % ap.FLAC_BLOCK) for s in signals)
    f_y, f_info = torch.empty((n_y,), dtype=torch.uint8, device=dev), torch.empty((R + 1, 3), dtype=torch.int64, device=dev)
    f_ws = torch.empty((int(lib.vv_pcm_flac_ws_bytes(frames, R)) // 8 + 1,), dtype=torch.int64, device=dev)

    def flac():
        rc = lib.vv_pcm_flac(eng.ctx, x.data_ptr(), x.numel(), f_d.data_ptr(), f_h.data_ptr(), R, SR, f_y.data_ptr(), n_y, f_info.data_ptr(),
                             f_ws.data_ptr(), f_ws.numel() * 8, stream)
        assert rc == 0, lib.vv_last_error(eng.ctx)

    rounds = {"adpcm": [], "ulaw": [], "flac": []}
    for _ in range(3):                                         # alternated: all see the same box at the same time
        for name, fn in (("adpcm", adpcm), ("ulaw", ulaw), ("flac", flac)):
            rounds[name].append(events_ms(fn, reps // 3 + 1))
    res = {"requests": R, "audio_s": round(n_in / SR, 1), "blocks": at // BA, "bytes_in": 2 * n_in, "adpcm_bytes_out": at}
    for name, rs in rounds.items():
        res[f"{name}_call"] = stats([t for r in rs for t in r])
        meds = [float(np.median(r)) for r in rs]
        res[f"{name}_call"]["drift_of_round_medians"] = round((max(meds) - min(meds)) / float(np.median(meds)), 4)
    res["adpcm_over_flac"] = round(res["adpcm_call"]["median_ms"] / res["flac_call"]["median_ms"], 3)
    res["adpcm_over_ulaw"] = round(res["adpcm_call"]["median_ms"] / res["ulaw_call"]["median_ms"], 2)
    # ---- the decoders on the same clips
    flac()
    hinfo, fy = f_info.cpu().numpy(), f_y.cpu().numpy()
    flac_files, adpcm_files, ulaw_files = [], [], []
    for r, s in enumerate(signals):
        end = int(hinfo[r + 1, 0]) if r + 1 < R else int(hinfo[R, 0])
        flac_files.append(ap.flac_stream_header(SR, s.size, int(hinfo[r, 1]), int(hinfo[r, 2])) + fy[int(hinfo[r, 0]): end].tobytes())
        adpcm_files.append(ap.adpcm_wav(host[a_rows[r][2]: a_rows[r][2] + -(-s.size // SPB) * BA], SR, s.size).tobytes())
        ulaw_files.append(ap.AudioProcessor._g711_wav(ap.lin2ulaw(s), SR, "ulaw"))
    pcm, out = eng.wav_clips([ap.wav_container(adpcm_files[0])])
    off, n, _w, _r, _c = out[0]
    assert np.array_equal(pcm.cpu().numpy()[off: off + 2 * n].view(np.int16), ap._decode_wav(adpcm_files[0])[0][:, 0]), "the device samples differ"
    t = {"adpcm": [], "ulaw": [], "flac": []}
    for _ in range(3):
        t["adpcm"] += host_ms(lambda: eng.wav_clips([ap.wav_container(f) for f in adpcm_files]), reps // 3 + 1)
        t["ulaw"] += host_ms(lambda: eng.wav_clips([ap.wav_container(f) for f in ulaw_files]), reps // 3 + 1)
        t["flac"] += host_ms(lambda: eng.flac_clips(flac_files), reps // 3 + 1)
    res.update({"wav_clips_adpcm": stats(t["adpcm"]), "wav_clips_ulaw": stats(t["ulaw"]), "flac_clips": stats(t["flac"]),
                "file_bytes": {"adpcm": sum(map(len, adpcm_files)), "ulaw": sum(map(len, ulaw_files)), "flac": sum(map(len, flac_files))}})
    return res


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--reps", type=int, default=21)
    p.add_argument("--out", default="")
    a = p.parse_args()
    assert torch.cuda.is_available(), "adpcm_bench times the GPU path; there is nothing to measure without a HIP device"
    spec = ModelSpec.tiny()                   # the kernels under the clock take their sizes as arguments; the context can be small
    eng = rt.HipSynth(spec, make_synthetic_weights(spec), acoustic_dtype="bf16", nfe_step=4)
    res = {"metric": "output_adpcm", "reps": a.reps, "sample_rate": SR, "samples_per_block": SPB, **device_identity()}
    signals = speech_input()
    res["b32"] = measure(eng, signals, a.reps)
    res["b1"] = measure(eng, signals[:1], a.reps)
    res["quality"] = quality()
    eng.close()
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
