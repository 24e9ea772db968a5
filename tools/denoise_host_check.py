#!/usr/bin/env python3
"""The kernels of csrc/vv_denoise.hip (with vv_denoise_fft.h) on the CPU under sanitizers, against the host mirror.

Builds tools/denoise_host_check.cpp (the kernel source on tools/hip_host_shim.h, exact-size heap buffers) twice, with
-fsanitize=address,undefined and with -fsanitize=thread, and runs
  denoise : rows of 0, 1, 255, 256, 257, 1023, 1024 and 1025 samples (nothing, one sample, around a hop, around a frame) in one call at
            strength 1 with two bias rows; rows of 1 and 257 samples with the destination 2, 4 and 6 bytes past a 16-byte boundary; with
            --reduced not, also the batches of tests/test_denoise_gpu.py (the lengths of tests/denoise_util.py at strengths 0.25 and 1,
            the mixed-strength batch, strength 0 on full-scale noise and alternation).  y and every magnitude of every frame must equal
            core.audio_processor.denoise_pcm bit for bit, and nothing outside a row's span may be written.
  bias    : signals of 1024, 1280 and (--reduced not) 5000 samples, alone and two ragged rows in one call == denoise_bias bit for bit
The plane starts with the first signal and ends with the last; y ends with the last row.  Needs no GPU.

    python tools/denoise_host_check.py [--cxx clang++] [--keep DIR] [--san asan|tsan|both] [--reduced]"""
import os
import struct
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import host_check_common as H  # noqa: E402
import numpy as np  # noqa: E402

NAME = "denoise"
EDGES = (0, 1, 255, 256, 257, 1023, 1024, 1025)
SENTINEL = -21846     # 0xAAAA: what the program fills every block with


def find_cxx():
    return H.find_cxx()


def build(cxx, work, san="asan"):
    return H.build(NAME, cxx, work, san)


def run_denoise(exe, work, sigs, strengths, bias_rows, bias, yoff=0, gap=3):
    from vietvoice_tts_amd.core import audio_processor as ap
    window, tw = ap.denoise_tables()
    plane, xo = H.pack_signals(sigs, gap)
    yo, n_y = H.place_outputs([s.size for s in sigs])
    strengths = [float(s) for s in (strengths if isinstance(strengths, (list, tuple)) else [strengths] * len(sigs))]
    rows = [[xo[k], s.size, yo[k], bias_rows[k]] for k, s in enumerate(sigs)]
    frames = [-(-s.size // 256) + 3 for s in sigs]
    fin, fout = os.path.join(work, "dn_in.bin"), os.path.join(work, "dn_out.bin")
    with open(fin, "wb") as f:
        f.write(struct.pack("<7q", plane.size, len(rows), n_y, bias.shape[0], sum(frames), max(max(fr - 3, 1) for fr in frames), yoff))
        for part in (np.array(rows, np.int64), np.array(strengths, np.float64), bias, window, tw, plane):
            f.write(np.ascontiguousarray(part).tobytes())
    H.run(exe, ["denoise", fin, fout])
    y = np.fromfile(fout, np.int16, count=n_y)
    mag = np.fromfile(fout, np.float64, offset=2 * n_y).reshape(-1, 1024)
    written, bad, at = np.zeros(n_y, bool), [], 0
    for k, x in enumerate(sigs):
        want, want_mag = ap.denoise_pcm(x, bias[bias_rows[k]], strengths[k], mags=True)
        written[yo[k]: yo[k] + x.size] = True
        if not (np.array_equal(y[yo[k]: yo[k] + x.size], want) and np.array_equal(mag[at: at + frames[k]].view(np.uint64), want_mag.view(np.uint64))):
            bad.append(x.size)
        at += frames[k]
    if not (y[~written] == SENTINEL).all():
        bad.append("a sample outside a row's span was written")
    return bad


def run_bias(exe, work, plane, rows):
    from vietvoice_tts_amd.core import audio_processor as ap
    window, tw = ap.denoise_tables()
    frames = [(n - 1024) // 256 + 1 for _o, n in rows]
    fin, fout = os.path.join(work, "db_in.bin"), os.path.join(work, "db_out.bin")
    with open(fin, "wb") as f:
        f.write(struct.pack("<4q", plane.size, len(rows), sum(frames), max(frames)))
        for part in (np.array([[o, n, 0, 0] for o, n in rows], np.int64), window, tw, plane):
            f.write(np.ascontiguousarray(part).tobytes())
    H.run(exe, ["bias", fin, fout])
    got = np.fromfile(fout, np.float64).reshape(len(rows), 513)
    return [n for k, (o, n) in enumerate(rows) if not np.array_equal(got[k].view(np.uint64), ap.denoise_bias(plane[o: o + n]).view(np.uint64))]


def cases(exe, work, reduced=False):
    from tests import denoise_util as du
    bias = np.stack([du.random_bias(21), du.random_bias(22, 20000.0)])
    sigs = [du.speechlike(n, 300 + n) for n in EDGES]
    yield H.check(f"denoise rows of {EDGES}", not run_denoise(exe, work, sigs, 1.0, [k % 2 for k in range(len(sigs))], bias))
    for yoff in (2, 4, 6):
        two = [du.speechlike(1, 11), du.speechlike(257, 12)]
        yield H.check(f"denoise destination + {yoff} bytes", not run_denoise(exe, work, two, [0.5, 2.0], [1, 0], bias, yoff=yoff))
    for n in (1024, 1280) if reduced else (1024, 1280, 5000):
        x = du.speechlike(n, 500 + n)
        yield H.check(f"bias of {n} samples", not run_bias(exe, work, x, [[0, n]]))
        yield H.check(f"bias of {n} and of its first 1024 in one call", not run_bias(exe, work, x, [[0, 1024], [0, n]]))
    if reduced:
        return
    sigs = [du.speechlike(n, 300 + n) for n in du.LENGTHS]
    for s in (0.25, 1.0):
        yield H.check(f"denoise the lengths of denoise_util at strength {s}", not run_denoise(exe, work, sigs, s, [k % 2 for k in range(len(sigs))], bias))
    sigs = [du.speechlike(n, 700 + n) for n in (1, 257, 1024, 3000, 5000)]
    yield H.check("denoise mixed strengths", not run_denoise(exe, work, sigs, [0.5, 2.0, 1.0, 0.25, 16.0], [0, 1, 1, 0, 1], bias, gap=7))
    sigs = [du.noise(5000, 9), du.alternation(5000)]
    yield H.check("denoise strength 0 on full-scale signals", not run_denoise(exe, work, sigs, 0.0, [0, 1], bias))
    yield H.check("denoise an all-zero bias", not run_denoise(exe, work, sigs, 1.0, [0, 1], np.zeros_like(bias)))


if __name__ == "__main__":
    H.main(NAME, cases, __doc__)
