#!/usr/bin/env python3
"""The kernels of csrc/vv_watermark.hip (with vv_denoise_fft.h) on the CPU under sanitizers, against the host mirror.

Builds tools/watermark_host_check.cpp (the kernel source on tools/hip_host_shim.h, exact-size heap buffers) twice, with
-fsanitize=address,undefined and with -fsanitize=thread, and runs
  embed  : rows of 0, 1, 255, 256, 257, 1023, 1024 and 1025 samples (nothing, one sample, around a hop, around a frame) in one call at
           strength 0.2 with three payloads; rows of 1 and 257 samples with the destination 2, 4 and 6 bytes past a 16-byte boundary; with
           --reduced not, also the groups of test_embed_equals_the_mirror_bit_for_bit at strengths 0, 0.2 and 0.5 and the batch of
           test_a_row_in_a_batch_equals_itself_alone.  y must equal core.audio_processor.watermark_embed bit for bit, and nothing
           outside a row's span may be written.
  detect : the same edge rows, marked and unmarked, in one call; with --reduced not, also the rows (1, 1023, 5000) and (96000, 1, 5000) of
           test_detect_stats_and_cells_equal_the_mirror_exactly.  Every cell and every int64 of the statistic must equal
           watermark_cells / watermark_stats.
The plane starts with the first signal and ends with the last; y ends with the last row.  Needs no GPU.

    python tools/watermark_host_check.py [--cxx clang++] [--keep DIR] [--san asan|tsan|both] [--reduced]"""
import os
import struct
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import host_check_common as H  # noqa: E402
import numpy as np  # noqa: E402

NAME = "watermark"
EDGES = (0, 1, 255, 256, 257, 1023, 1024, 1025)
SENTINEL = -21846     # 0xAAAA: what the program fills every block with


def find_cxx():
    return H.find_cxx()


def build(cxx, work, san="asan"):
    return H.build(NAME, cxx, work, san)


def _tables(key):
    from vietvoice_tts_amd.core import audio_processor as ap
    window, tw = ap.denoise_tables()
    return np.ascontiguousarray(ap.watermark_chips(key), np.int8), window, tw


def run_embed(exe, work, sigs, payloads, strength, key, yoff=0, gap=3):
    from vietvoice_tts_amd.core import audio_processor as ap
    chips, window, tw = _tables(key)
    plane, xo = H.pack_signals(sigs, gap)
    yo, n_y = H.place_outputs([s.size for s in sigs])
    rows = [[xo[k], s.size, yo[k], ap.watermark_message(payloads[k])] for k, s in enumerate(sigs)]
    frames = [-(-s.size // 256) + 3 for s in sigs]
    fin, fout = os.path.join(work, "wm_in.bin"), os.path.join(work, "wm_out.bin")
    with open(fin, "wb") as f:
        f.write(struct.pack("<6q2d", plane.size, len(rows), n_y, sum(frames), max(max(fr - 3, 1) for fr in frames), yoff, 1.0 + strength, 1.0 - strength))
        for part in (np.array(rows, np.int64), chips, window, tw, plane):
            f.write(np.ascontiguousarray(part).tobytes())
    H.run(exe, ["embed", fin, fout])
    y = np.fromfile(fout, np.int16)
    written = np.zeros(n_y, bool)
    bad = []
    for k, x in enumerate(sigs):
        written[yo[k]: yo[k] + x.size] = True
        if not np.array_equal(y[yo[k]: yo[k] + x.size], ap.watermark_embed(x, key, payloads[k], strength)):
            bad.append(x.size)
    if y.size != n_y or not (y[~written] == SENTINEL).all():
        bad.append("a sample outside a row's span was written")
    return bad


def run_detect(exe, work, sigs, key, gap=5):
    from vietvoice_tts_amd.core import audio_processor as ap
    chips, window, tw = _tables(key)
    plane, xo = H.pack_signals(sigs, gap)
    rows = [[xo[k], s.size, 0, 0] for k, s in enumerate(sigs)]
    frames = [-(-s.size // 256) + 3 for s in sigs]
    fin, fout = os.path.join(work, "wd_in.bin"), os.path.join(work, "wd_out.bin")
    with open(fin, "wb") as f:
        f.write(struct.pack("<4q", plane.size, len(rows), sum(frames), max(frames)))
        for part in (np.array(rows, np.int64), chips, window, tw, plane):
            f.write(np.ascontiguousarray(part).tobytes())
    H.run(exe, ["detect", fin, fout])
    R = len(rows)
    stats = np.fromfile(fout, np.int64, count=R * 256 * 24 * 2).reshape(R, 256, 24, 2)
    cells = np.fromfile(fout, np.int32, offset=8 * stats.size).reshape(-1, 320)
    bad, at = [], 0
    for k, x in enumerate(sigs):
        if not (np.array_equal(cells[at: at + frames[k]], ap.watermark_cells(x)) and np.array_equal(stats[k], ap.watermark_stats(x, key))):
            bad.append(x.size)
        at += frames[k]
    return bad


def cases(exe, work, reduced=False):
    from tests import watermark_util as wu
    from vietvoice_tts_amd.core import audio_processor as ap
    sigs = [wu.speechlike(n, 300 + n) for n in EDGES]
    payloads = [(0x1234, 0xBEEF, 0)[k % 3] for k in range(len(sigs))]
    yield H.check(f"embed rows of {EDGES}", not run_embed(exe, work, sigs, payloads, 0.2, wu.KEY))
    for yoff in (2, 4, 6):
        two = [wu.speechlike(1, 11), wu.speechlike(257, 12)]
        yield H.check(f"embed destination + {yoff} bytes", not run_embed(exe, work, two, [1, 0xFFFF], 0.5, wu.KEY, yoff=yoff))
    marked = [ap.watermark_embed(x, wu.KEY, 0x1234, 0.2) for x in sigs]
    yield H.check(f"detect marked rows of {EDGES}", not run_detect(exe, work, marked, wu.KEY))
    yield H.check("detect unmarked rows of 1025, 0 and 1 samples", not run_detect(exe, work, [sigs[7], sigs[0], sigs[1]], wu.WRONG_KEY))
    if reduced:
        return
    sigs = [wu.speechlike(n, 300 + n) for n in wu.LENGTHS]
    for strength in (0.0, 0.2, 0.5):
        for i, group in enumerate((sigs[0:3], sigs[3:6], [sigs[6], sigs[0], sigs[4]])):
            yield H.check(f"embed group {i} of watermark_util's lengths at strength {strength}",
                          not run_embed(exe, work, group, [0x1234, 0xBEEF, 0], strength, wu.KEY))
    sigs = [wu.speechlike(n, 700 + n) for n in (1, 257, 3000, 5000)]
    yield H.check("embed four rows, gap 7", not run_embed(exe, work, sigs, [1, 0xFFFF, 0x1234, 0xBEEF], 0.2, wu.KEY, gap=7))
    for mark in (True, False):
        make = (lambda n, seed: ap.watermark_embed(wu.speechlike(n, seed), wu.KEY, 0x1234, 0.2)) if mark else wu.speechlike
        s = {n: make(n, 40 + n % 7) for n in (1, 1023, 5000, 96000)}
        for lens in ((1, 1023, 5000), (96000, 1, 5000)):
            yield H.check(f"detect {'marked' if mark else 'unmarked'} rows of {lens}", not run_detect(exe, work, [s[n] for n in lens], wu.KEY))


if __name__ == "__main__":
    H.main(NAME, cases, __doc__)
