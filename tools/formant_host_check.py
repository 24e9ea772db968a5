#!/usr/bin/env python3
"""The kernels of csrc/vv_formant.hip on the CPU under sanitizers, against the host mirror.

Builds tools/formant_host_check.cpp (the kernel source on tools/hip_host_shim.h, exact-size heap buffers) twice, with
-fsanitize=address,undefined and with -fsanitize=thread, and runs the cases of tests/formant_util.py as rows of one call:
  edges : DEVICE_CASES up to 257 samples (0, 1, one less than, equal to and one more than a hop) and FRAME_EDGE_CASES (one less than,
          equal to and one more than an analysis frame, in x and in y), with flat frames next to live ones; rows of 1 and 257 samples
          with the destination 2, 4 and 6 bytes past a 16-byte boundary
  full  : with --reduced not, also every other case of DEVICE_CASES (700 to 5000 samples, the saturating square, constant, zeros)
z and every tap of every frame's filter must equal core.audio_processor (formant_filters, apply_formant_filters) bit for bit, and
nothing outside a row's span may be written.  x and y start with the first signal and end with the last; z ends with the last row.
Needs no GPU.

    python tools/formant_host_check.py [--cxx clang++] [--keep DIR] [--san asan|tsan|both] [--reduced]"""
import os
import struct
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import host_check_common as H  # noqa: E402
import numpy as np  # noqa: E402

NAME = "formant"
SENTINEL = -21846     # 0xAAAA: what the program fills every block with


def find_cxx():
    return H.find_cxx()


def build(cxx, work, san="asan"):
    return H.build(NAME, cxx, work, san)


def run_formant(exe, work, items, zoff=0):
    """items = tests.formant_util.device_case dicts, as the rows of one call -> the names that differ"""
    from vietvoice_tts_amd.core import audio_processor as ap
    wa, g = ap.formant_tables()
    xs, xo = H.pack_signals([c["x"] for c in items], 3)
    ys, yo = H.pack_signals([c["y"] for c in items], 5)
    zo, n_z = H.place_outputs([c["y"].size for c in items])
    rows = [[xo[k], c["x"].size, yo[k], c["y"].size, zo[k], c["tn"], c["td"]] for k, c in enumerate(items)]
    frames = [-(-c["y"].size // 256) + 1 for c in items]
    fin, fout = os.path.join(work, "fm_in.bin"), os.path.join(work, "fm_out.bin")
    with open(fin, "wb") as f:
        f.write(struct.pack("<7q", xs.size, ys.size, len(rows), n_z, sum(frames), max(frames), zoff))
        for part in (np.array(rows, np.int64), wa, g, ap.wsola_window(), xs, ys):
            f.write(np.ascontiguousarray(part).tobytes())
    H.run(exe, [fin, fout])
    z = np.fromfile(fout, np.int16, count=n_z)
    taps = np.fromfile(fout, np.float64, offset=2 * n_z).reshape(-1, 2048)
    written, bad, at = np.zeros(n_z, bool), [], 0
    for k, c in enumerate(items):
        n_f = c["y"].size
        written[zo[k]: zo[k] + n_f] = True
        h = taps[at: at + frames[k]]
        if not (h.shape == c["h"].shape and np.array_equal(h.view(np.uint64), np.ascontiguousarray(c["h"]).view(np.uint64))
                and np.array_equal(z[zo[k]: zo[k] + n_f], c["z"])):
            bad.append(c["name"])
        at += frames[k]
    if not (z[~written] == SENTINEL).all():
        bad.append("a sample outside a row's span was written")
    return bad


def cases(exe, work, reduced=False):
    from tests import formant_util as fu
    small = [fu.device_case(*c) for c in fu.DEVICE_CASES if c[2] <= 257] + [fu.device_case(*c) for c in fu.FRAME_EDGE_CASES]
    yield H.check(f"formant edge rows {[c['x'].size for c in small]}", not run_formant(exe, work, small))
    for zoff in (2, 4, 6):
        yield H.check(f"formant destination + {zoff} bytes", not run_formant(exe, work, [small[1], small[4]], zoff=zoff))
    if reduced:
        return
    rest = [fu.device_case(*c) for c in fu.DEVICE_CASES if c[2] > 257]
    yield H.check(f"formant rows {[c['x'].size for c in rest]}", not run_formant(exe, work, rest))
    every = [fu.device_case(*c) for c in fu.DEVICE_CASES]
    yield H.check("formant every case of DEVICE_CASES in one call", not run_formant(exe, work, every))


if __name__ == "__main__":
    H.main(NAME, cases, __doc__)
