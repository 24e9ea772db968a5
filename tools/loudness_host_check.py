#!/usr/bin/env python3
"""The kernels of csrc/vv_loudness.hip on the CPU under address and undefined-behaviour sanitizers.

Builds tools/loudness_host_check.cpp (a stand-alone program: the kernel source with host stand-ins for the HIP keywords, one thread per
GPU thread, exact-size heap buffers) with  clang++ -std=c++20 -ffp-contract=off -fsanitize=address,undefined  and runs it on the requests
of tests/test_loudness_gpu.py: all of them in one launch out of place and in place, a subset in another order, one alone, an empty one, and
the destination 2, 4 and 6 bytes past an 8-byte boundary.  Every result must equal the numpy mirror (stats ==, PCM array_equal), nothing
outside a request's slice may be written, and the sanitizers must stay silent.  Needs no GPU; takes about a minute.

    python tools/loudness_host_check.py [--cxx clang++] [--keep DIR] [--san asan|tsan] [--reduced]"""
import argparse
import os
import shutil
import struct
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402

from tests.output_util import pack_requests  # noqa: E402
from tests.test_loudness_gpu import _cases  # noqa: E402
from vietvoice_tts_amd.core import audio_processor as ap  # noqa: E402

SR, PEAK, GUARD, SENTINEL = 24000, -1.0, 64, -21846


SANITIZERS = {"asan": ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"], "tsan": ["-fsanitize=thread"]}
TIME_LIMIT = 600      # seconds for one run of the built program


def main(argv=None):
    p = argparse.ArgumentParser()
    p.add_argument("--cxx", default=os.environ.get("CXX") or next((c for c in ("/opt/rocm/lib/llvm/bin/clang++", shutil.which("clang++")) if c and os.path.exists(c)), "clang++"))
    p.add_argument("--keep", default="")
    p.add_argument("--san", choices=("asan", "tsan"), default="asan", help="address + undefined behaviour, or thread")
    p.add_argument("--reduced", action="store_true", help="every request once, in place, and three at each destination offset")
    a = p.parse_args(argv)
    work = a.keep or tempfile.mkdtemp(prefix="loud_host_")
    os.makedirs(work, exist_ok=True)
    exe = os.path.join(work, "loudness_host_check")
    subprocess.run([a.cxx, "-std=c++20", "-O1", "-g", "-ffp-contract=off", *SANITIZERS[a.san],
                    "-pthread", "-w", os.path.join(ROOT, "tools", "loudness_host_check.cpp"), "-o", exe], check=True)
    sub = SR // 10
    rps, _last = ap._loud_run_lengths(sub)
    items = []
    for name, x, target in _cases():
        _L, zbar, kept, peak = ap.measure_loudness(x, SR)
        g = ap.loudness_gain(zbar, kept, peak, ap.loudness_target(target), ap.loudness_ceiling(PEAK))
        items.append((name, x, target, np.array([zbar, kept, peak, g]), ap.normalize_loudness(x, SR, target, PEAK)))

    def run(order, gap, in_place=False, yoff=0):
        plane, reqs = pack_requests([[items[i][1]] for i in order], gap=gap)
        rows, pos, runs, max_n = [], GUARD, 0, 0
        for (so, n), in reqs:
            rows.append([so, n, so if in_place else pos, runs])
            runs += (n // sub) * rps + -(-(n % sub) // ap.LOUD_RUN)
            pos += n + 1 + (len(rows) % 4)
            max_n = max(max_n, n)
        n_y = pos + GUARD
        y0 = np.full(n_y, SENTINEL, np.int16)
        par = np.array([[ap.loudness_target(items[i][2]), ap.loudness_ceiling(PEAK)] for i in order], np.float64)
        fin, fout = os.path.join(work, "in.bin"), os.path.join(work, "out.bin")
        with open(fin, "wb") as f:
            f.write(struct.pack("<6q", len(rows), sub, plane.size, n_y, runs, max_n))
            for part in (np.array(rows, np.int64), ap.loudness_tables(SR), par, plane, y0):
                f.write(np.ascontiguousarray(part).tobytes())
        env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0")
        r = subprocess.run([exe, fin, fout] + (["inplace"] if in_place else []) + [f"yoff={yoff}"], capture_output=True, text=True, env=env, timeout=TIME_LIMIT)
        if r.returncode != 0 or r.stderr.strip():
            raise SystemExit(f"the host program failed (exit {r.returncode}):\n{r.stderr[-4000:]}")
        raw = open(fout, "rb").read()
        st = np.frombuffer(raw[: 32 * len(rows)], np.float64).reshape(-1, 4)
        y = np.frombuffer(raw[32 * len(rows):], np.int16)
        base, written, bad = (plane if in_place else y0), np.zeros(y.size, bool), []
        for k, (i, (_so, n, do, _ro)) in enumerate(zip(order, rows)):
            written[do: do + n] = True
            name, _x, _t, want_st, want_y = items[i]
            if not (np.all(st[k] == want_st) and np.array_equal(y[do: do + n], want_y)):
                bad.append(name)
        if not np.array_equal(y[~written], base[~written]):
            bad.append("a sample outside a request's slice was written")
        print(f"requests {len(order):2d}  gap {gap}  in_place {int(in_place)}  destination + {2 * yoff} bytes  runs {runs:5d}  " + ("equal to the mirror" if not bad else f"DIFFERS: {bad}"))
        return not bad

    every = list(range(len(items)))
    if a.reduced:
        ok = [run(every, 3, in_place=True), run([0], 3)] + [run([11, 0, len(items) - 1], 3, yoff=k) for k in (1, 2, 3)]
    else:
        ok = [run(every, 3), run(every, 3, in_place=True), run([11, 9, 14, 6, 0, 13, 5, len(items) - 1], 2), run([11], 9), run([0], 3)]
        ok += [run(every, 3, yoff=k) for k in (1, 2, 3)]
    if not a.keep:
        shutil.rmtree(work, ignore_errors=True)
    if not all(ok):
        raise SystemExit(1)
    print("ok: the kernels equal the mirror bit for bit; no sanitizer report")


if __name__ == "__main__":
    main()
