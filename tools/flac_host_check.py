#!/usr/bin/env python3
"""The kernels of csrc/vv_flac.hip on the CPU under address and undefined-behaviour sanitizers.

Builds tools/flac_host_check.cpp (a stand-alone program: the kernel source with host stand-ins for the HIP keywords, one thread per GPU
thread, exact-size heap buffers) with  clang++ -std=c++20 -fsanitize=address,undefined  and runs it on the rows of
tests/test_flac_gpu.py (tests/flac_util.device_cases) in one launch, shuffled, at odd source offsets, with y sized to the frame bounds
exactly.  The bytes and info must equal the numpy mirror, nothing past the total may be written, and the sanitizers must stay silent.
Needs no GPU; takes about a minute.

With --lpc-order 1 ... 12 the kernels of vv_pcm_flac_lpc run, on the same rows plus the short frames and the frame without
energy under the window of tests/flac_lpc_util.lpc_cases, against the mirror with that order.

    python tools/flac_host_check.py [--cxx clang++] [--keep DIR] [--rate HZ] [--lpc-order P] [--san asan|tsan] [--reduced]"""
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

from tests.flac_util import device_cases  # noqa: E402
from tests.output_util import pack_requests  # noqa: E402

FILL = 0xAA


SANITIZERS = {"asan": ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"], "tsan": ["-fsanitize=thread"]}
TIME_LIMIT = 600      # seconds for one run of the built program


def main(argv=None):
    p = argparse.ArgumentParser()
    p.add_argument("--cxx", default=os.environ.get("CXX") or next((c for c in ("/opt/rocm/lib/llvm/bin/clang++", shutil.which("clang++")) if c and os.path.exists(c)), "clang++"))
    p.add_argument("--keep", default="")
    p.add_argument("--san", choices=("asan", "tsan"), default="asan", help="address + undefined behaviour, or thread")
    p.add_argument("--rate", type=int, default=24000)
    p.add_argument("--lpc-order", type=int, default=0)
    p.add_argument("--reduced", action="store_true", help="the first launch alone: every row, shuffled, at odd source offsets")
    a = p.parse_args(argv)
    work = a.keep or tempfile.mkdtemp(prefix="flac_host_")
    os.makedirs(work, exist_ok=True)
    exe = os.path.join(work, "flac_host_check")
    subprocess.run([a.cxx, "-std=c++20", "-O1", "-g", *SANITIZERS[a.san], "-ffp-contract=off", "-pthread", "-w",
                    os.path.join(ROOT, "tools", "flac_host_check.cpp"), "-o", exe], check=True)
    from tests.flac_lpc_util import lpc_cases, mirror_layout
    cases = lpc_cases() if a.lpc_order else device_cases()

    def run(order, gap):
        plane, reqs = pack_requests([[cases[i][1]] for i in order], gap=gap)
        rows = [[so, n, cases[i][2], cases[i][3]] for i, ((so, n),) in zip(order, reqs)]
        want, info, bound = mirror_layout([cases[i] for i in order], a.rate, a.lpc_order)
        fin, fout = os.path.join(work, "in.bin"), os.path.join(work, "out.bin")
        with open(fin, "wb") as f:
            f.write(struct.pack("<4q", len(rows), plane.size, bound, a.rate))
            for part in (np.array(rows, np.int64), plane, np.full(bound, FILL, np.uint8)):
                f.write(np.ascontiguousarray(part).tobytes())
        r = subprocess.run([exe, fin, fout] + ([str(a.lpc_order)] if a.lpc_order else []), capture_output=True, text=True, env=dict(os.environ, ASAN_OPTIONS="detect_leaks=0"), timeout=TIME_LIMIT)
        if r.returncode != 0 or r.stderr.strip():
            raise SystemExit(f"the host program failed (exit {r.returncode}):\n{r.stderr[-4000:]}")
        raw = open(fout, "rb").read()
        got_info = np.frombuffer(raw[: 24 * (len(rows) + 1)], np.int64).reshape(-1, 3)
        got = np.frombuffer(raw[24 * (len(rows) + 1):], np.uint8)
        ok = np.array_equal(got_info, info) and np.array_equal(got[: want.size], want) and (got[want.size:] == FILL).all()
        print(f"rows {len(order):2d}  gap {gap}  rate {a.rate}  {want.size} bytes  " + ("equal to the mirror" if ok else "DIFFERS"), flush=True)
        return ok

    every = list(range(len(cases)))
    ok = [run(every, 3)] if a.reduced else [run(every, 3), run(every[::-3], 2), run([every[3]], 9)]
    if not a.keep:
        shutil.rmtree(work, ignore_errors=True)
    if not all(ok):
        raise SystemExit(1)
    print("ok: the kernels equal the mirror byte for byte; no sanitizer report")


if __name__ == "__main__":
    main()
