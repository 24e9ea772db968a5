#!/usr/bin/env python3
"""The kernels of csrc/vv_prosody.hip on the CPU under address and undefined-behaviour sanitizers.

Builds tools/prosody_host_check.cpp (a stand-alone program: the kernel source with host stand-ins for the HIP keywords, one thread per
GPU thread, exact-size heap buffers) with  clang++ -std=c++20 -ffp-contract=off -fsanitize=address,undefined  and runs it on the requests
of tests/test_prosody_gpu.py (tests/prosody_util.stretch_cases: every length under every ratio): all of them in one launch, a subset in
another order, and the destination 2, 4 and 6 bytes past an 8-byte boundary.  Every result must equal the numpy mirror (pos and PCM
array_equal), nothing outside a request's output may be written, and the sanitizers must stay silent.  Needs no GPU; takes a minute or two.

    python tools/prosody_host_check.py [--cxx clang++] [--keep DIR] [--quick] [--san asan|tsan] [--reduced]"""
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
from tests.prosody_util import stretch_cases  # noqa: E402
from vietvoice_tts_amd.core import audio_processor as ap  # noqa: E402

GUARD, SENTINEL, POS_SENTINEL = 64, -21846, -1431655766


SANITIZERS = {"asan": ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"], "tsan": ["-fsanitize=thread"]}
TIME_LIMIT = 600      # seconds for one run of the built program


def main(argv=None):
    p = argparse.ArgumentParser()
    p.add_argument("--cxx", default=os.environ.get("CXX") or next((c for c in ("/opt/rocm/lib/llvm/bin/clang++", shutil.which("clang++")) if c and os.path.exists(c)), "clang++"))
    p.add_argument("--keep", default="")
    p.add_argument("--san", choices=("asan", "tsan"), default="asan", help="address + undefined behaviour, or thread")
    p.add_argument("--reduced", action="store_true", help="a third of the requests in one launch, a ninth at each destination offset")
    p.add_argument("--quick", action="store_true", help="one launch of a third of the requests")
    a = p.parse_args(argv)
    work = a.keep or tempfile.mkdtemp(prefix="prosody_host_")
    os.makedirs(work, exist_ok=True)
    exe = os.path.join(work, "prosody_host_check")
    subprocess.run([a.cxx, "-std=c++20", "-O1", "-g", "-ffp-contract=off", *SANITIZERS[a.san],
                    "-pthread", "-w", os.path.join(ROOT, "tools", "prosody_host_check.cpp"), "-o", exe], check=True)
    items = [(name, x, p_, q_) + ap.time_stretch(x, p_, q_) for name, x, p_, q_ in stretch_cases()]

    def run(order, gap, yoff=0):
        plane, reqs = pack_requests([[items[i][1]] for i in order], gap=gap)
        rows, dst, po = [], GUARD, 3
        for k, (i, ((so, n),)) in enumerate(zip(order, reqs)):
            _name, _x, p_, q_, y, pos = items[i]
            rows.append([so, n, dst, p_, q_, po])
            dst += y.size + 1 + (k % 4)                      # every alignment of the destination's 8-byte grid
            po += pos.size + (k % 3)                         # gaps in pos as well
        n_y, n_pos = dst + GUARD, po + 5
        y0 = np.full(n_y, SENTINEL, np.int16)
        fin, fout = os.path.join(work, "in.bin"), os.path.join(work, "out.bin")
        with open(fin, "wb") as f:
            f.write(struct.pack("<4q", len(rows), plane.size, n_y, n_pos))
            for part in (np.array(rows, np.int64), ap.wsola_window(), plane, y0):
                f.write(np.ascontiguousarray(part).tobytes())
        env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0")
        r = subprocess.run([exe, fin, fout, f"yoff={yoff}"], capture_output=True, text=True, env=env, timeout=TIME_LIMIT)
        if r.returncode != 0 or r.stderr.strip():
            raise SystemExit(f"the host program failed (exit {r.returncode}):\n{r.stderr[-4000:]}")
        raw = open(fout, "rb").read()
        got_pos = np.frombuffer(raw[: 4 * n_pos], np.int32)
        got_y = np.frombuffer(raw[4 * n_pos:], np.int16)
        wrote_y, wrote_pos, bad = np.zeros(n_y, bool), np.zeros(n_pos, bool), []
        for i, (_so, _n, do, _p, _q, po_) in zip(order, rows):
            name, _x, _p, _q, y, pos = items[i]
            wrote_y[do: do + y.size] = True
            wrote_pos[po_: po_ + pos.size] = True
            if not (np.array_equal(got_y[do: do + y.size], y) and np.array_equal(got_pos[po_: po_ + pos.size], pos)):
                bad.append(name)
        if not ((got_y[~wrote_y] == SENTINEL).all() and (got_pos[~wrote_pos] == POS_SENTINEL).all()):
            bad.append("something outside a request's output was written")
        print(f"requests {len(order):2d}  gap {gap}  destination + {2 * yoff} bytes  " + ("equal to the mirror" if not bad else f"DIFFERS: {bad}"),
              flush=True)
        return not bad

    every = list(range(len(items)))
    if a.reduced:
        ok = [run(every[::3], 3)] + [run(every[1::9], 3, yoff=k) for k in (1, 2, 3)]
    elif a.quick:
        ok = [run(every[::3], 3)]
    else:
        ok = [run(every, 3), run(every[::-5], 2), run([every[-1]], 9)] + [run(every[1::4], 3, yoff=k) for k in (1, 2, 3)]
    if not a.keep:
        shutil.rmtree(work, ignore_errors=True)
    if not all(ok):
        raise SystemExit(1)
    print("ok: the kernels equal the mirror bit for bit; no sanitizer report")


if __name__ == "__main__":
    main()
