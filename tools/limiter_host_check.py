#!/usr/bin/env python3
"""The kernels of csrc/vv_limiter.hip on the CPU under address and undefined-behaviour sanitizers.

Builds tools/limiter_host_check.cpp (a stand-alone program: the kernel source with host stand-ins for the HIP keywords, one thread per
GPU thread, exact-size heap buffers) with  clang++ -std=c++20 -ffp-contract=off -fsanitize=address,undefined  and runs it on the requests
of tests/test_limiter_gpu.py: per look-ahead and mode all of them in one launch out of place and in place, a subset in another order,
output windows, the destination 2, 4 and 6 bytes past an 8-byte boundary, and a pre-gain read from a measurement.  Every result must
equal the numpy mirror (stats ==, PCM array_equal), nothing outside a request's window may be written, and the sanitizers must stay
silent.  Needs no GPU; takes a few minutes.

    python tools/limiter_host_check.py [--cxx clang++] [--keep DIR] [--quick] [--san asan|tsan] [--reduced]"""
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
from vietvoice_tts_amd.core import audio_processor as ap  # noqa: E402

SR, PEAK, GUARD, SENTINEL = 24000, -1.0, 64, -21846
MODES = ("sample", "true")


def _gpu_cases(L):
    """tests/test_limiter_gpu.py's signals without importing it (it needs torch and a device at import)."""
    import types
    src = open(os.path.join(ROOT, "tests", "test_limiter_gpu.py"), encoding="utf-8").read()
    mod = types.ModuleType("limiter_gpu_cases")
    stub = types.ModuleType("torch")
    pytest_stub = types.SimpleNamespace(mark=types.SimpleNamespace(gpu=None, parametrize=lambda *a, **k: (lambda f: f)),
                                        fixture=lambda *a, **k: (lambda f: f))
    sys.modules.setdefault("torch", stub)
    code = compile(src, "test_limiter_gpu.py", "exec")
    mod.__dict__["__name__"] = "limiter_gpu_cases"
    saved = sys.modules.get("pytest")
    sys.modules["pytest"] = pytest_stub
    try:
        exec(code, mod.__dict__)
    finally:
        if saved is not None:
            sys.modules["pytest"] = saved
        else:
            del sys.modules["pytest"]
        if sys.modules.get("torch") is stub:
            del sys.modules["torch"]
    return mod._cases(L)


SANITIZERS = {"asan": ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"], "tsan": ["-fsanitize=thread"]}
TIME_LIMIT = 600      # seconds for one run of the built program


def main(argv=None):
    p = argparse.ArgumentParser()
    p.add_argument("--cxx", default=os.environ.get("CXX") or next((c for c in ("/opt/rocm/lib/llvm/bin/clang++", shutil.which("clang++")) if c and os.path.exists(c)), "clang++"))
    p.add_argument("--keep", default="")
    p.add_argument("--san", choices=("asan", "tsan"), default="asan", help="address + undefined behaviour, or thread")
    p.add_argument("--quick", action="store_true", help="L = 3 only")
    p.add_argument("--reduced", action="store_true", help="L = 3: every request once, six at each destination offset, the windows in place")
    a = p.parse_args(argv)
    work = a.keep or tempfile.mkdtemp(prefix="limit_host_")
    os.makedirs(work, exist_ok=True)
    exe = os.path.join(work, "limiter_host_check")
    subprocess.run([a.cxx, "-std=c++20", "-O1", "-g", "-ffp-contract=off", *SANITIZERS[a.san],
                    "-pthread", "-w", os.path.join(ROOT, "tools", "limiter_host_check.cpp"), "-o", exe], check=True)

    def run(items, L, mode, order, gap, in_place=False, yoff=0, windows=None, meas=None, targets=None):
        """items = [(name, x, gain, want_y, want_stats)]"""
        plane, reqs = pack_requests([[items[i][1]] for i in order], gap=gap)
        rows, pos = [], GUARD
        for k, ((so, n),) in enumerate(reqs):
            lo, on = (0, n) if windows is None else windows[k]
            rows.append([so, n, so + lo if in_place else pos, lo, on])
            pos += on + 1 + (len(rows) % 4)
        n_y = pos + GUARD
        y0 = np.full(n_y, SENTINEL, np.int16)
        c = ap.loudness_ceiling(PEAK)
        par = np.array([[ap.loudness_target(None if targets is None else targets[i]), c, items[i][2]] for i in order], np.float64)
        fin, fout = os.path.join(work, "in.bin"), os.path.join(work, "out.bin")
        with open(fin, "wb") as f:
            f.write(struct.pack("<6q", len(rows), L, MODES.index(mode), plane.size, n_y, 0 if meas is None else 1))
            parts = [np.array(rows, np.int64), ap.limiter_window(L), ap.limiter_taps(), par]
            if meas is not None:
                parts.append(np.array([meas[i] for i in order], np.float64))
            for part in parts + [plane, y0]:
                f.write(np.ascontiguousarray(part).tobytes())
        env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0")
        r = subprocess.run([exe, fin, fout] + (["inplace"] if in_place else []) + [f"yoff={yoff}"], capture_output=True, text=True, env=env, timeout=TIME_LIMIT)
        if r.returncode != 0 or r.stderr.strip():
            raise SystemExit(f"the host program failed (exit {r.returncode}):\n{r.stderr[-4000:]}")
        raw = open(fout, "rb").read()
        st = np.frombuffer(raw[: 32 * len(rows)], np.float64).reshape(-1, 4)
        y = np.frombuffer(raw[32 * len(rows):], np.int16)
        base, written, bad = (plane if in_place else y0), np.zeros(y.size, bool), []
        for k, (i, (_so, n, do, lo, on)) in enumerate(zip(order, rows)):
            written[do: do + on] = True
            name, _x, _g, want_y, want_st = items[i]
            if not (np.all(st[k] == want_st) and np.array_equal(y[do: do + on], want_y[lo: lo + on])):
                bad.append(name)
        if not np.array_equal(y[~written], base[~written]):
            bad.append("a sample outside a request's window was written")
        print(f"L {L:4d} {mode:6s} requests {len(order):2d}  gap {gap}  in_place {int(in_place)}  windows {int(windows is not None)}  meas {int(meas is not None)}  "
              f"destination + {2 * yoff} bytes  " + ("equal to the mirror" if not bad else f"DIFFERS: {bad}"), flush=True)
        return not bad

    ok = []
    for L in ((3,) if a.quick or a.reduced else (3, 120, 1024)):
        cases = _gpu_cases(3 if L == 1024 else L)
        if L != 3:
            cases = [c for c in cases if c[1].size <= 6000][:6] + ([] if L == 1024 else cases[-1:])      # one thread per GPU thread is slow
        for mode in MODES:
            items = []
            for name, x, g in cases:
                y, st = ap.limit_peaks(x, SR, PEAK, mode, gain=g, L=L)
                items.append((name, x, g, y, np.array([st["g"], st["e_max"], st["s_min"], st["n_limited"]])))
            every = list(range(len(items)))
            if a.reduced:
                W = 2 * L + ap.LIMIT_H
                win = [(min(x.size, (0, 1, W, x.size // 2, 2047)[k % 5]), 0) for k, (_n, x, *_r) in enumerate(items)]
                win = [(lo, (x.size - lo, max(0, min(x.size - lo, x.size // 3)), 0, min(x.size - lo, 1))[k % 4]) for k, ((lo, _z), (_n, x, *_r)) in enumerate(zip(win, items))]
                ok += [run(items, L, mode, every, 3), run(items, L, mode, every, 3, windows=win, in_place=True)]
                ok += [run(items, L, mode, [13, 9, 11, 6, 0, 12], 2, yoff=k, in_place=k == 2) for k in (1, 2, 3)]
                continue
            ok += [run(items, L, mode, every, 3), run(items, L, mode, every, 3, in_place=True)]
            if L == 3:
                ok += [run(items, L, mode, [13, 9, 11, 6, 0, 12], 2), run(items, L, mode, [13], 9)]
                ok += [run(items, L, mode, every, 3, yoff=k, in_place=k == 2) for k in (1, 2, 3)]
                W = 2 * L + ap.LIMIT_H
                win = []
                for k, (_n, x, *_r) in enumerate(items):
                    n = x.size
                    lo = min(n, (0, 1, W, n // 2, 2047)[k % 5])
                    win.append((lo, (n - lo, max(0, min(n - lo, n // 3)), 0, min(n - lo, 1))[k % 4]))
                ok += [run(items, L, mode, every, 3, windows=win), run(items, L, mode, every, 3, windows=win, in_place=True)]
    # the pre-gain from a measurement
    from tests.loudness_util import speechlike
    xs = [speechlike(30000, SR, seed=61), np.zeros(3000, np.int16), speechlike(14000, SR, seed=64)]
    xs[0][7000] = 32767
    targets = [-12.0, -16.0, None]
    items, meas = [], []
    for x, t, g0 in zip(xs, targets, (1.0, 1.0, 3.0)):
        _L, zbar, kept, peak = ap.measure_loudness(x, SR)
        T = ap.loudness_target(t)
        meas.append([zbar, kept, peak, ap.loudness_gain(zbar, kept, peak, T, ap.loudness_ceiling(PEAK))])
        g = ap.limiter_pregain(zbar, kept, peak, T) if t is not None else g0
        y, st = ap.limit_peaks(x, SR, PEAK, "true", gain=g, L=120)
        items.append((f"meas{len(items)}", x, g0, y, np.array([st["g"], st["e_max"], st["s_min"], st["n_limited"]])))
    if not a.reduced:
        ok.append(run(items, 120, "true", [0, 1, 2], 3, meas=meas, targets=targets, in_place=True))
    if not a.keep:
        shutil.rmtree(work, ignore_errors=True)
    if not all(ok):
        raise SystemExit(1)
    print("ok: the kernels equal the mirror bit for bit; no sanitizer report")


if __name__ == "__main__":
    main()
