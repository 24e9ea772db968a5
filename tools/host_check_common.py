"""What the tools/*_host_check.py built on tools/hip_host_shim.h share: the compiler, the two sanitizer builds, one run under a time limit.

    asan : -fsanitize=address,undefined   an index past the end of an exact-size block, a misaligned vector access, a signed overflow
    tsan : -fsanitize=thread              an LDS (or HBM) write and a read by two threads of a workgroup with no barrier between them
One program cannot have both.  A report of either is text on stderr and a non-zero exit: run() raises on both."""
import argparse
import os
import shutil
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

SANITIZERS = {"asan": ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"], "tsan": ["-fsanitize=thread"]}
ENV = {"ASAN_OPTIONS": "detect_leaks=0", "UBSAN_OPTIONS": "print_stacktrace=1", "TSAN_OPTIONS": "halt_on_error=1"}
TIME_LIMIT = 300          # seconds for one run of a built program: a kernel that broke the shuffle rule of the shim would wait for ever


def find_cxx():
    return os.environ.get("CXX") or next((c for c in ("/opt/rocm/lib/llvm/bin/clang++", shutil.which("clang++")) if c and os.path.exists(c)), None)


def build(name, cxx, work, san="asan", extra=()):
    """tools/<name>_host_check.cpp -> work/<name>_host_check_<san>"""
    exe = os.path.join(work, f"{name}_host_check_{san}")
    subprocess.run([cxx, "-std=c++20", "-O1", "-g", "-ffp-contract=off", *SANITIZERS[san], "-pthread", "-w", *extra,
                    os.path.join(ROOT, "tools", f"{name}_host_check.cpp"), "-o", exe], check=True)
    return exe


def run(exe, args, timeout=TIME_LIMIT):
    r = subprocess.run([exe, *[str(a) for a in args]], capture_output=True, text=True, env=dict(os.environ, **ENV), timeout=timeout)
    if r.returncode != 0 or r.stderr.strip():
        raise RuntimeError(f"{os.path.basename(exe)} {' '.join(str(a) for a in args[:1])} failed (exit {r.returncode}):\n{r.stderr[-4000:]}")


def main(name, cases, doc):
    """The command line of one tool: both builds (or one), the full list (or the reduced one of the suite)."""
    p = argparse.ArgumentParser(description=doc, formatter_class=argparse.RawDescriptionHelpFormatter)
    p.add_argument("--cxx", default=find_cxx() or "clang++")
    p.add_argument("--keep", default="")
    p.add_argument("--san", choices=("asan", "tsan", "both"), default="both")
    p.add_argument("--reduced", action="store_true", help="the list tests/test_host_sanitizers_cpu.py runs")
    a = p.parse_args()
    work = a.keep or tempfile.mkdtemp(prefix=f"{name}_host_")
    os.makedirs(work, exist_ok=True)
    ok = True
    for san in (("asan", "tsan") if a.san == "both" else (a.san,)):
        t0 = time.time()
        exe = build(name, a.cxx, work, san)
        t1 = time.time()
        res = list(cases(exe, work, a.reduced))
        bad = [label for label, good in res if not good]
        print(f"{name} {san}: {len(res)} cases, {len(bad)} differ {bad[:8]}  (build {t1 - t0:.0f} s, run {time.time() - t1:.0f} s)", flush=True)
        ok &= not bad
    if not a.keep:
        shutil.rmtree(work, ignore_errors=True)
    if not ok:
        raise SystemExit(1)
    print("ok: the kernels equal the mirror bit for bit; no sanitizer report")


def check(label, good):
    """One case's verdict, printed where it fails; returns the pair the callers collect."""
    if not good:
        print(f"  DIFFERS: {label}", flush=True)
    return label, bool(good)


FILL = 0xAA               # what an output holds before a launch; what no thread owns must still hold it afterwards


def filled(shape, dtype):
    """An output buffer before its launch: every byte 0xAA."""
    import numpy as np
    a = np.empty(shape, dtype)
    a.view(np.uint8).reshape(-1)[:] = FILL
    return a


def still_filled(a):
    """Every byte of ``a`` (a slice of an output that no thread owns) is still 0xAA."""
    import numpy as np
    return bool((np.ascontiguousarray(a).view(np.uint8) == FILL).all())


class Alias:
    """Argument: the block of argument ``k`` of the same launch once more."""
    def __init__(self, k):
        self.k = k


class Off:
    """Argument: a block whose first byte lies ``byte_off`` past a 16-byte boundary (its last byte still ends the allocation)."""
    def __init__(self, a, byte_off):
        self.a, self.byte_off = a, byte_off


class Batch:
    """The launches of one run of a program on tools/host_check_driver.h.  add() takes a kernel's arguments in order: a numpy array is an
    exact-size block holding it (an output comes as filled()), None a null pointer, an int or a float a scalar; run() returns, per launch,
    {argument index: the block after the launch, in the array's dtype and shape}."""

    def __init__(self, exe, work, name):
        self.exe, self.fin, self.fout = exe, os.path.join(work, f"{name}_in.bin"), os.path.join(work, f"{name}_out.bin")
        self.parts, self.outs = [], []

    def add(self, kernel, grid, block, args, shmem=0):
        import struct
        import numpy as np
        g = tuple(grid) + (1,) * (3 - len(tuple(grid))) if not isinstance(grid, int) else (grid, 1, 1)
        k = kernel.encode()
        b = [struct.pack("<q", len(k)), k, struct.pack("<6q", *g, block, shmem, len(args))]
        outs = {}
        for i, a in enumerate(args):
            off = 0
            if isinstance(a, Off):
                a, off = a.a, a.byte_off
            if a is None:
                b.append(struct.pack("<3q", 3, -1, 0))
            elif isinstance(a, Alias):
                b.append(struct.pack("<2q", 2, a.k))
            elif isinstance(a, np.ndarray):
                a = np.ascontiguousarray(a)
                b += [struct.pack("<3q", 3, a.nbytes, off), a.tobytes()]
                outs[i] = (a.dtype, a.shape, a.nbytes)
            elif isinstance(a, (bool, int, np.integer)):
                b.append(struct.pack("<2q", 0, int(a)))
            else:
                b.append(struct.pack("<qd", 1, float(a)))
        self.parts.append(b"".join(b))
        self.outs.append(outs)
        return len(self.outs) - 1

    def run(self, timeout=TIME_LIMIT):
        import struct
        import numpy as np
        with open(self.fin, "wb") as f:
            f.write(struct.pack("<q", len(self.parts)) + b"".join(self.parts))
        run(self.exe, [self.fin, self.fout], timeout)
        raw, pos, res = open(self.fout, "rb").read(), 0, []
        for outs in self.outs:
            d = {}
            for i, (dt, shape, nb) in outs.items():
                d[i] = np.frombuffer(raw, dt, nb // max(dt.itemsize, 1), pos).reshape(shape)
                pos += nb
            res.append(d)
        assert pos == len(raw), "the program wrote another number of bytes than its blocks hold"
        self.parts, self.outs = [], []
        return res


def pack_signals(sigs, gap=3):
    """int16 signals into one plane, the first at element 0, the last ending the plane, ``gap`` samples of 32767 junk between them (source
    offsets that are no multiple of a hop) -> (plane, offsets)"""
    import numpy as np
    parts, offs, pos = [], [], 0
    for k, s in enumerate(sigs):
        if k:
            parts.append(np.full(gap, 32767, np.int16))
            pos += gap
        parts.append(np.asarray(s, np.int16).reshape(-1))
        offs.append(pos)
        pos += parts[-1].size
    return np.concatenate(parts), offs


def place_outputs(lens):
    """Destinations of the rows, the first at element 0, the last ending the buffer, 1 to 4 untouched samples between -> (offsets, total)"""
    offs, pos = [], 0
    for k, n in enumerate(lens):
        if k:
            pos += 1 + (k % 4)
        offs.append(pos)
        pos += n
    return offs, pos
