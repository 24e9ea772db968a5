#!/usr/bin/env python3
"""The kernels of csrc/vv_flac_decode.hip on the CPU under address and undefined-behaviour sanitizers.

Builds tools/flac_decode_host_check.cpp (a stand-alone program: the kernel source with host stand-ins for the HIP keywords, exact-size
heap buffers) with  clang++ -std=c++20 -fsanitize=address,undefined  and feeds it
  * the valid streams of tests/flac_decode_util.cases(), as one batch: the PCM bytes must equal the Python mirror's;
  * the malformed streams of tests/flac_decode_util.malformed() and malformed_corpus() (every truncation and every single-bit flip of two
    small streams), as one batch: the reason code and the byte position must equal the mirror's (a flip that leaves the stream valid
    must give the mirror's samples);
the sanitizers must stay silent.  A stream the container parser refuses never reaches the kernels and is only counted.  Needs no GPU.

    python tools/flac_decode_host_check.py [--cxx clang++] [--keep DIR] [--valid | --malformed] [--san asan|tsan]"""
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


def find_cxx():
    return os.environ.get("CXX") or next((c for c in ("/opt/rocm/lib/llvm/bin/clang++", shutil.which("clang++")) if c and os.path.exists(c)), None)


SANITIZERS = {"asan": ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"], "tsan": ["-fsanitize=thread"]}
TIME_LIMIT = 600      # seconds for one run of the built program


def build(cxx, work, san="asan"):
    exe = os.path.join(work, "flac_decode_host_check" + ("" if san == "asan" else "_" + san))
    subprocess.run([cxx, "-std=c++20", "-O1", "-g", *SANITIZERS[san], "-pthread", "-w",
                    os.path.join(ROOT, "tools", "flac_decode_host_check.cpp"), "-o", exe], check=True)
    return exe


def run(exe, work, streams):
    """streams [(name, bytes)] through the host program in one batch, against the mirror: -> (streams the kernels saw, refused in the
    container, the names that differ)."""
    from vietvoice_tts_amd.core.audio_processor import FlacError, flac_container, flac_decode
    rows, parts, want, names, pos, skipped = [], [], [], [], 0, 0
    for name, data in streams:
        try:
            info = flac_container(data)
        except FlacError:
            skipped += 1
            continue
        body = data[info.start:]
        rows.append([pos, len(body), info.channels, info.bits, info.min_block, info.max_block, info.rate, info.total])
        parts.append(body + b"\0" * (-len(body) % 4))
        pos += len(parts[-1])
        try:
            frames, _w, _r = flac_decode(data)
            want.append((0, frames.shape[0], frames.tobytes()))
        except FlacError as e:
            want.append((e.code, e.position - info.start, b""))
        names.append(name)
    buf = b"".join(parts)
    buf += b"\0" * (-len(buf) % 8 + 8)
    R = len(rows)
    fin, fout = os.path.join(work, "in.bin"), os.path.join(work, "out.bin")
    with open(fin, "wb") as f:
        f.write(struct.pack("<2q", R, len(buf)) + np.array(rows, np.int64).tobytes() + buf)
    r = subprocess.run([exe, fin, fout], capture_output=True, text=True, env=dict(os.environ, ASAN_OPTIONS="detect_leaks=0"), timeout=TIME_LIMIT)
    if r.returncode != 0 or r.stderr.strip():
        raise SystemExit(f"the host program failed (exit {r.returncode}):\n{r.stderr[-4000:]}")
    raw = open(fout, "rb").read()
    info = np.frombuffer(raw[: 32 * R], np.int64).reshape(R, 4)
    info2 = np.frombuffer(raw[32 * R: 48 * R], np.int64).reshape(R, 2)
    lay = np.frombuffer(raw[48 * R: 96 * R], np.int64).reshape(R, 6)
    pcm = raw[96 * R + 8:]
    bad = []
    for i, (code, n, data) in enumerate(want):
        if code:
            got = (int(info[i, 0]), int(info[i, 1])) if info[i, 0] else (int(info2[i, 0]), int(info2[i, 1]))
            ok = got == (code, n)
        else:
            ok = info[i, 0] == 0 and info2[i, 0] == 0 and info[i, 3] == n and pcm[lay[i, 0]: lay[i, 0] + len(data)] == data
        if not ok:
            bad.append(names[i])
    return R, skipped, bad


def main(argv=None):
    p = argparse.ArgumentParser()
    p.add_argument("--cxx", default=find_cxx() or "clang++")
    p.add_argument("--keep", default="")
    p.add_argument("--san", choices=("asan", "tsan"), default="asan", help="address + undefined behaviour, or thread")
    p.add_argument("--valid", action="store_true")
    p.add_argument("--malformed", action="store_true")
    a = p.parse_args(argv)
    from tests.flac_decode_util import cases, malformed, malformed_corpus
    work = a.keep or tempfile.mkdtemp(prefix="flac_decode_host_")
    os.makedirs(work, exist_ok=True)
    exe = build(a.cxx, work, a.san)
    ok = True
    if a.valid or not a.malformed:
        n, skipped, bad = run(exe, work, [(c[0], c[1]) for c in cases()])
        print(f"valid streams: {n} through the kernels, {skipped} refused in the container, {len(bad)} differ {bad[:8]}", flush=True)
        ok &= not bad and not skipped
    if a.malformed or not a.valid:
        n, skipped, bad = run(exe, work, [(m[0], m[1]) for m in malformed()] + list(malformed_corpus()))
        print(f"malformed streams: {n} through the kernels, {skipped} refused in the container, {len(bad)} differ {bad[:8]}", flush=True)
        ok &= not bad
    if not a.keep:
        shutil.rmtree(work, ignore_errors=True)
    if not ok:
        raise SystemExit(1)
    print("ok: the kernels equal the mirror in samples, reason codes and positions; no sanitizer report")


if __name__ == "__main__":
    main()
