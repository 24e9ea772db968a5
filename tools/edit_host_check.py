#!/usr/bin/env python3
"""The kernels of csrc/vv_edit.hip on the CPU under sanitizers, against numpy, bit for bit.

Builds tools/edit_host_check.cpp (the kernel source on tools/hip_host_shim.h, exact-size heap buffers) twice, with
-fsanitize=address,undefined and with -fsanitize=thread, and runs
  splice  : 0, 1, 255, 256, 257 and 600 descriptor rows (one, two and three LDS passes) x B of 1 and 3 x ld_out of 4 and 1000; in every
            case with a row, one starts at output sample 0, one ends at sample ld_out - 1 and one reads src[n_src - 1]; rows of no
            samples fill a list that the output has no room for; the rows of the items are shuffled over the passes
  restore : n_mel of 4 and 100 x cd of n_mel and n_mel + 4 x ld_keep of N and N + 3, seq_len of 0, N and N + 5 in one batch of three,
            on 2 workgroups (the device launches up to 2048), so that the grid-stride loop takes further trips
The full and the reduced list are the same: every case is an edge and the whole takes seconds.  Needs no GPU.

    python tools/edit_host_check.py [--cxx clang++] [--keep DIR] [--san asan|tsan|both] [--reduced]"""
import os
import struct
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import host_check_common as H  # noqa: E402
import numpy as np  # noqa: E402

NAME = "edit"
SPLICE_ROWS = (0, 1, 255, 256, 257, 600)


def find_cxx():
    return H.find_cxx()


def build(cxx, work, san="asan"):
    return H.build(NAME, cxx, work, san)


def splice_case(n_rows, B, ld_out, seed):
    """-> (src int16, rows [[item, src_off, dst_off, n]], want int16 [B, ld_out]); the rows of one item are disjoint on the output."""
    rng = np.random.default_rng(seed)
    n_src = 1203
    src = rng.integers(-32768, 32768, n_src).astype(np.int16)
    src[-1] = 32767
    rows = []
    for b, part in enumerate(np.array_split(np.arange(n_rows), B)):
        m = part.size
        k = min(m, (ld_out + 1) // 2)                                       # rows with samples: spans between 2 k sorted cut points
        if k:
            inner = np.sort(rng.choice(np.arange(1, ld_out), 2 * k - 2, replace=False)) if k > 1 else np.array([], np.int64)
            cuts = np.concatenate([[0], inner, [ld_out]]).astype(np.int64)   # the first span starts at 0, the last ends at ld_out
            for a0, a1 in cuts.reshape(-1, 2):
                n = int(a1 - a0)
                rows.append([b, int(rng.integers(0, n_src - n + 1)), int(a0), n])
        rows += [[b, int(rng.integers(0, n_src + 1)), int(rng.choice(cuts)), 0] for _ in range(m - k)]      # at a seam: inside no span
    if rows:
        r = max(rows, key=lambda r: r[3])
        r[1] = n_src - r[3]                                                 # the last sample read is src[n_src - 1]
        rows = [rows[i] for i in rng.permutation(len(rows))]
    want = np.zeros((B, ld_out), np.int16)
    for b, so, do, n in rows:
        want[b, do: do + n] = src[so: so + n]
    return src, rows, want


def restore_case(n_mel, cd, pad, seed):
    rng = np.random.default_rng(seed)
    B, N = 3, (300 if n_mel == 4 else 37)                                   # 900 and 2775 float4s: more than 2 workgroups hold
    ld_keep = N + pad
    x = rng.standard_normal((B, N, n_mel)).astype(np.float32)
    cat = rng.standard_normal((B, N, cd)).astype(np.float32)
    keep = rng.choice(np.array([0, 0, 1, 255], np.uint8), (B, ld_keep))
    keep[:, 0], keep[:, N - 1] = 1, 1
    seq_len = np.array([0, N, N + 5], np.int32)
    want = x.copy()
    for b in range(B):
        t = np.arange(N)
        m = (t < seq_len[b]) & (keep[b, :N] != 0)
        want[b, m] = cat[b, m, :n_mel]
    return x, cat, keep, seq_len, want


def cases(exe, work, reduced=False):
    """Runs every case through exe; yields (label, equal to numpy)."""
    fin, fout = os.path.join(work, "edit_in.bin"), os.path.join(work, "edit_out.bin")
    seed = 0
    for n_rows in SPLICE_ROWS:
        for B in (1, 3):
            for ld_out in (4, 1000):
                seed += 1
                src, rows, want = splice_case(n_rows, B, ld_out, seed)
                with open(fin, "wb") as f:
                    f.write(struct.pack("<4q", src.size, len(rows), B, ld_out) + np.array(rows, np.int64).tobytes() + src.tobytes())
                H.run(exe, ["splice", fin, fout])
                got = np.fromfile(fout, np.int16).reshape(B, ld_out)
                yield H.check(f"splice rows {n_rows} B {B} ld_out {ld_out}", np.array_equal(got, want))
    for n_mel in (4, 100):
        for cd in (n_mel, n_mel + 4):
            for pad in (0, 3):
                seed += 1
                x, cat, keep, seq_len, want = restore_case(n_mel, cd, pad, seed)
                with open(fin, "wb") as f:
                    f.write(struct.pack("<6q", x.shape[0], x.shape[1], n_mel, cd, keep.shape[1], 2))
                    for part in (x, cat, keep, seq_len):
                        f.write(part.tobytes())
                H.run(exe, ["restore", fin, fout])
                got = np.fromfile(fout, np.float32).reshape(x.shape)
                yield H.check(f"restore n_mel {n_mel} cd {cd} ld_keep N+{pad}", np.array_equal(got.view(np.uint32), want.view(np.uint32)))


if __name__ == "__main__":
    H.main(NAME, cases, __doc__)
