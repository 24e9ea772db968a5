#!/usr/bin/env python3
"""noise_fill_kernel of csrc/vv_noise.hip on the CPU under sanitizers, against tests/philox_reference.py.

Builds tools/noise_host_check.cpp (the kernel source on tools/hip_host_shim.h, exact-size heap buffers) twice, with
-fsanitize=address,undefined and with -fsanitize=thread, and runs CASES: both kinds x n_mel of 4 and 100 x N of 1 and 37, B = 3 with
seq_len of -3, 0 and N + 5 (clamped to 0, 0 and N), and the device test's lengths (37, 1, 0) with the all-ones key words.
  x is one exact block of B N n_mel floats, filled with 0xAA: the kernel owns every element (rows past a length are +0.0f), so none may
  keep the fill; seq_len and keys are exact blocks of B ints and 2 B 64-bit words.
  grid: restated from vvk_noise_fill (csrc/vv_noise.hip: `grid = min((total + 255) / 256, 256 * 8)`, 256 threads), but at most 2
  workgroups, so that the grid-stride loop takes further trips (N 37 x n_mel 100 x B 3 = 2775 groups against 512 threads).
  uniform: bit for bit.  normal: |z - z_ref| <= 2^-20 r, the device test's NORMAL_BOUND (tests/test_noise_gpu.py), whose derivation
  allows logf 1 ulp, sqrtf 1 and sinpif / cospif 2.  On the host cospif / sinpif are the shim's stand-ins (cos(pi x) in double, rounded
  once) and logf is the host libm's: the normal result speaks for the indexing of that path, not for the device's functions.
The full and the reduced list are the same: every case is an edge and the whole takes seconds.  Needs no GPU.

    python tools/noise_host_check.py [--cxx clang++] [--keep DIR] [--san asan|tsan|both] [--reduced]"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import host_check_common as H  # noqa: E402
import numpy as np  # noqa: E402

NAME = "noise"
ONES = (1 << 64) - 1
NORMAL_BOUND = 2.0 ** -20           # x r: tests/test_noise_gpu.py
# (n_mel, N, seq_len, keys): what tests/test_noise_gpu.py runs on the device as well
CASES = [(n_mel, N, (-3, 0, N + 5), ((9527, 1), (0, 0), (ONES, (1 << 63) | 5))) for n_mel in (4, 100) for N in (1, 37)]
CASES.append((100, 37, (37, 1, 0), ((ONES, ONES), (0, 1), (9527, 0))))
CASES.append((4, 37, (36, 37, 1), ((0, ONES), (ONES, 0), (1, 1))))


def find_cxx():
    return H.find_cxx()


def build(cxx, work, san="asan"):
    return H.build(NAME, cxx, work, san)


def reference(n_mel, N, seq, keys, kind):
    sys.path.insert(0, H.ROOT)
    from tests import philox_reference as pr
    return pr.fill(np.array(keys, dtype=np.uint64), list(seq), N, n_mel, kind)


def verdict(got, n_mel, N, seq, keys, kind):
    """got [B][N][n_mel] float32 -> equal to the reference (uniform: bit for bit; normal: inside NORMAL_BOUND x r), padding rows +0.0f."""
    if kind == 1:
        want = reference(n_mel, N, seq, keys, 1).astype(np.float32)
        return np.array_equal(got.view(np.uint32), want.view(np.uint32))
    z, r = reference(n_mel, N, seq, keys, 0)
    live = r > 0
    g = got.astype(np.float64)
    return bool(np.isfinite(g).all() and (np.abs(g - z)[live] <= NORMAL_BOUND * r[live]).all() and (got.view(np.uint32)[~live] == 0).all())


def cases(exe, work, reduced=False):
    """Runs every case through exe; yields (label, equal to the reference)."""
    bt, meta = H.Batch(exe, work, NAME), []
    for n_mel, N, seq, keys in CASES:
        for kind in (1, 0):
            B = len(seq)
            per_item = N * n_mel // 4
            total = per_item * B
            grid = min((total + 255) // 256, 2)
            bt.add(f"noise_fill<{kind}>", grid, 256, [H.filled((B, N, n_mel), np.float32), np.array(seq, np.int32), np.array(keys, np.uint64).reshape(-1),
                                                    N, n_mel, per_item, total])
            meta.append((n_mel, N, seq, keys, kind))
    for (n_mel, N, seq, keys, kind), out in zip(meta, bt.run()):
        yield H.check(f"noise {'uniform' if kind else 'normal'} n_mel {n_mel} N {N} seq_len {seq}", verdict(out[0], n_mel, N, seq, keys, kind))


if __name__ == "__main__":
    H.main(NAME, cases, __doc__)
