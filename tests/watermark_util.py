"""Signals and cases of the N22 tests (keyed audio watermark), shared by test_watermark_cpu.py, test_watermark_gpu.py and
tools/watermark_bench.py.  Nothing here comes from the product: the signals and the G.711 mu-law round trip are written out."""
import numpy as np

from tests.denoise_util import LENGTHS, noise, speechlike              # noqa: F401  (the seven lengths of N19: below, at and above a hop and a frame)
from tests.prosody_util import speechy                                 # noqa: F401

SR = 24000
N, H, LO, K, G, P, NB, Q = 1024, 256, 22, 320, 4, 64, 24, 256
KEY, WRONG_KEY = 0x0123456789ABCDEF, 0x0123456789ABCDEE
PAYLOADS = (0x1234, 0xBEEF)
SEEDS = (1, 2, 3)
CUT = 5 * 1024 + 128                                             # samples taken off the front: 20.5 hops
NULL_MAX = 2.0118                                                # the largest score of the null pool (profiles/watermark/notes.md)
POOL_KINDS = {"speechlike": speechlike, "speechy": speechy, "noise": noise}
POOL_SECONDS = (1, 4, 11)
POOL_SEEDS = range(16)


def frames_of(n):
    return -(-n // H) + 3


def ulaw_round_trip(x):
    """int16 -> G.711 mu-law codes -> int16, by the formulas of the recommendation (bias 33 on 14-bit magnitudes), written out here."""
    v = np.asarray(x, dtype=np.int64)
    sign = v < 0
    mag = np.minimum(np.where(sign, -v, v) >> 2, 8158) + 33       # 14-bit magnitude, biased
    seg = np.floor(np.log2(mag)).astype(np.int64) - 5             # 0 ... 7
    quant = (mag >> (seg + 1)) & 0xF
    lin = (((quant << 1) | 33) << seg) - 33                       # the decoder's midpoint, 14 bits
    return (np.where(sign, -lin, lin) * 4).astype(np.int16)


def ulaw_decode(codes):
    """G.711 mu-law codes (uint8) -> int16, written out."""
    c = ~np.asarray(codes, dtype=np.uint8)
    seg, quant = ((c >> 4) & 7).astype(np.int64), (c & 0xF).astype(np.int64)
    lin = (((quant << 1) | 33) << seg) - 33
    return (np.where(c & 0x80, -lin, lin) * 4).astype(np.int16)


def naive_stats(cells, chips):
    """The statistic by the definition, cell by cell (slow: small inputs only) -> int64 [256][24][2]."""
    d, c = np.asarray(cells, dtype=np.int64), np.asarray(chips, dtype=np.int64)
    out = np.zeros((Q, NB, 2), np.int64)
    for q in range(Q):
        for f in range(d.shape[0]):
            g = ((f + q) // G) % P
            for kk in range(K):
                j = (kk + 7 * g) % NB
                out[q, j, 0] += c[g, kk] * d[f, kk]
                out[q, j, 1] += d[f, kk] * d[f, kk]
    return out


def null_pool():
    """The pool the threshold is measured on: (name, unmarked int16 signal) for every kind, length and seed."""
    for kind, make in POOL_KINDS.items():
        for secs in POOL_SECONDS:
            for seed in POOL_SEEDS:
                yield f"{kind}-{secs}s-{seed}", make(secs * SR, seed)
