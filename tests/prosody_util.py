"""Helpers of the prosody tests: an independent WSOLA reference in plain loops and Python integers, written from the
specification and apart from core/audio_processor.py, and the test signals."""
import math
from operator import mul

import numpy as np

N, HS, D = 512, 256, 128
LENGTHS = (0, 1, 255, 256, 257, 511, 512, 513, 767, 768, 1000, 5003)
RATIOS = ((3, 2), (2, 3), (25, 21), (23, 29), (32, 31), (2, 1), (1, 2))


def ref_window():
    return [0.5 - 0.5 * math.cos(2.0 * math.pi * k / N) for k in range(N)]


def ref_stretch(x, p, q):
    """-> (list of output samples, list of pos_0 ... pos_M).  x: a sequence of ints in the int16 range."""
    xs = [int(v) for v in x]
    n = len(xs)

    def at(i):
        return xs[i] if 0 <= i < n else 0

    n_s = (n * p + q - 1) // q
    M = (n_s + HS - 1) // HS
    pos = [-HS]
    for m in range(1, M + 1):
        a = ((m - 1) * HS * q) // p
        t = [at(pos[m - 1] + HS + k) for k in range(N)]
        span = [at(a - D + k) for k in range(N + 2 * D)]
        best_c, best_d = None, None
        for d in range(-D, D):
            c = sum(map(mul, t, span[d + D: d + D + N]))
            better = best_c is None or c > best_c
            if not better and c == best_c:          # among equals: the smaller |delta|, the negative one first
                better = abs(d) < abs(best_d) or (abs(d) == abs(best_d) and d < best_d)
            if better:
                best_c, best_d = c, d
        pos.append(a + best_d)
    w = ref_window()
    out = []
    for i in range(n_s):
        m = i // HS + 1
        k = i - (m - 1) * HS
        v = w[k + HS] * float(at(pos[m - 1] + k + HS)) + w[k] * float(at(pos[m] + k))
        r = round(v)                                # Python's round: ties to even
        out.append(max(-32768, min(32767, r)))
    return out, pos


def speechy(n, seed):
    """Something between noise and a voiced sound, int16, full of sign changes and a few full-scale samples."""
    rng = np.random.default_rng(seed)
    t = np.arange(n, dtype=np.float64)
    f0 = 90.0 + 60.0 * rng.random()
    x = 9000.0 * np.sin(2 * np.pi * f0 * t / 24000.0) + 5000.0 * np.sin(2 * np.pi * 3.1 * f0 * t / 24000.0 + 1.0)
    x = x * (0.6 + 0.4 * np.sin(2 * np.pi * 3.0 * t / 24000.0)) + 1500.0 * rng.standard_normal(n)
    x = np.clip(np.rint(x), -32768, 32767).astype(np.int16)
    if n > 8:
        x[rng.integers(0, n, 3)] = (-32768, 32767, -32768)
    return x


def pulse_train(n=24000, period=240, f=700.0, sr=24000):
    """A 100 Hz train of decaying 700 Hz pulses: period 240 samples."""
    k = np.arange(period, dtype=np.float64)
    one = 12000.0 * np.exp(-k / 40.0) * np.sin(2 * np.pi * f * k / sr)
    return np.rint(np.tile(one, n // period + 1)[:n]).astype(np.int16)


def sine(f, n=24000, amp=12000.0, sr=24000):
    return np.rint(amp * np.sin(2 * np.pi * f * np.arange(n, dtype=np.float64) / sr)).astype(np.int16)


def autocorr_peak(y, lo=120, hi=480):
    """The lag in [lo, hi) with the largest autocorrelation of the middle of y."""
    v = np.asarray(y, np.float64)
    v = v[len(v) // 8: len(v) - len(v) // 8]
    r = [float(np.dot(v[:-lag], v[lag:])) for lag in range(lo, hi)]
    return lo + int(np.argmax(r))


def spectrum_peak(y, sr=24000):
    """(peak frequency on a 1 Hz grid, share of the Hann-windowed energy within +-3 bins of it) of the middle ``sr`` samples of y
    (zero padded when shorter)."""
    v = np.asarray(y, np.float64)
    if v.size > sr:
        lo = (v.size - sr) // 2
        v = v[lo: lo + sr]
    v = v * np.hanning(v.size)
    P = np.abs(np.fft.rfft(v, sr)) ** 2
    k = int(np.argmax(P))
    return float(k), float(P[max(k - 3, 0): k + 4].sum() / P.sum())


def full_scale(n, kind):
    """The largest sums the search can meet: every sample -32768, or +32767 / -32768 in runs of 37 (a period inside the search radius)."""
    if kind == "dc":
        return np.full(n, -32768, np.int16)
    return np.where((np.arange(n) // 37) % 2 == 0, 32767, -32768).astype(np.int16)


def stretch_cases():
    """[(name, int16 signal, p, q)]: every length under every ratio and two full-scale signals, what the device test and
    tools/prosody_host_check.py run in ONE launch."""
    cases = [(f"len{n}_{p}over{q}", speechy(n, 1000 + 16 * i + j), p, q) for i, n in enumerate(LENGTHS) for j, (p, q) in enumerate(RATIOS)]
    return cases + [("full_scale_dc", full_scale(1500, "dc"), 3, 2), ("full_scale_square", full_scale(1500, "square"), 2, 3)]
