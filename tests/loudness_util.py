"""Shared helpers of the loudness tests (tests/test_loudness_cpu.py, tests/test_loudness_gpu.py): an INDEPENDENT reference of DESIGN §8 N12.

The reference filters the whole signal sequentially with scipy.signal.lfilter: the same filter structure as the product (direct form II
transposed), but one pass over the whole signal with no run decomposition, no tables and no second pass -- that is where it is
independent.  Its block sums, gates and gain are written here from the Recommendation's text, apart from the product code."""
import numpy as np

TABLE_48K = {                                   # ITU-R BS.1770-4, table 1 and table 2 (48 kHz)
    "shelf_b": [1.53512485958697, -2.69169618940638, 1.19839281085285],
    "shelf_a": [-1.69065929318241, 0.73248077421585],
    "hp_b": [1.0, -2.0, 1.0],
    "hp_a": [-1.99004745483398, 0.99007225036621],
}
ABS_LUFS, REL_LU = -70.0, -10.0


def ref_coefficients(sr):
    """The two K-weighting biquads at ``sr`` from the analogue prototypes (bilinear transform with pre-warped corner), as (b, a) pairs."""
    def proto(f0, Q, shelf_db=None):
        K = np.tan(np.pi * f0 / sr)
        a0 = 1 + K / Q + K * K
        a = np.array([1.0, 2 * (K * K - 1) / a0, (1 - K / Q + K * K) / a0])
        if shelf_db is None:
            return np.array([1.0, -2.0, 1.0]), a
        Vh = 10 ** (shelf_db / 20)
        Vb = Vh ** 0.4996667741545416
        return np.array([(Vh + Vb * K / Q + K * K) / a0, 2 * (K * K - Vh) / a0, (Vh - Vb * K / Q + K * K) / a0]), a
    return proto(1681.974450955533, 0.7071752369554196, 3.999843853973347), proto(38.13547087602444, 0.5003270373238773)


def ref_subblock_sums(x, sr):
    """Sum of the squared K-weighted signal over each complete 100 ms of int16 ``x``; only the complete sub-blocks are filtered."""
    from scipy.signal import lfilter
    sub = sr // 10
    J = len(x) // sub
    if J == 0:
        return np.zeros(0)
    (b1, a1), (b2, a2) = ref_coefficients(sr)
    y = lfilter(b2, a2, lfilter(b1, a1, np.asarray(x[: J * sub], np.float64) / 32768.0))
    return (y * y).reshape(J, sub).sum(axis=1)


def ref_blocks(q, sub):
    """Mean square of every 400 ms block (75 % overlap) from the 100 ms sums."""
    q = np.asarray(q, np.float64)
    if q.size < 4:
        return np.zeros(0)
    return np.array([q[j: j + 4].sum() for j in range(q.size - 3)]) / (4 * sub)


def ref_gate(z):
    """-> (zbar, kept mask, thresholds (absolute, relative) in the linear domain); zbar = 0 with nothing kept."""
    z = np.asarray(z, np.float64)
    t_abs = 10 ** ((ABS_LUFS + 0.691) / 10)
    above = z > t_abs
    if not above.any():
        return 0.0, above, (t_abs, None)
    t_rel = z[above].mean() * 10 ** (REL_LU / 10)
    keep = above & (z > t_rel)
    return (float(z[keep].mean()) if keep.any() else 0.0), keep, (t_abs, t_rel)


def ref_measure(x, sr):
    """-> dict(q, z, zbar, keep, thresholds, kept, peak, lufs) of int16 ``x``."""
    x = np.asarray(x)
    q = ref_subblock_sums(x, sr)
    z = ref_blocks(q, sr // 10)
    zbar, keep, thr = ref_gate(z)
    kept = int(keep.sum())
    return {"q": q, "z": z, "zbar": zbar, "keep": keep, "thresholds": thr, "kept": kept,
            "peak": int(np.abs(x.astype(np.int64)).max(initial=0)), "lufs": -0.691 + 10 * np.log10(zbar) if kept else float("-inf")}


def ref_gain(m, target, peak_dbfs):
    """-> (gain, ceiling-limited?) from ref_measure's dict; target None = measure only."""
    if target is None or m["kept"] == 0 or m["peak"] == 0:
        return 1.0, False
    g = np.sqrt(10 ** ((target + 0.691) / 10) / m["zbar"])
    c = 32767 * 10 ** (peak_dbfs / 20)
    if m["peak"] * g > c:
        return c / m["peak"], True
    return float(g), False


def ref_normalize(x, sr, target, peak_dbfs=-1.0):
    """-> (int16 result, ref_measure's dict, gain, ceiling-limited?)."""
    m = ref_measure(x, sr)
    g, limited = ref_gain(m, target, peak_dbfs)
    y = np.clip(np.rint(np.asarray(x, np.float64) * g), -32768, 32767).astype(np.int16)
    return y, m, g, limited


def threshold_margin(m):
    """Smallest relative distance of a block above the absolute gate from the relative threshold, and of any block from the absolute one."""
    t_abs, t_rel = m["thresholds"]
    z = m["z"]
    d = [np.abs(z / t_abs - 1).min()] if z.size else []
    if t_rel is not None:
        d.append(np.abs(z[z > t_abs] / t_rel - 1).min())
    return min(d) if d else float("inf")


# ---------------------------------------------------------------------------------------------- signals of the GPU cases
FREQS = (140.0, 310.0, 620.0, 997.0, 1480.0, 2350.0, 3400.0)


def speechlike(n, sr, seed, amp=6000.0):
    """Seven sinusoids (140 - 3400 Hz, amplitude ``amp`` in all) under a 0.7 Hz envelope clipped at zero; the envelope starts at its
    maximum so that the first 400 ms are loud, and long signals have quiet stretches that the relative gate drops."""
    rng = np.random.default_rng(seed)
    t = np.arange(n) / sr
    ph = rng.uniform(0, 2 * np.pi, len(FREQS))
    s = sum(np.sin(2 * np.pi * f * t + p) for f, p in zip(FREQS, ph)) / len(FREQS)
    env = (np.maximum(np.cos(2 * np.pi * 0.7 * t) + 0.95, 0.0) / 1.95) ** 3
    return np.clip(np.rint(amp * s * env), -32768, 32767).astype(np.int16)


def sine(n, sr, f=997.0, amp=32767.0):
    return np.clip(np.rint(amp * np.sin(2 * np.pi * f * np.arange(n) / sr)), -32768, 32767).astype(np.int16)
