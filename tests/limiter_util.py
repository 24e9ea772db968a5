"""Independent reference for the N13 limiter tests: the seven steps of DESIGN §8 N13 from scipy's filters, written apart from the
product code (core/audio_processor.py) -- scipy.signal.upfirdn for the 4x interpolation, scipy.ndimage.minimum_filter1d for the sliding
minimum and scipy.ndimage.correlate1d for the window average, both with mode="nearest" (= the clamp of the specification).  scipy sums
in its own order, so this reference is close to the mirror, not bit-equal: gains within 1e-12, PCM within output_util.lsb_condition."""
import numpy as np
from scipy.ndimage import correlate1d, minimum_filter1d
from scipy.signal import upfirdn

H = 12
SR = 24000


def ref_taps():
    k = np.arange(-4 * H, 4 * H + 1)
    return np.sinc(k / 4.0) * np.kaiser(8 * H + 1, 8.0)


def ref_window(L):
    k = np.arange(-L, L + 1)
    w = 0.5 * (1.0 + np.cos(np.pi * k / (L + 1)))
    return w / w.sum()


def ref_ceiling(peak_dbfs):
    return 32767.0 * 10.0 ** (peak_dbfs / 20.0)


def ref_estimate(v, mode):
    """e[i]: |v[i]|, or the largest magnitude of the four 4x-interpolated points i, i + 1/4, i + 2/4, i + 3/4."""
    v = np.asarray(v, np.float64)
    if mode == "sample" or v.size == 0:
        return np.abs(v)
    up = upfirdn(ref_taps(), v, up=4)                     # up[4H + 4i + p] = the point i + p / 4
    pts = up[4 * H: 4 * H + 4 * v.size].reshape(v.size, 4)
    return np.abs(pts).max(axis=1)


def ref_gains(x, c, mode, gain=1.0, L=120):
    """-> (v, e, s) of the whole signal."""
    v = np.asarray(x, np.float64) * gain
    e = ref_estimate(v, mode)
    if v.size == 0:
        return v, e, np.ones(0)
    r = np.where(e > c, c / np.maximum(e, 1e-300), 1.0)
    m = minimum_filter1d(r, size=2 * L + 1, mode="nearest")
    A = correlate1d(1.0 - m, ref_window(L), mode="nearest")
    return v, e, np.minimum(1.0 - A, r)


def ref_limit(x, peak_dbfs, mode, gain=1.0, L=120):
    v, _e, s = ref_gains(x, ref_ceiling(peak_dbfs), mode, gain, L)
    return np.clip(np.rint(v * s), -32768, 32767).astype(np.int16)


def sine(n, f, amp=30000.0, phase=0.0, sr=SR):
    return np.rint(amp * np.sin(2 * np.pi * f * np.arange(n) / sr + phase)).astype(np.int16)


def noisy(n, seed, scale=6000.0):
    """Band-limited-ish noise with a slow envelope, a few bursts: some stretches reach a -1 dBFS ceiling at gain 1.7, others never."""
    rng = np.random.default_rng(seed)
    x = rng.standard_normal(n)
    if n > 4:
        x = np.convolve(x, [0.25, 0.5, 0.25], mode="same")
    env = 0.35 + 0.65 * np.abs(np.sin(np.arange(n) * (2 * np.pi / 4099.0) + seed))
    return np.clip(np.rint(x * env * scale * 1.6), -32768, 32767).astype(np.int16)


def with_full_scale(x):
    """Full-scale samples at 0, n / 3 and n - 1."""
    x = x.copy()
    if x.size:
        x[0], x[x.size // 3], x[-1] = 32767, -32768, 32767
    return x
