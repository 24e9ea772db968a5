"""Signals and cases of the N19 tests (vocoder-bias denoiser), shared by test_denoise_cpu.py and test_denoise_gpu.py.  Nothing here comes
from the product: the signals are written out, and the hum-and-tone measurement uses numpy's own FFT."""
import numpy as np

N, H, BINS = 1024, 256, 513
LENGTHS = (1, 255, 256, 257, 1023, 1025, 5000)          # below, at and above a hop and a frame; many hops


def speechlike(n, seed):
    """Seeded speech-like input: a few summed sinusoids under a slow envelope, plus noise."""
    rng = np.random.default_rng(seed)
    t = np.arange(n, dtype=np.float64)
    f0 = 100.0 + 80.0 * rng.random()
    x = sum(a * np.sin(2 * np.pi * k * f0 * t / 24000.0 + p) for k, a, p in ((1, 7000.0, 0.0), (2, 4000.0, 0.7), (3.02, 2500.0, 1.9), (7, 900.0, 0.3)))
    x = x * (0.55 + 0.45 * np.sin(2 * np.pi * 2.5 * t / 24000.0 + 0.4)) + 1200.0 * rng.standard_normal(n)
    return np.clip(np.rint(x), -32768, 32767).astype(np.int16)


def noise(n, seed):
    """Random full-scale noise."""
    return np.random.default_rng(seed).integers(-32768, 32768, n).astype(np.int16)


def alternation(n):
    """+-full scale, sample by sample: the largest magnitude a bin can carry."""
    return np.where(np.arange(n) % 2 == 0, 32767, -32768).astype(np.int16)


def random_bias(seed, scale=60000.0):
    """A non-trivial positive profile: of the size of the noise floor of speechlike() under the window, so some bins clamp and others do not."""
    return np.random.default_rng(seed).random(BINS) * scale + 1.0


def hum_and_tone(n=6000):
    """The issue's case: -> (tone + hum, the rounded hum alone), int16."""
    t = np.arange(n, dtype=np.float64)
    hum = 300.0 * np.sin(2 * np.pi * 40.0 * t / 1024.0 + 0.3)
    tone = 8000.0 * np.sin(2 * np.pi * 150.37 * t / 1024.0)
    return np.rint(tone + hum).astype(np.int16), np.rint(hum).astype(np.int16)


def segment_amplitudes(x, at=2048):
    """|rfft| of the Hann-windowed 1024-sample segment at ``at`` (numpy's transform and the window written out here)."""
    w = 0.5 - 0.5 * np.cos(2.0 * np.pi * np.arange(N) / N)
    return np.abs(np.fft.rfft(w * np.asarray(x[at: at + N], dtype=np.float64)))


def frames_of(n):
    return -(-n // H) + 3
