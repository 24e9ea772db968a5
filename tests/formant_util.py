"""Helpers of the formant tests: the synthetic vowel, an envelope estimate that shares nothing with the code under
test (a cepstrally smoothed log spectrum), the fundamental by autocorrelation, and the signals and cases of the device tests."""
import numpy as np

SR = 24000
F0 = 110.0
RESONANCES = ((500.0, 80.0), (1500.0, 100.0), (2500.0, 120.0))       # (centre, bandwidth) in Hz
P, NA, H, L = 24, 1024, 256, 2048
MEANING_CASES = ((4, None), (-4, None), (3, 1.25), (-3, 0.75))        # (pitch in semitones, tempo)


def vowel(f0=F0, seconds=1.0, sr=SR, peak=12000.0):
    """An impulse train at f0 through three two-pole resonances in cascade, int16."""
    n = int(round(seconds * sr))
    v = np.zeros(n, np.float64)
    v[np.unique(np.floor(np.arange(0.0, n, sr / f0)).astype(np.int64))] = 1.0
    for fc, bw in RESONANCES:
        r = np.exp(-np.pi * bw / sr)
        a1, a2 = -2.0 * r * np.cos(2.0 * np.pi * fc / sr), r * r
        out = np.zeros(n, np.float64)
        for i in range(n):
            out[i] = v[i] - a1 * (out[i - 1] if i >= 1 else 0.0) - a2 * (out[i - 2] if i >= 2 else 0.0)
        v = out
    return np.rint(v * (peak / np.abs(v).max())).astype(np.int16)


def envelope(sig, f0, sr=SR, nfft=16384):
    """The log-magnitude spectrum of the middle of ``sig`` smoothed in the cepstrum: quefrencies at and above 0.6 pitch periods are
    removed, so the harmonics of f0 are gone and the resonances stay.  -> (frequencies, envelope in nepers)."""
    v = np.asarray(sig, np.float64)
    m = min(v.size, nfft)
    lo = (v.size - m) // 2
    seg = v[lo: lo + m] * np.hanning(m)
    logmag = np.log(np.abs(np.fft.rfft(seg, nfft)) + 1e-9)
    cep = np.fft.irfft(logmag, nfft)
    cut = int(0.6 * sr / f0)
    lift = np.zeros(nfft)
    lift[:cut] = 1.0
    lift[nfft - cut + 1:] = 1.0
    return np.fft.rfftfreq(nfft, 1.0 / sr), np.fft.rfft(cep * lift, nfft).real


def peak_in(freqs, env, lo, hi):
    """The frequency of the envelope's highest local maximum in [lo, hi] Hz (the skirt of a neighbouring resonance at the band's edge is
    no peak); the largest value where the band holds none."""
    sel = np.nonzero((freqs >= lo) & (freqs <= hi))[0]
    tops = [i for i in sel if 0 < i < env.size - 1 and env[i - 1] < env[i] >= env[i + 1]]
    best = max(tops, key=lambda i: env[i]) if tops else sel[np.argmax(env[sel])]
    return float(freqs[best])


def resonance(sig, f0, near, ratio, sr=SR):
    """Where the resonance the source has at ``near`` Hz lies in ``sig``: the envelope's peak in the band that holds both candidates,
    ``near`` and ``near * ratio``, with a sixth of an octave on either side."""
    freqs, env = envelope(sig, f0, sr)
    lo, hi = min(near, near * ratio), max(near, near * ratio)
    return peak_in(freqs, env, lo / 2.0 ** (1 / 6), hi * 2.0 ** (1 / 6))


def fundamental(sig, sr=SR, lo=60.0, hi=400.0):
    """f0 as the autocorrelation peak of the middle of ``sig``, over lags of sr / hi ... sr / lo samples, refined by a parabola."""
    v = np.asarray(sig, np.float64)
    v = v[v.size // 8: v.size - v.size // 8]
    spec = np.abs(np.fft.rfft(v, 2 * v.size)) ** 2
    r = np.fft.irfft(spec)[: v.size]
    a, b = int(sr / hi), int(sr / lo)
    k = a + int(np.argmax(r[a: b]))
    d = 0.5 * (r[k - 1] - r[k + 1]) / (r[k - 1] - 2.0 * r[k] + r[k + 1])
    return sr / (k + d)


def closer_in_log(value, a, b):
    """value lies closer to a than to b, in log frequency."""
    return abs(np.log(value / a)) < abs(np.log(value / b))


def rms(sig):
    return float(np.sqrt(np.mean(np.asarray(sig, np.float64) ** 2)))


# ------------------------------------------------------------------ the device tests' signals
def speechy(n, seed):
    """The seeded speech stand-in of the FLAC tests' kind: a voiced sound with noise, sign changes and a few full-scale samples."""
    from tests.prosody_util import speechy as make
    return make(n, seed)


def signal(kind, n, seed=0):
    if kind == "speech":
        return speechy(n, 4000 + seed)
    if kind == "silence_then_signal":          # flat frames next to live ones
        x = speechy(n, 4100 + seed)
        x[: (2 * n) // 5] = 0
        return x
    if kind == "square":                       # +-32767 in runs of 23: the filter's output saturates
        return np.where((np.arange(n) // 23) % 2 == 0, 32767, -32767).astype(np.int16)
    if kind == "constant":
        return np.full(n, 1234, np.int16)
    if kind == "zeros":
        return np.zeros(n, np.int16)
    raise ValueError(kind)


# (name, kind, n, pitch, tempo): every length, every pitch, every tempo and every content at least once -- a cross, not the product
DEVICE_CASES = (
    ("len0", "speech", 0, 4, None), ("len1", "speech", 1, -4, None), ("len255", "speech", 255, 12, None), ("len256", "speech", 256, -12, None),
    ("len257", "speech", 257, 4, 1.25), ("len700", "speech", 700, -4, 0.75), ("len1500", "speech", 1500, 12, 0.75),
    ("len5000", "speech", 5000, -12, 1.25), ("len5000_up", "speech", 5000, 4, None), ("quiet_start", "silence_then_signal", 5000, -4, None),
    ("quiet_start_fast", "silence_then_signal", 1500, 4, 1.25), ("square", "square", 1500, 4, None), ("square_down", "square", 700, -12, 0.75),
    ("constant", "constant", 1500, -4, None), ("zeros", "zeros", 700, 4, 1.25),
)

# one sample less than, equal to and one more than an analysis frame of NA samples, in x (and at no tempo in y), and in y alone
FRAME_EDGE_CASES = (
    ("len1023", "speech", 1023, 4, None), ("len1024", "speech", 1024, -4, None), ("len1025", "speech", 1025, 12, None),
    ("y1023", "speech", 767, 4, 0.75), ("y1024", "speech", 1280, -4, 1.25), ("y1025", "silence_then_signal", 1281, -12, 1.25),
)


def device_case(name, kind, n, pitch, tempo):
    """One case as the device call takes it, with the mirror's results: x, y = shift_prosody's result, tn / td, z, h, flat."""
    from vietvoice_tts_amd.core.audio_processor import (apply_formant_filters, formant_filters, prosody_plan, prosody_tempo, shift_prosody)
    x = signal(kind, n, seed=len(name))
    y = shift_prosody(x, pitch, tempo)
    tn, td = prosody_tempo(prosody_plan(n, pitch, tempo))
    h, flat = formant_filters(x, y, tn, td)
    return dict(name=name, x=x, y=y, tn=tn, td=td, z=apply_formant_filters(y, h), h=h, flat=flat)
