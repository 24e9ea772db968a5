"""Helpers of the FLAC tests (tests/test_flac_cpu.py, tests/test_flac_gpu.py): a stand-alone decoder written from the format (RFC 9639)
in plain loops and Python integers, which shares no code and no table with the encoder's mirror in core/audio_processor.py, a slow and
obvious reference of the subframe sizes for brute-force checks, and the seeded signals both test files run on."""
import numpy as np

BLOCK = 4096
RATES = {1: 88200, 2: 176400, 3: 192000, 4: 8000, 5: 16000, 6: 22050, 7: 24000, 8: 32000, 9: 44100, 10: 48000, 11: 96000}
BLOCK_SIZES = {1: 192, 2: 576, 3: 1152, 4: 2304, 5: 4608, 8: 256, 9: 512, 10: 1024, 11: 2048, 12: 4096, 13: 8192, 14: 16384, 15: 32768}


def crc_bits(data, poly, width):
    """CRC by shifting one message bit at a time through a ``width``-bit register: initial value 0, no reflection, no final XOR."""
    reg, top, mask = 0, 1 << (width - 1), (1 << width) - 1
    for byte in bytes(data):
        for i in range(7, -1, -1):
            fed = ((reg & top) != 0) != (((byte >> i) & 1) != 0)
            reg = (reg << 1) & mask
            if fed:
                reg ^= poly
    return reg


class Bits:
    def __init__(self, data, pos=0):
        self.data, self.pos = bytes(data), pos * 8

    def read(self, n):
        """The next n bits as an unsigned number, most significant bit first."""
        end = self.pos + n
        if end > 8 * len(self.data):
            raise ValueError("the stream ends inside a frame")
        last = (end + 7) >> 3
        v = (int.from_bytes(self.data[self.pos >> 3: last], "big") >> (8 * last - end)) & ((1 << n) - 1)
        self.pos = end
        return v

    def signed(self, n):
        v = self.read(n)
        return v - (1 << n) if v >> (n - 1) else v

    def unary(self):
        q = 0
        while self.read(1) == 0:
            q += 1
        return q


def _coded_number(b):
    first = b.read(8)
    if first < 0x80:
        return first
    n = 0
    while first & (0x80 >> n):
        n += 1
    assert 2 <= n <= 7, "bad lead byte of the coded number"
    v = first & (0x7F >> n)
    for _ in range(n - 1):
        c = b.read(8)
        assert c >> 6 == 2, "bad continuation byte of the coded number"
        v = (v << 6) | (c & 0x3F)
    return v


def _subframe(b, m, bps):
    assert b.read(1) == 0, "subframe padding bit"
    kind = b.read(6)
    assert b.read(1) == 0, "wasted bits are never flagged by this encoder"
    if kind == 0:
        return [b.signed(bps)] * m, ("constant", 0, 0, [])
    if kind == 1:
        return [b.signed(bps) for _ in range(m)], ("verbatim", 0, 0, [])
    assert 8 <= kind <= 12, f"subframe type {kind:06b}"
    o = kind - 8
    out = [b.signed(bps) for _ in range(o)]
    method = b.read(2)
    assert method in (0, 1), "reserved residual coding method"
    width, escape = (4, 15) if method == 0 else (5, 31)
    po = b.read(4)
    assert m % (1 << po) == 0 and (m >> po) >= o, "partition order does not fit the block"
    ks, res = [], []
    for p in range(1 << po):
        k = b.read(width)
        count = (m >> po) - (o if p == 0 else 0)
        if k == escape:
            raw = b.read(5)
            res += [b.signed(raw) if raw else 0 for _ in range(count)]
            ks.append(("escape", raw))
            continue
        ks.append(k)
        for _ in range(count):
            q = b.unary()
            u = (q << k) | (b.read(k) if k else 0)
            res.append(u >> 1 if u % 2 == 0 else -((u + 1) >> 1))
    coeff = {0: [], 1: [1], 2: [2, -1], 3: [3, -3, 1], 4: [4, -6, 4, -1]}[o]
    for r in res:
        out.append(r + sum(c * out[-1 - j] for j, c in enumerate(coeff)))
    return out, ("fixed", o, po, ks)


def decode_frames(data, sample_rate=None, first_number=None):
    """Frames back to back until the data ends exactly: -> (samples int16, [(type, order, po, ks, bytes)], [frame numbers])."""
    data = bytes(data)
    pos, samples, frames, numbers = 0, [], [], []
    while pos < len(data):
        b = Bits(data, pos)
        assert b.read(14) == 0x3FFE, f"no sync code at byte {pos}"
        assert b.read(1) == 0, "reserved bit after the sync code"
        assert b.read(1) == 0, "fixed block size stream expected"
        bs_code, sr_code = b.read(4), b.read(4)
        assert b.read(4) == 0, "one channel expected"
        assert b.read(3) == 4, "16 bits per sample expected"
        assert b.read(1) == 0, "reserved bit of the frame header"
        number = _coded_number(b)
        if bs_code == 6:
            m = b.read(8) + 1
        elif bs_code == 7:
            m = b.read(16) + 1
        else:
            assert bs_code in BLOCK_SIZES, "reserved block size code"
            m = BLOCK_SIZES[bs_code]
        if sr_code == 12:
            rate = b.read(8) * 1000
        elif sr_code == 13:
            rate = b.read(16)
        elif sr_code == 14:
            rate = b.read(16) * 10
        else:
            assert sr_code != 15, "invalid rate code"
            rate = RATES.get(sr_code)                     # 0 = taken from the stream header
        if sample_rate is not None and rate is not None:
            assert rate == sample_rate, (rate, sample_rate)
        assert b.pos % 8 == 0
        head_end = b.pos // 8
        assert b.read(8) == crc_bits(data[pos:head_end], 0x07, 8), "CRC-8 of the frame header"
        block, what = _subframe(b, m, 16)
        pad = (-b.pos) % 8
        assert b.read(pad) == 0 if pad else True, "padding bits are zero"
        body_end = b.pos // 8
        assert b.read(16) == crc_bits(data[pos:body_end], 0x8005, 16), "CRC-16 of the frame"
        assert all(-32768 <= v <= 32767 for v in block), "a decoded sample leaves 16 bits"
        samples += block
        numbers.append(number)
        frames.append(what + (body_end + 2 - pos,))
        pos = body_end + 2
    if first_number is not None:
        assert numbers == list(range(first_number, first_number + len(numbers))), numbers
    return np.array(samples, dtype=np.int16), frames, numbers


def stream_header(data):
    """``fLaC`` and the metadata blocks: -> (the STREAMINFO fields, the byte at which the frames start)."""
    data = bytes(data)
    assert data[:4] == b"fLaC", "stream marker"
    pos, info = 4, None
    while True:
        last, kind = data[pos] >> 7, data[pos] & 0x7F
        size = int.from_bytes(data[pos + 1: pos + 4], "big")
        body = data[pos + 4: pos + 4 + size]
        assert len(body) == size
        if kind == 0:
            assert size == 34 and info is None and pos == 4, "STREAMINFO comes first, once, with 34 bytes"
            v = int.from_bytes(body[10:18], "big")
            info = dict(min_block=int.from_bytes(body[0:2], "big"), max_block=int.from_bytes(body[2:4], "big"),
                        min_frame=int.from_bytes(body[4:7], "big"), max_frame=int.from_bytes(body[7:10], "big"), rate=v >> 44,
                        channels=((v >> 41) & 7) + 1, bits=((v >> 36) & 31) + 1, total=v & ((1 << 36) - 1), md5=body[18:34])
        pos += 4 + size
        if last:
            break
    assert info is not None and info["channels"] == 1 and info["bits"] == 16 and info["min_block"] == info["max_block"] == BLOCK
    return info, pos


def decode_stream(data, first_number=0):
    """A complete stream: ``fLaC``, the metadata blocks, frames to the very end.  -> (samples, frames, info) with info = the STREAMINFO
    fields.  Checks what the header promises against what the frames hold."""
    data = bytes(data)
    info, pos = stream_header(data)
    samples, frames, numbers = decode_frames(data[pos:], info["rate"], first_number)
    sizes = [f[4] for f in frames]
    if info["total"]:
        assert info["total"] == samples.size, (info["total"], samples.size)
    if info["min_frame"]:
        assert info["min_frame"] == min(sizes)
    if info["max_frame"]:
        assert info["max_frame"] == max(sizes)
    assert all(f[4] for f in frames)
    assert not frames or BLOCK * (len(frames) - 1) < samples.size <= BLOCK * len(frames)      # only the last frame may be short
    return samples, frames, info


# ------------------------------------------------------------------ the sizes, slowly
def zigzag(r):
    return 2 * r if r >= 0 else -2 * r - 1


def rice_bits(residuals, k):
    """The bits of the residuals under parameter k, counted code by code."""
    total = 0
    for r in residuals:
        total += (zigzag(r) >> k) + 1 + k
    return total


def differences(x, o):
    x = [int(v) for v in x]
    for _ in range(o):
        x = [b - a for a, b in zip(x, x[1:])]
    return x


def fixed_bits(x, o, po, ks=None):
    """Size of the Fixed(o, po) subframe of the samples x: with the given parameters, or (ks None) the best k of each partition and the
    lowest such k.  -> (bits, ks); None if (o, po) is not a candidate."""
    m = len(x)
    if o > min(4, m - 1) or m % (1 << po) or (m >> po) <= o:
        return None
    res, ps = differences(x, o), m >> po
    bits, chosen, at = 8 + 16 * o + 2 + 4, [], 0
    for p in range(1 << po):
        count = ps - (o if p == 0 else 0)
        part = res[at: at + count]
        at += count
        if ks is None:
            sizes = [rice_bits(part, k) for k in range(15)]
            k = sizes.index(min(sizes))
        else:
            k = ks[p]
        chosen.append(k)
        bits += 4 + rice_bits(part, k)
    assert at == len(res)
    return bits, chosen


def best_subframe(x):
    """The issue's rule by brute force: -> (type, o, po, ks, bits)."""
    x = [int(v) for v in x]
    m = len(x)
    if all(v == x[0] for v in x):
        return ("constant", 0, 0, [], 24)
    best = None
    for o in range(5):
        for po in range(5):
            got = fixed_bits(x, o, po)
            if got is not None and (best is None or got[0] < best[4]):      # ascending o, then po: the first of equals stays
                best = ("fixed", o, po, got[1], got[0])
    if 8 + 16 * m < best[4]:
        return ("verbatim", 0, 0, [], 8 + 16 * m)
    return best


# ------------------------------------------------------------------ the signals (seeded)
LENGTHS = (1, 2, 5, 15, 16, 17, 4095, 4096, 4097, 4096 + 5, 4096 + 24, 4096 + 256, 2 * 4096, 3 * 4096 + 1000)


def _switching(rng, n, period):
    t = np.arange(n)
    loud = (t // period) % 2 == 1
    return np.where(loud, rng.integers(-20000, 20001, n), rng.integers(-3, 4, n)).astype(np.int16)


def signals(n=BLOCK):
    """name -> int16 signal of n samples; the dictionary's order is fixed."""
    rng = np.random.default_rng(20240)
    t = np.arange(n)
    out = {
        "zeros": np.zeros(n, np.int16),
        "floor": np.full(n, -32768, np.int16),
        "noise8": rng.integers(-8, 9, n).astype(np.int16),
        "walk20": np.cumsum(rng.integers(-20, 21, n)).astype(np.int16),
        "ramp": (3 * t - 6000).astype(np.int16),
        "sine200": np.rint(12000 * np.sin(2 * np.pi * 200 * t / 24000)).astype(np.int16),
        "sine1k": np.rint(12000 * np.sin(2 * np.pi * 1000 * t / 24000)).astype(np.int16),
        "fullnoise": rng.integers(-32768, 32768, n).astype(np.int16),
        "alternating": np.where(t % 2 == 0, 32767, -32768).astype(np.int16),
        "switch2048": _switching(rng, n, 2048),
        "switch1024": _switching(rng, n, 1024),
        "switch512": _switching(rng, n, 512),
        "switch256": _switching(rng, n, 256),
    }
    return out


def speechlike(n, seed=5, sr=24000):
    """A seeded voiced-speech stand-in: a harmonic series with a wandering pitch under a slow envelope, plus a little noise."""
    rng = np.random.default_rng(seed)
    t = np.arange(n) / sr
    f0 = 120 + 30 * np.sin(2 * np.pi * 0.7 * t) + 10 * np.sin(2 * np.pi * 2.3 * t)
    phase = 2 * np.pi * np.cumsum(f0) / sr
    x = sum(np.sin(h * phase) / h for h in range(1, 12))
    env = 0.55 + 0.45 * np.sin(2 * np.pi * 1.7 * t + 1.0)
    x = 6000 * env * x + rng.normal(0, 40, n)
    return np.clip(np.rint(x), -32768, 32767).astype(np.int16)


# frames whose best Fixed subframe has EXACTLY the size of the verbatim one (8 + 16 m bits): verbatim needs to be strictly smaller, so
# they stay Fixed(0, 0).  Found once by a seeded search over full-scale noise; hard-coded so that the case cannot silently go missing
VERBATIM_TIES = (
    [9160, -1061, 5546, -10258, 1518, -1586, 6362, -19564, 1232, -24476, 11307, -7183, 810, -8156, 2482, -14992],
    [1996, 9177, 18996, -19471, -552, -2460, -5401, -1061, 16259, -3754, 18668, 756, -2130, 13809, 13885, 917, -606],
    [9891, -6122, -4415, 12210, 3690, 9254, -12557, 10477, -7079, -768, 12443, 8153, 14943, -7835, 7096, 14617, -6573, 11517, -18826, 17685,
     7506, 10622, 9296, 9133, -6619, -12421, -4566, 2770, -5884, -16970, -12578, 16683],
)


def device_cases():
    """[(name, pcm, frame0, last)]: the rows of the device tests -- every signal as one frame, short and long signals, frame numbers of
    every coded length, one block of a stream (last = 0)."""
    big = signals(3 * BLOCK + 1000)
    rng = np.random.default_rng(77)
    cases = [(name, x, 0, 1) for name, x in signals().items()]
    cases += [
        ("speech_13288", speechlike(3 * BLOCK + 1000), 0, 1),
        ("walk_4097", big["walk20"][: BLOCK + 1], 127, 1),
        ("sine_4101", big["sine200"][: BLOCK + 5], 2047, 1),
        ("switch_4120", big["switch256"][: BLOCK + 24], 2048, 1),
        ("sine1k_4352", big["sine1k"][: BLOCK + 256], 65535, 1),
        ("one", np.array([-5], np.int16), 128, 1),
        ("two", np.array([7, -9], np.int16), 0, 1),
        ("five", big["walk20"][100:105], 3, 1),
        ("noise_15", rng.integers(-3000, 3000, 15).astype(np.int16), 0, 1),
        ("noise_16", rng.integers(-300, 300, 16).astype(np.int16), 0, 1),
        ("noise_17", rng.integers(-30, 30, 17).astype(np.int16), (1 << 31) - 2, 1),
        ("speech_4095", speechlike(BLOCK - 1, 9), 1, 1),
        ("stream_block", big["switch512"][: 2 * BLOCK], 65536, 0),
        ("stream_tail", big["ramp"][: 1000], 65538, 1),
    ]
    cases += [(f"verbatim_tie_{len(y)}", np.array(y, np.int16), 5 + i, 1) for i, y in enumerate(VERBATIM_TIES)]
    return cases


def mirror_layout(cases, rate):
    """What one vv_pcm_flac call over ``cases`` must give: -> (bytes, info (R + 1) x 3, the sum of the frame bounds)."""
    from vietvoice_tts_amd.core.audio_processor import flac_encode_frames, flac_frame_bound
    parts, info, at, bound = [], [], 0, 0
    for _name, x, frame0, last in cases:
        data, lo, hi = flac_encode_frames(x, rate, frame0, bool(last))
        info.append([at, lo, hi])
        parts.append(data)
        at += data.size
        full = x.size // BLOCK
        bound += full * flac_frame_bound(BLOCK) + flac_frame_bound(x.size - full * BLOCK)
    info.append([at, 0, 0])
    return np.concatenate(parts), np.array(info, np.int64), bound
