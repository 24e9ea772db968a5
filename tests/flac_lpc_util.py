"""Helpers of the LPC tests of the FLAC output (tests/test_flac_lpc_cpu.py, tests/test_flac_lpc_gpu.py): a decoder that reads
LPC subframes (types 32 ... 63) as well, written from the format (RFC 9639) in plain loops and Python integers -- precision, shift and
coefficients come from the stream, nothing from the encoder's mirror --, a slow reference of a subframe's size, and the rows of the
device tests.  The bit reader, the CRC and the seeded signals are those of tests/flac_util.py."""
import numpy as np

from tests.flac_util import BLOCK, BLOCK_SIZES, RATES, Bits, crc_bits, device_cases, rice_bits, signals


def _residual(b, m, order):
    """The residual section: -> (residuals, po, ks)."""
    method = b.read(2)
    assert method in (0, 1), "reserved residual coding method"
    width, escape = (4, 15) if method == 0 else (5, 31)
    po = b.read(4)
    assert m % (1 << po) == 0 and (m >> po) >= order, "partition order does not fit the block"
    ks, res = [], []
    for p in range(1 << po):
        k = b.read(width)
        assert k != escape, "the escape code is never written by this encoder"
        ks.append(k)
        for _ in range((m >> po) - (order if p == 0 else 0)):
            u = (b.unary() << k) | (b.read(k) if k else 0)
            res.append(u >> 1 if u % 2 == 0 else -((u + 1) >> 1))
    return res, po, ks


def _subframe(b, m, bps):
    assert b.read(1) == 0, "subframe padding bit"
    kind = b.read(6)
    assert b.read(1) == 0, "wasted bits are never flagged by this encoder"
    if kind == 0:
        return [b.signed(bps)] * m, ("constant", 0, 0, [])
    if kind == 1:
        return [b.signed(bps) for _ in range(m)], ("verbatim", 0, 0, [])
    if 8 <= kind <= 12:
        order = kind - 8
        out = [b.signed(bps) for _ in range(order)]
        res, po, ks = _residual(b, m, order)
        coeff = {0: [], 1: [1], 2: [2, -1], 3: [3, -3, 1], 4: [4, -6, 4, -1]}[order]
        for r in res:
            out.append(r + sum(c * out[-1 - j] for j, c in enumerate(coeff)))
        return out, ("fixed", order, po, ks)
    assert 32 <= kind <= 63, f"subframe type {kind:06b}"
    order = kind - 31
    assert order <= m, "more warm-up samples than the block holds"
    out = [b.signed(bps) for _ in range(order)]
    precision = b.read(4) + 1
    assert precision != 16, "invalid coefficient precision"
    shift = b.signed(5)
    assert shift >= 0, "a negative shift is forbidden"
    coeff = [b.signed(precision) for _ in range(order)]            # the first one multiplies the sample directly before
    res, po, ks = _residual(b, m, order)
    for r in res:
        out.append(r + (sum(c * out[-1 - j] for j, c in enumerate(coeff)) >> shift))      # Python's >> floors, as the format wants
    return out, ("lpc", order, po, ks, precision, shift, coeff)


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


def decode_frames(data, sample_rate=None, first_number=None):
    """Frames back to back until the data ends exactly: -> (samples int16, [{"what": the subframe's tuple, "bytes", "bits": of the
    subframe, "m"}], [frame numbers]).  Header CRC-8 and frame CRC-16 are checked."""
    data = bytes(data)
    pos, samples, frames, numbers = 0, [], [], []
    while pos < len(data):
        b = Bits(data, pos)
        assert b.read(15) == 0x7FFC and b.read(1) == 0, f"no sync code of a fixed-block-size stream at byte {pos}"
        bs_code, sr_code = b.read(4), b.read(4)
        assert b.read(4) == 0 and b.read(3) == 4 and b.read(1) == 0, "one channel of 16 bits expected"
        number = _coded_number(b)
        m = b.read(8) + 1 if bs_code == 6 else b.read(16) + 1 if bs_code == 7 else BLOCK_SIZES[bs_code]
        rate = b.read(8) * 1000 if sr_code == 12 else b.read(16) if sr_code == 13 else b.read(16) * 10 if sr_code == 14 else RATES.get(sr_code)
        assert sr_code != 15 and (sample_rate is None or rate is None or rate == sample_rate), (sr_code, rate)
        head_end = b.pos // 8
        assert b.read(8) == crc_bits(data[pos:head_end], 0x07, 8), "CRC-8 of the frame header"
        start = b.pos
        block, what = _subframe(b, m, 16)
        bits = b.pos - start
        pad = (-b.pos) % 8
        assert pad == 0 or b.read(pad) == 0, "padding bits are zero"
        body_end = b.pos // 8
        assert b.read(16) == crc_bits(data[pos:body_end], 0x8005, 16), "CRC-16 of the frame"
        assert len(block) == m and all(-32768 <= v <= 32767 for v in block), "a decoded sample leaves 16 bits"
        samples += block
        numbers.append(number)
        frames.append(dict(what=what, bytes=body_end + 2 - pos, bits=bits, m=m))
        pos = body_end + 2
    if first_number is not None:
        assert numbers == list(range(first_number, first_number + len(numbers))), numbers
    return np.array(samples, dtype=np.int16), frames, numbers


# ------------------------------------------------------------------ the size of an LPC subframe, slowly
def lpc_residuals(x, shift, coeff):
    x = [int(v) for v in x]
    p = len(coeff)
    return [x[n] - (sum(coeff[j] * x[n - 1 - j] for j in range(p)) >> shift) for n in range(p, len(x))]


def lpc_bits(x, shift, coeff, po, ks=None, precision=12):
    """Size of the LPC subframe of the samples x with the given predictor and partition order, code by code: with the given Rice
    parameters, or (ks None) the best k of each partition and the lowest such k.  -> (bits, ks); None if po does not fit."""
    m, p = len(x), len(coeff)
    if m % (1 << po) or (m >> po) <= p:
        return None
    res, at = lpc_residuals(x, shift, coeff), 0
    bits, chosen = 8 + 16 * p + 4 + 5 + precision * p + 2 + 4, []
    for part in range(1 << po):
        count = (m >> po) - (p if part == 0 else 0)
        piece = res[at: at + count]
        at += count
        sizes = [rice_bits(piece, k) for k in range(15)]
        k = sizes.index(min(sizes)) if ks is None else ks[part]
        chosen.append(k)
        bits += 4 + sizes[k]
    assert at == len(res)
    return bits, chosen


# ------------------------------------------------------------------ the rows of the device tests
def no_energy(m=40):
    """Only the first and the last sample are not zero: the window is zero there, so R[0] == 0 and the frame has no LPC candidate."""
    x = np.zeros(m, np.int16)
    x[0], x[-1] = 1200, -700
    return x


def lpc_cases():
    """[(name, pcm, frame0, last)]: the rows of tests/flac_util.device_cases, frames of 2, 3, 13 and 14 samples (below and around the
    highest order) and the frame without energy under the window."""
    big = signals(BLOCK)
    cases = list(device_cases())
    cases += [(f"short_{m}", big["sine1k"][100: 100 + m].copy(), 40 + m, 1) for m in (2, 3, 13, 14)]
    cases.append(("no_energy", no_energy(), 9, 1))
    return cases


def mirror_layout(cases, rate, lpc_order=0):
    """What one vv_pcm_flac_lpc call over ``cases`` must give (lpc_order 0: vv_pcm_flac): -> (bytes, info (R + 1) x 3, the sum of the
    frame bounds)."""
    from vietvoice_tts_amd.core.audio_processor import flac_encode_frames, flac_frame_bound
    parts, info, at, bound = [], [], 0, 0
    for _name, x, frame0, last in cases:
        data, lo, hi = flac_encode_frames(x, rate, frame0, bool(last), lpc_order)
        info.append([at, lo, hi])
        parts.append(data)
        at += data.size
        full = x.size // BLOCK
        bound += full * flac_frame_bound(BLOCK) + flac_frame_bound(x.size - full * BLOCK)
    info.append([at, 0, 0])
    return np.concatenate(parts), np.array(info, np.int64), bound
