"""A FLAC *writer* in plain Python integers (RFC 9639), for the tests of the FLAC input.  It shares nothing with the
product: it starts from known samples and explicit choices (channel assignment, depth, block sizes, blocking, frame numbers, subframe
kind and order, LPC precision / shift / coefficients, wasted bits, residual method, partition order, parameters, escapes, metadata
blocks, ID3v2 prefix, trailing bytes), so the expected output of every case is its own input, independent of any decoder."""
import struct

import numpy as np

from tests.flac_util import crc_bits

RATE_CODES = {88200: 1, 176400: 2, 192000: 3, 8000: 4, 16000: 5, 22050: 6, 24000: 7, 32000: 8, 44100: 9, 48000: 10, 96000: 11}
BLOCK_CODES = {192: 1, 576: 2, 1152: 3, 2304: 4, 4608: 5, 256: 8, 512: 9, 1024: 10, 2048: 11, 4096: 12, 8192: 13, 16384: 14, 32768: 15}
DEPTH_CODES = {8: 1, 12: 2, 16: 4, 20: 5, 24: 6, 32: 7}
FIXED = ((), (1,), (2, -1), (3, -3, 1), (4, -6, 4, -1))


class BitWriter:
    def __init__(self):
        self.v, self.n = 0, 0

    def put(self, value, bits):
        assert bits >= 0 and -(1 << bits) <= value < (1 << bits), (value, bits)
        self.v = (self.v << bits) | (value & ((1 << bits) - 1))
        self.n += bits

    def unary(self, zeros):
        self.put(1, zeros + 1)

    def align(self):
        self.put(0, -self.n % 8)

    def bytes(self):
        assert self.n % 8 == 0
        return self.v.to_bytes(self.n // 8, "big")


def coded_number(v):
    """The extended UTF-8 coding of a frame or sample number: 1 ... 7 bytes for up to 36 bits."""
    if v < 0x80:
        return bytes([v])
    n = 2
    while n < 7 and v >= 1 << (5 * n + 1):
        n += 1
    lead = ((0xFF << (8 - n)) & 0xFF) | (v >> (6 * (n - 1)) if n < 7 else 0)
    return bytes([lead] + [0x80 | ((v >> (6 * i)) & 0x3F) for i in range(n - 2, -1, -1)])


def _rice_len(us, k):
    return sum((u >> k) + 1 + k for u in us)


def subframe(w, x, depth, kind="verbatim", order=0, precision=12, shift=0, coefs=(), wasted=0, method=0, po=0, params=None, escapes=None,
             type_code=None, precision_code=None, shift_code=None, po_code=None):
    """One subframe of the samples x at ``depth`` bits.  ``params``: the Rice parameter of each partition (None = the cheapest),
    ``escapes``: {partition: raw bits}.  type_code / precision_code / shift_code / po_code overwrite the written fields (malformed streams)."""
    x = [int(v) for v in x]
    bs = len(x)
    assert all(v % (1 << wasted) == 0 for v in x)
    x = [v >> wasted for v in x]
    de = depth - wasted
    assert all(-(1 << (de - 1)) <= v < (1 << (de - 1)) for v in x), "sample does not fit the depth"
    code = {"constant": 0, "verbatim": 1, "fixed": 8 + order, "lpc": 32 + order - 1}[kind] if type_code is None else type_code
    w.put(0, 1)
    w.put(code, 6)
    w.put(1 if wasted else 0, 1)
    if wasted:
        w.unary(wasted - 1)
    if kind == "constant":
        assert all(v == x[0] for v in x)
        w.put(x[0], de)
        return
    if kind == "verbatim":
        for v in x:
            w.put(v, de)
        return
    for v in x[:order]:
        w.put(v, de)
    if kind == "lpc":
        assert len(coefs) == order
        w.put(precision - 1 if precision_code is None else precision_code, 4)
        w.put(shift if shift_code is None else shift_code, 5)
        for c in coefs:
            w.put(c, precision)
    else:
        coefs, shift = FIXED[order], 0
    res = [x[i] - (sum(c * x[i - 1 - j] for j, c in enumerate(coefs)) >> shift) for i in range(order, bs)]
    w.put(method, 2)
    w.put(po if po_code is None else po_code, 4)
    pbits, escapes = 4 + method, escapes or {}
    kmax = (1 << pbits) - 2
    at = 0
    for part in range(1 << po):
        n = (bs >> po) - (order if part == 0 else 0)
        rs = res[at:at + n]
        at += n
        if part in escapes:
            raw = escapes[part]
            w.put((1 << pbits) - 1, pbits)
            w.put(raw, 5)
            for r in rs:
                assert raw > 0 or r == 0
                if raw:
                    w.put(r, raw)
            continue
        us = [2 * r if r >= 0 else -2 * r - 1 for r in rs]
        k = params[part] if params is not None else min(range(kmax + 1), key=lambda k: (_rice_len(us, k), k))
        w.put(k, pbits)
        for u in us:
            w.unary(u >> k)
            w.put(u & ((1 << k) - 1), k)
    assert at == len(res)


def frame(channels, bits, rate, number, assign=None, variable=False, block_field=None, rate_field="table", depth_code=None, subs=None,
          corrupt_crc8=False, corrupt_crc16=False):
    """One frame.  channels: the samples of each channel as they are to come OUT (left, right for the stereo modes); assign: None =
    independent, 8 left/side, 9 side/right, 10 mid/side.  block_field: None = the table code where one exists, else 6 / 7 = the 8- /
    16-bit field.  rate_field: "table", 0 (STREAMINFO's), 12 (kHz), 13 (Hz), 14 (tens of Hz).  subs: one dict of subframe() options per
    channel (default verbatim)."""
    nch, bs = len(channels), len(channels[0])
    ch = [[int(v) for v in c] for c in channels]
    if assign == 8:
        ch = [ch[0], [a - b for a, b in zip(ch[0], ch[1])]]
    elif assign == 9:
        ch = [[a - b for a, b in zip(ch[0], ch[1])], ch[1]]
    elif assign == 10:
        ch = [[(a + b) >> 1 for a, b in zip(ch[0], ch[1])], [a - b for a, b in zip(ch[0], ch[1])]]
    bcode = block_field if block_field is not None else BLOCK_CODES.get(bs, 6 if bs <= 256 else 7)
    rcode = RATE_CODES[rate] if rate_field == "table" else rate_field
    head = bytes([0xFF, 0xF8 | (1 if variable else 0), (bcode << 4) | rcode,
                  ((assign if assign is not None else nch - 1) << 4) | ((DEPTH_CODES[bits] if depth_code is None else depth_code) << 1)])
    head += coded_number(number)
    if bcode == 6:
        head += bytes([bs - 1])
    elif bcode == 7:
        head += struct.pack(">H", bs - 1)
    if rcode == 12:
        head += bytes([rate // 1000])
    elif rcode == 13:
        head += struct.pack(">H", rate)
    elif rcode == 14:
        head += struct.pack(">H", rate // 10)
    head += bytes([crc_bits(head, 0x07, 8) ^ (1 if corrupt_crc8 else 0)])
    w = BitWriter()
    side = {8: 1, 9: 0, 10: 1}.get(assign, -1)
    for c in range(nch):
        subframe(w, ch[c], bits + (1 if c == side else 0), **((subs[c] if subs else None) or {}))
    w.align()
    body = head + w.bytes()
    return body + struct.pack(">H", crc_bits(body, 0x8005, 16) ^ (1 if corrupt_crc16 else 0))


def streaminfo(min_block, max_block, rate, channels, bits, total, last=True):
    packed = (rate << 44) | ((channels - 1) << 41) | ((bits - 1) << 36) | total
    return bytes([0x80 if last else 0, 0, 0, 34]) + struct.pack(">HH", min_block, max_block) + bytes(6) + packed.to_bytes(8, "big") + bytes(16)


def metadata(kind, body, last=False):
    return bytes([(0x80 if last else 0) | kind]) + len(body).to_bytes(3, "big") + bytes(body)


def id3v2(size):
    return b"ID3\x04\x00\x00" + bytes([(size >> 21) & 0x7F, (size >> 14) & 0x7F, (size >> 7) & 0x7F, size & 0x7F]) + bytes(range(256)) * (size // 256) + bytes(size % 256)


def stream(frames, rate, channels, bits, total, min_block, max_block, blocks=(), prefix=b"", trailing=b""):
    """A complete file: prefix, ``fLaC``, STREAMINFO, further metadata blocks [(type, body)], the frames, trailing bytes."""
    head = b"fLaC" + streaminfo(min_block, max_block, rate, channels, bits, total, last=not blocks)
    for i, (kind, body) in enumerate(blocks):
        head += metadata(kind, body, last=i == len(blocks) - 1)
    return prefix + head + b"".join(frames) + trailing


def simple_stream(x, bits=16, rate=24000, block=4096, total=None, variable=False, first_number=0, assign=None, subs=None, blocks=(), prefix=b"",
                  trailing=b"", block_field=None, rate_field="table", depth_code=None, max_block=None):
    """x (n, channels) -> a stream of frames of ``block`` samples (the last one short); with ``variable`` the coded number is the first
    sample's.  ``subs``: a function (frame index, channel, samples) -> subframe() options, or None."""
    x = np.asarray(x).reshape(len(x), -1)
    n, nch = x.shape
    frames = []
    for f, at in enumerate(range(0, n, block)):
        part = x[at:at + block]
        opts = [subs(f, c, part[:, c]) for c in range(nch)] if subs else None
        frames.append(frame([part[:, c] for c in range(nch)], bits, rate, at if variable else first_number + f, assign, variable,
                            block_field, rate_field, depth_code, opts))
    return stream(frames, rate, nch, bits, n if total is None else total, min(block, 65535), max_block or max(block, 16), blocks, prefix, trailing)


def layout(x, bits):
    """(n, channels) samples -> what the WAV of the same PCM decodes to: int8, int16, or int32 = the sample in the upper three bytes
    with the sign pad in the lowest."""
    x = np.asarray(x, np.int64).reshape(len(x), -1)
    if bits == 8:
        return x.astype(np.int8)
    if bits == 16:
        return x.astype(np.int16)
    return ((x << 8) | np.where(x < 0, 0xFF, 0)).astype(np.int32)


def wav_bytes(x, bits, rate):
    """The RIFF/WAVE file of the same PCM (8 bits unsigned, as WAVE has it)."""
    x = np.asarray(x, np.int64).reshape(len(x), -1)
    n, nch = x.shape
    if bits == 8:
        raw = (x + 128).astype(np.uint8).tobytes()
    elif bits == 16:
        raw = x.astype("<i2").tobytes()
    else:
        raw = (x & 0xFFFFFF).astype("<u4").reshape(-1, 1).view(np.uint8)[:, :3].tobytes()
    fmt = struct.pack("<HHIIHH", 1, nch, rate, rate * nch * bits // 8, nch * bits // 8, bits)
    return b"RIFF" + struct.pack("<I", 36 + len(raw)) + b"WAVEfmt " + struct.pack("<I", 16) + fmt + b"data" + struct.pack("<I", len(raw)) + raw + (b"\0" if len(raw) & 1 else b"")


def _noise(rng, n, nch, bits, scale=0.3):
    top = int((1 << (bits - 1)) * scale)
    return rng.integers(-top, top + 1, (n, nch)).astype(np.int64)


def _tone(n, nch, bits, rng):
    t = np.arange(n)[:, None]
    amp = (1 << (bits - 1)) * 0.4
    return np.round(amp * np.sin(2 * np.pi * t * (0.011 + 0.004 * np.arange(nch)[None, :])) + rng.integers(-3, 4, (n, nch))).astype(np.int64)


_CASES = None


def cases():
    """[(name, FLAC bytes, samples (n, channels) int64, bits, rate)]: the case list of the issue.  Built once."""
    global _CASES
    if _CASES is not None:
        return _CASES
    rng = np.random.default_rng(1709)
    out = []

    def add(name, data, x, bits=16, rate=24000):
        out.append((name, data, np.asarray(x, np.int64).reshape(len(x), -1), bits, rate))

    const = lambda f, c, s: dict(kind="constant")                      # noqa: E731
    # block sizes
    x = np.array([[-1234]])
    add("block_1", simple_stream(x, block=1, max_block=16), x)
    x = _tone(16 * 3 + 1, 1, 16, rng)
    add("block_16_17", stream([frame([x[:16, 0]], 16, 24000, 0), frame([x[16:32, 0]], 16, 24000, 1), frame([x[32:, 0]], 16, 24000, 2)],
                              24000, 1, 16, 49, 16, 17), x)
    for b in (192, 4096, 4608):
        x = _tone(b + 100, 1, 16, rng)
        add(f"block_{b}", simple_stream(x, block=b, subs=lambda f, c, s: dict(kind="fixed", order=2, po=0 if len(s) % 2 else 1)), x)
    x = np.full((65535, 2), 77)
    x[:, 1] = -3
    add("block_65535_constant", simple_stream(x, block=65535, subs=const), x)
    # every block-size code (constant subframes keep the large ones small) and the explicit fields
    for b, code in sorted(BLOCK_CODES.items()):
        x = np.full((b, 1), code * 100 - 800)
        add(f"block_code_{code}", simple_stream(x, block=b, subs=const), x)
    x = _noise(rng, 200, 1, 16)
    add("block_field_8bit", simple_stream(x, block=200, block_field=6), x)
    add("block_field_16bit_small", simple_stream(x, block=200, block_field=7), x)
    x = _noise(rng, 300, 1, 16)
    add("block_field_16bit", simple_stream(x, block=300), x)
    # every rate code
    x = _noise(rng, 64, 1, 16)
    for rate in sorted(RATE_CODES):
        add(f"rate_{rate}", simple_stream(x, rate=rate, block=64), x, 16, rate)
    add("rate_from_streaminfo", simple_stream(x, rate=12345, block=64, rate_field=0), x, 16, 12345)
    add("rate_khz_field", simple_stream(x, rate=11000, block=64, rate_field=12), x, 16, 11000)
    add("rate_hz_field", simple_stream(x, rate=11025, block=64, rate_field=13), x, 16, 11025)
    add("rate_tens_field", simple_stream(x, rate=352800, block=64, rate_field=14), x, 16, 352800)
    add("depth_from_streaminfo", simple_stream(x, block=64, depth_code=0), x)
    # coded numbers across the 1 -> 2 -> 3 byte lengths
    x = _noise(rng, 16 * 4, 1, 16)
    add("numbers_127", simple_stream(x, block=16, first_number=126), x)
    add("numbers_2047", simple_stream(x, block=16, first_number=2046), x)
    add("numbers_7_bytes", stream([frame([x[:, 0]], 16, 24000, (1 << 35) + 5, variable=True)], 24000, 1, 16, 64, 16, 64), x)
    # variable blocking
    x = _tone(16 + 100 + 4096 + 33, 2, 16, rng)
    cuts, frames = [0, 16, 116, 4212, 4245], []
    for a, b in zip(cuts, cuts[1:]):
        frames.append(frame([x[a:b, 0], x[a:b, 1]], 16, 24000, a, variable=True, subs=[dict(kind="fixed", order=1)] * 2))
    add("variable_blocking", stream(frames, 24000, 2, 16, len(x), 16, 4096), x)
    # channels
    for nch in (1, 2, 3, 8):
        x = _tone(500, nch, 16, rng)
        add(f"channels_{nch}", simple_stream(x, block=256, subs=lambda f, c, s: dict(kind="fixed", order=c % 5 if len(s) > 4 else 0)), x)
    # stereo modes with odd sides, full-scale opposite channels (a 17-bit side at 16 bits, a 25-bit side at 24)
    for assign in (None, 8, 9, 10):
        x = _tone(301, 2, 16, rng)
        x[::2, 0] |= 1
        x[::2, 1] &= ~1
        add(f"stereo_{assign}", simple_stream(x, block=128, assign=assign, subs=lambda f, c, s: dict(kind="fixed", order=1)), x)
    for bits in (16, 24):
        top = 1 << (bits - 1)
        x = np.array([[top - 1, -top], [-top, top - 1], [top - 1, -top], [-top, top - 1]] * 8)
        for assign in (8, 9, 10):
            add(f"full_scale_side_{bits}_{assign}", simple_stream(x, bits=bits, block=32, assign=assign), x, bits)
    # predictors at block sizes equal to the order and order + 1
    for o in range(5):
        for bs in sorted({max(o, 1), o + 1}):
            x = _noise(rng, bs, 1, 16)
            add(f"fixed_{o}_block_{bs}", simple_stream(x, block=bs, max_block=16, subs=lambda f, c, s, o=o: dict(kind="fixed", order=o)), x)
    for o in (1, 2, 12, 32):
        q = [int(v) for v in rng.integers(-300, 301, o)]
        q[0] = 1800
        for bs in (o, o + 1, o + 200):
            x = _tone(bs, 1, 16, rng) // 4
            add(f"lpc_{o}_block_{bs}", simple_stream(x, block=bs, max_block=max(bs, 16),
                                                     subs=lambda f, c, s, o=o, q=q: dict(kind="lpc", order=o, precision=12, shift=11, coefs=q, method=1)), x)
    # partition orders 0 ... the highest that fits; partition 0 holding exactly ``order`` samples
    x = _tone(4096, 1, 16, rng)
    for po in range(0, 11):
        add(f"partition_order_{po}", simple_stream(x, block=4096, subs=lambda f, c, s, po=po: dict(kind="fixed", order=4, po=po)), x)
    x = np.full((32768, 1), 5)
    add("partition_order_15", simple_stream(x, block=32768, subs=lambda f, c, s: dict(kind="fixed", order=1, po=15)), x)
    x = _noise(rng, 64, 1, 16)
    add("partition_0_empty", simple_stream(x, block=64, subs=lambda f, c, s: dict(kind="fixed", order=4, po=4)), x)
    # Rice parameters 0, 14 and 30; escapes of 0, 1 and 31 raw bits
    x = _noise(rng, 64, 1, 16, 0.0001)
    add("rice_0", simple_stream(x, block=64, subs=lambda f, c, s: dict(kind="fixed", order=0, params=[0])), x)
    x = _noise(rng, 64, 1, 16, 0.9)
    add("rice_14", simple_stream(x, block=64, subs=lambda f, c, s: dict(kind="fixed", order=0, params=[14])), x)
    x = _noise(rng, 64, 1, 24, 0.9)
    add("rice_30", simple_stream(x, bits=24, block=64, subs=lambda f, c, s: dict(kind="fixed", order=0, method=1, params=[30])), x, 24)
    x = _noise(rng, 64, 1, 16)
    x[:16] = 0
    x[16:32, 0] = -(np.arange(16) % 2)
    add("escapes_0_1", simple_stream(x, block=64, subs=lambda f, c, s: dict(kind="fixed", order=0, po=2, escapes={0: 0, 1: 1})), x)
    x = _noise(rng, 32, 1, 24, 0.99)
    x[::2] *= -1
    add("escape_31", simple_stream(x, bits=24, block=32, subs=lambda f, c, s: dict(kind="fixed", order=4, method=1, escapes={0: 31})), x, 24)
    # wasted bits
    for wb in (1, 7):
        x = _tone(200, 2, 16, rng) >> wb << wb
        add(f"wasted_{wb}", simple_stream(x, block=100, assign=8 if wb == 1 else None,
                                          subs=lambda f, c, s, wb=wb: dict(kind="fixed", order=2, wasted=wb if c == 0 or wb == 7 else 0)), x)
    # 24-bit LPC at full scale: the prediction sum needs 64 bits
    top = (1 << 23) - 1
    x = np.array([[top if (i // 3) % 2 else -top - 1] for i in range(200)])
    q = [16383, -16384] * 16
    add("lpc_24_full_scale", simple_stream(x, bits=24, block=200, subs=lambda f, c, s: dict(kind="lpc", order=32, precision=15, shift=15, coefs=q,
                                                                                            method=1, escapes={0: 31})), x, 24)
    # the container
    x = _tone(700, 1, 16, rng)
    fx = lambda f, c, s: dict(kind="fixed", order=2)                    # noqa: E731
    add("total_unknown", simple_stream(x, block=256, total=0, subs=fx), x)
    add("padding_and_unknown_block", simple_stream(x, block=256, subs=fx, blocks=[(1, bytes(70000)), (99, b"\xff\xf8" * 50), (4, b"tags")]), x)
    add("id3_prefix", simple_stream(x, block=256, subs=fx, prefix=id3v2(300)), x)
    add("trailing_bytes", simple_stream(x, block=256, subs=fx, trailing=b"\xff\xf8\xc9\x08junk" * 9), x)
    # a verbatim subframe whose bytes spell a complete frame header with a correct CRC-8: the chain must pass over it
    fake = bytes([0xFF, 0xF8, 0x67, 0x08, 0x00, 0x1F])
    fake += bytes([crc_bits(fake, 0x07, 8)])
    payload = (fake + bytes([0x02]) + bytes(range(64)))[:70]
    x = np.frombuffer(payload, ">i2").astype(np.int64).reshape(-1, 1)
    x = np.concatenate([x, _noise(rng, 29, 1, 16)])
    add("header_inside_verbatim", simple_stream(x, block=64, max_block=64), x)
    for bits in (8, 24):
        x = _tone(300, 2, bits, rng)
        add(f"depth_{bits}", simple_stream(x, bits=bits, block=128, assign=10, subs=lambda f, c, s: dict(kind="fixed", order=2)), x, bits)
    _CASES = out
    return out


def malformed():
    """[(name, bytes, reason code, position)]: one stream per refusal of the issue's list, each one change away from a valid stream.
    Codes as in core.audio_processor.FlacStatus: 1 bad header, 2 CRC-8, 3 CRC-16, 4 reserved, 5 partition, 6 range, 7 overrun, 8 chain,
    9 frame too long, 10 clip too long.  The position is the first byte of the frame that holds the problem."""
    rng = np.random.default_rng(99)
    x = _tone(300, 1, 16, rng)
    good = simple_stream(x, block=128)                                  # verbatim: a flipped body bit changes no length, only the CRC-16
    f0 = 42
    f1 = f0 + len(frame([x[:128, 0]], 16, 24000, 0))
    f2 = f1 + len(frame([x[128:256, 0]], 16, 24000, 1))

    def flip(data, byte, bit=0):
        b = bytearray(data)
        b[byte] ^= 1 << bit
        return bytes(b)

    def one(sub, bs=128, **kw):
        return stream([frame([x[:bs, 0]], 16, 24000, 0, subs=[sub], **kw)], 24000, 1, 16, bs, 16, 4096)

    out = [
        ("header_bit", flip(good, f1 + 4, 1), 2, f1),
        ("sync_bit", flip(good, f1, 3), 1, f1),
        ("body_bit", flip(good, f1 + 30, 2), 3, f1),
        ("crc16_bit", flip(good, f2 - 1, 0), 3, f1),
        ("cut_last_frame", good[:-7], 7, f2),
        ("reserved_subframe_type", one(dict(kind="verbatim", type_code=5)), 4, f0),
        ("lpc_precision_15", one(dict(kind="lpc", order=1, coefs=[1], precision=2, shift=0, precision_code=15)), 4, f0),
        ("lpc_negative_shift", one(dict(kind="lpc", order=1, coefs=[1], precision=2, shift=0, shift_code=-3)), 4, f0),
        ("partition_misfit", one(dict(kind="fixed", order=0, po_code=1), bs=127), 5, f0),
        ("total_disagrees", simple_stream(x, block=128, total=301), 8, len(good)),
        ("total_short", simple_stream(x, block=128, total=200), 8, f1),
        ("garbage_after_total_0", simple_stream(x, block=128, total=0, trailing=b"junk"), 1, len(good)),
    ]
    for bits in (12, 20, 32):
        xs = _tone(64, 1, 8, rng)
        out.append((f"depth_{bits}", simple_stream(xs, bits=bits, block=64), 1, 4))
    # a frame over the bound: Rice parameter 0 on large residuals spends far more than twice the verbatim size
    xl = np.array([[1000 if i % 2 else -1000] for i in range(64)])
    out.append(("frame_over_the_bound", simple_stream(xl, block=64, subs=lambda f, c, s: dict(kind="fixed", order=0, params=[0])), 9, f0))
    # a restored sample outside the depth: LPC with a gain of 2 on full-scale warm-up (the writer's own check is bypassed by hand)
    w = BitWriter()
    w.put(0, 1); w.put(32, 6); w.put(0, 1); w.put(32767, 16)           # noqa: E702  LPC order 1, warm-up 32767
    w.put(1, 4); w.put(0, 5); w.put(1, 2)                              # noqa: E702  precision 2, shift 0, coefficient 1
    w.put(0, 2); w.put(0, 4); w.put(0, 4)                              # noqa: E702  method 0, partition order 0, k = 0
    for _ in range(15):
        w.put(0b001, 3)                                                # u = 2: residual +1 on top of the prediction
    w.align()
    head = bytes([0xFF, 0xF8, 0x67, 0x08, 0x00, 15])
    head += bytes([crc_bits(head, 0x07, 8)])
    body = head + w.bytes()
    out.append(("sample_out_of_range", stream([body + struct.pack(">H", crc_bits(body, 0x8005, 16))], 24000, 1, 16, 16, 16, 16), 6, f0))
    return out


def corpus_streams():
    """The two small streams of the malformed corpus: mono 16 bits, fixed blocking, Fixed + Rice, a known total; and stereo 8 bits,
    variable blocking, mid/side, LPC + wasted bits + an escape partition, total 0."""
    rng = np.random.default_rng(7)
    a = _tone(41, 1, 16, rng)
    sa = simple_stream(a, block=16, subs=lambda f, c, s: dict(kind="fixed", order=2 if len(s) > 2 else 0, po=1 if len(s) == 16 else 0))
    b = _tone(40, 2, 8, rng) >> 1 << 1
    frames = []
    for at, n in ((0, 16), (16, 24)):
        subs = [dict(kind="lpc", order=2, precision=5, shift=3, coefs=[12, -5], method=1, po=1 if n == 16 else 0), dict(kind="fixed", order=1, wasted=1, escapes={0: 6})]
        frames.append(frame([b[at:at + n, 0], b[at:at + n, 1]], 8, 16000, at, assign=8, variable=True, subs=subs))
    sb = stream(frames, 16000, 2, 8, 0, 16, 24)
    return [("mono16", sa, a, 16, 24000), ("stereo8", sb, b, 8, 16000)]


def malformed_corpus():
    """Every truncation length and every single-bit flip of the first 400 bytes and of the last frame of the two small streams:
    yields (name, bytes).  What each must give is whatever the mirror says: the device has to say the same."""
    for name, data, _x, _bits, _rate in corpus_streams():
        for n in range(len(data)):
            yield f"{name}_cut_{n}", data[:n]
        for bit in range(8 * len(data)):                                    # the streams are shorter than 400 bytes: every bit of them
            b = bytearray(data)
            b[bit >> 3] ^= 0x80 >> (bit & 7)
            yield f"{name}_flip_{bit}", bytes(b)
