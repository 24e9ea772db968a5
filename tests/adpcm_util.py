"""What the N25 tests share (tests/test_adpcm_cpu.py, tests/test_adpcm_gpu.py, tests/test_adpcm_host_cpu.py, tools/adpcm_host_check.py,
tests/golden/make_adpcm_golden.py): the encoder's inputs, WAVE files written here byte by byte (not by the code under test), and a
per-sample reference of the IMA coder in plain Python integers, which shares no code and no table access pattern with the vectorised
mirror of core/audio_processor.py.  stdlib audioop, where it exists, is the other reference (CPython removed it in 3.13: the golden
file holds what it said)."""
import os
import struct

import numpy as np

from tests.flac_util import speechlike

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "adpcm_golden.npz")
SPBS = (505, 1017, 2041)                                 # 8 / 16 kHz, 22.05 / 24 kHz, 44.1 / 48 kHz
RATE_OF_SPB = {505: 8000, 1017: 24000, 2041: 48000}

STEPS = [7, 8, 9, 10, 11, 12, 13, 14, 16, 17, 19, 21, 23, 25, 28, 31, 34, 37, 41, 45, 50, 55, 60, 66, 73, 80, 88, 97, 107, 118, 130, 143, 157, 173, 190, 209,
         230, 253, 279, 307, 337, 371, 408, 449, 494, 544, 598, 658, 724, 796, 876, 963, 1060, 1166, 1282, 1411, 1552, 1707, 1878, 2066, 2272, 2499,
         2749, 3024, 3327, 3660, 4026, 4428, 4871, 5358, 5894, 6484, 7132, 7845, 8630, 9493, 10442, 11487, 12635, 13899, 15289, 16818, 18500, 20350,
         22385, 24623, 27086, 29794, 32767]
INDEX = [-1, -1, -1, -1, 2, 4, 6, 8] * 2


def lengths(spb):
    return (1, 2, spb - 1, spb, spb + 1, 2 * spb, 3 * spb + 7)


def encoder_inputs(spb):
    """[(name, int16 signal)]: the speech stand-in at every length of the issue's list, and silence, a full-scale square wave that
    includes -32768 (the predictor clamp) and a ramp, each over 2 spb + 9 samples (a whole block, and a padded one)."""
    out = [(f"speech_{n}", speechlike(n, seed=5 + n % 7, sr=RATE_OF_SPB[spb])) for n in lengths(spb)]
    n = 2 * spb + 9
    out.append(("silence", np.zeros(n, np.int16)))
    out.append(("square", np.where((np.arange(n) // 37) % 2, 32767, -32768).astype(np.int16)))
    out.append(("ramp", np.clip(np.arange(n) * 29 - 30000, -32768, 32767).astype(np.int16)))
    return out


def pad_blocks(x, spb):
    """int16 [n] -> int64 [blocks][spb], the last block padded with its last real sample."""
    nb = -(-x.size // spb)
    return np.concatenate([x, np.full(nb * spb - x.size, x[-1], np.int16)]).reshape(nb, spb).astype(np.int64)


def ref_encode(block, s0, index):
    """lin2adpcm of one block body in plain integers -> (codes, reconstruction)."""
    pred, codes, recon = int(s0), [], []
    for v in block:
        step, d = STEPS[index], int(v) - pred
        sign, d = (8, -d) if d < 0 else (0, d)
        code, vp = 0, step >> 3
        if d >= step:
            code, d, vp = 4, d - step, vp + step
        if d >= step >> 1:
            code, d, vp = code | 2, d - (step >> 1), vp + (step >> 1)
        if d >= step >> 2:
            code, vp = code | 1, vp + (step >> 2)
        pred = max(-32768, min(32767, pred - vp if sign else pred + vp))
        code |= sign
        index = max(0, min(88, index + INDEX[code]))
        codes.append(code)
        recon.append(pred)
    return codes, recon


def ref_decode(codes, s0, index):
    """adpcm2lin of 4-bit codes in plain integers."""
    pred, out = int(s0), []
    for c in codes:
        step = STEPS[index]
        vp = (step >> 3) + (step if c & 4 else 0) + (step >> 1 if c & 2 else 0) + (step >> 2 if c & 1 else 0)
        pred = max(-32768, min(32767, pred - vp if c & 8 else pred + vp))
        index = max(0, min(88, index + INDEX[c]))
        out.append(pred)
    return out


def swap_nibbles(b):
    b = np.asarray(b, np.uint8)
    return ((b >> 4) | (b << 4)).astype(np.uint8)


# ------------------------------------------------------------------ what stdlib audioop says (live, or recorded in the golden file)
def audioop_encoder_record(audioop, x, spb):
    """Per block of ``x``: the exhaustive search done with audioop alone -> (best index [B], its error [B], the error of the carried-state
    encoder [B], the bytes of all blocks as the WAVE layout wants them).  The carried chain: block 0 starts at index 0, every next block
    at the index audioop's state holds after the block before."""
    blocks = pad_blocks(x, spb)
    best, errs, carried, data, carry = [], [], [], bytearray(), 0
    for b, blk in enumerate(blocks):
        body, s0 = blk[1:].astype(np.int16), int(blk[0])
        real = min(max(x.size - b * spb - 1, 0), spb - 1)

        def run(index):
            codes, state = audioop.lin2adpcm(body.tobytes(), 2, (s0, index))
            recon = np.frombuffer(audioop.adpcm2lin(codes, 2, (s0, index))[0], np.int16).astype(np.int64)
            return codes, state, int(((body.astype(np.int64) - recon)[:real] ** 2).sum())
        e = [run(k)[2] for k in range(89)]
        k = int(np.argmin(e))                                # the first of equals
        codes, _state, _e = run(k)
        best.append(k)
        errs.append(e[k])
        _c, state, ce = run(carry)
        carried.append(ce)
        carry = state[1]
        data += struct.pack("<hBB", s0, k, 0) + swap_nibbles(np.frombuffer(codes, np.uint8)).tobytes()
    return np.array(best, np.int64), np.array(errs, np.int64), np.array(carried, np.int64), bytes(data)


def audioop_adpcm_frames(audioop, payload, channels, block_align, fact=None):
    """ref_adpcm_frames with audioop.adpcm2lin per block and channel (its first code sits in the high nibble: swapped here)."""
    ch, ba, out = channels, block_align, []
    for at in range(0, len(payload), ba):
        blk = payload[at: at + ba]
        if len(blk) < 4 * ch:
            break
        chans = []
        for c in range(ch):
            s0, index = struct.unpack("<hB", blk[4 * c: 4 * c + 3])
            body = b"".join(blk[g: g + 4] for g in range(4 * ch + 4 * c, len(blk), 4 * ch))
            pcm = np.frombuffer(audioop.adpcm2lin(swap_nibbles(np.frombuffer(body, np.uint8)).tobytes(), 2, (s0, index))[0], np.int16)
            chans.append(np.concatenate([[s0], pcm]).astype(np.int16))
        m = min(len(c) for c in chans)
        out.append(np.stack([c[:m] for c in chans], axis=1))
    frames = np.concatenate(out) if out else np.zeros((0, ch), np.int16)
    return frames if fact is None else frames[:fact]


# ------------------------------------------------------------------ files for the decoder, written here
def wav_file(tag, channels, rate, block_align, bits, payload, fact=None, extensible=False, samples_per_block=None):
    """A RIFF/WAVE file around ``payload``: fmt (18 or 20 bytes, or WAVE_FORMAT_EXTENSIBLE with the tag in the sub-format), fact, data."""
    if extensible:
        fmt = struct.pack("<HHIIHHHHI", 0xFFFE, channels, rate, rate * block_align, block_align, bits, 22, bits, 0) + \
            struct.pack("<H", tag) + bytes.fromhex("000000001000800000aa00389b71")
    elif samples_per_block is not None:
        fmt = struct.pack("<HHIIHHHH", tag, channels, rate, rate * block_align // samples_per_block, block_align, bits, 2, samples_per_block)
    else:
        fmt = struct.pack("<HHIIHHH", tag, channels, rate, rate * block_align, block_align, bits, 0)
    body = b"WAVE" + b"fmt " + struct.pack("<I", len(fmt)) + fmt
    if fact is not None:
        body += b"fact" + struct.pack("<II", 4, fact)
    payload = bytes(payload)
    body += b"data" + struct.pack("<I", len(payload)) + payload + b"\0" * (len(payload) & 1)
    return b"RIFF" + struct.pack("<I", len(body)) + body


def parse_wav(data):
    """The test's own chunk walk -> dict(tag, channels, rate, block_align, bits, fact, payload, data_at, fmt_at)."""
    pos, out = 12, {"fact": None}
    while pos + 8 <= len(data):
        cid, size = data[pos: pos + 4], struct.unpack("<I", data[pos + 4: pos + 8])[0]
        body = data[pos + 8: pos + 8 + size]
        if cid == b"fmt ":
            tag, ch, rate, _br, ba, bits = struct.unpack("<HHIIHH", body[:16])
            if tag == 0xFFFE:
                tag = struct.unpack("<H", body[24:26])[0]
            out.update(tag=tag, channels=ch, rate=rate, block_align=ba, bits=bits, fmt_at=pos + 8)
        elif cid == b"fact":
            out["fact"] = struct.unpack("<I", body[:4])[0]
        elif cid == b"data":
            out.update(payload=body, data_at=pos + 8)
        pos += 8 + size + (size & 1)
    return out


def adpcm_payload(x, block_align, seed=0):
    """int16 frames [n][channels] -> blocks of ``block_align`` bytes in the WAVE layout, coded by ref_encode from a seeded step index per
    block and channel (a decoder test does not care how the codes were chosen).  n must fill whole blocks."""
    x = np.asarray(x, np.int16)
    n, ch = x.shape
    spb = (block_align // ch - 4) * 2 + 1
    assert n % spb == 0
    rng, out = np.random.default_rng(seed), bytearray()
    for b in range(n // spb):
        blk = x[b * spb: (b + 1) * spb]
        heads, bodies = b"", []
        for c in range(ch):
            index = int(rng.integers(0, 89))
            heads += struct.pack("<hBB", int(blk[0, c]), index, 0)
            codes, _ = ref_encode(blk[1:, c], blk[0, c], index)
            bodies.append(bytes(codes[i] | (codes[i + 1] << 4) for i in range(0, len(codes), 2)))
        out += heads
        for g in range(0, len(bodies[0]), 4):
            for c in range(ch):
                out += bodies[c][g: g + 4]
    return bytes(out)


def ref_adpcm_frames(payload, channels, block_align, fact=None):
    """The data chunk's bytes -> int16 frames [n][channels], block by block and code by code in plain Python (ref_decode); a trailing part
    of a block gives the frames whose codes are there for every channel."""
    ch, ba, out = channels, block_align, []
    for at in range(0, len(payload), ba):
        blk = payload[at: at + ba]
        if len(blk) < 4 * ch:
            break
        chans = []
        for c in range(ch):
            s0, index = struct.unpack("<hB", blk[4 * c: 4 * c + 3])
            codes, g = [], 4 * ch + 4 * c
            while g < len(blk):
                for byte in blk[g: g + 4]:
                    codes += [byte & 15, byte >> 4]
                g += 4 * ch
            chans.append([s0] + ref_decode(codes, s0, index))
        m = min(len(c) for c in chans)
        out += [[c[t] for c in chans] for t in range(m)]
    frames = np.array(out, np.int16).reshape(-1, ch)
    return frames if fact is None else frames[:fact]


def decoder_files():
    """[(name, file bytes, want, rate)]: mu-law and A-law over all 256 codes (mono and stereo), mono and stereo ADPCM at 8 / 16 / 24 kHz
    block sizes, WAVE_FORMAT_EXTENSIBLE, a fact chunk that states fewer frames, and a partial last block of every kind.  want = the int16
    frames [n][channels] for ADPCM (ref_adpcm_frames), or (tag, codes [n][channels]) for G.711: the caller has the tables."""
    out = []
    codes = np.arange(256, dtype=np.uint8)
    for tag, name in ((7, "ulaw"), (6, "alaw")):
        for ch in (1, 2):
            pay = np.concatenate([codes, codes[::-1], codes[:37 * ch]])
            out.append((f"{name}_{ch}ch", wav_file(tag, ch, 8000, ch, 8, pay, fact=pay.size // ch), (tag, pay.reshape(-1, ch)), 8000))
    out.append(("ulaw_ext", wav_file(7, 1, 8000, 1, 8, codes, extensible=True), (7, codes.reshape(-1, 1)), 8000))
    out.append(("alaw_fact", wav_file(6, 1, 8000, 1, 8, codes, fact=100), (6, codes[:100].reshape(-1, 1)), 8000))
    for rate, ba in ((8000, 256), (16000, 256), (24000, 512)):                                   # ba = bytes per channel and block
        for ch in (1, 2):
            spb = (ba - 4) * 2 + 1
            x = np.stack([speechlike(3 * spb, seed=11 + c, sr=rate) for c in range(ch)], axis=1)
            pay = adpcm_payload(x, ba * ch, seed=rate + ch)
            out.append((f"adpcm_{rate}_{ch}ch", wav_file(0x11, ch, rate, ba * ch, 4, pay, fact=3 * spb, samples_per_block=spb),
                        ref_adpcm_frames(pay, ch, ba * ch), rate))
    small = adpcm_payload(np.stack([speechlike(3 * 25, seed=3), speechlike(3 * 25, seed=4)], axis=1), 32, seed=1)      # 3 stereo blocks of 25 frames
    out.append(("adpcm_ext", wav_file(0x11, 2, 8000, 32, 4, small, extensible=True), ref_adpcm_frames(small, 2, 32), 8000))
    out.append(("adpcm_fact", wav_file(0x11, 2, 8000, 32, 4, small, fact=40), ref_adpcm_frames(small, 2, 32, 40), 8000))
    for cut in (1, 7, 8, 9, 12, 13, 19, 31):                                                     # a partial third block of every kind
        out.append((f"adpcm_part_{cut}", wav_file(0x11, 2, 8000, 32, 4, small[: 64 + cut]), ref_adpcm_frames(small[: 64 + cut], 2, 32), 8000))
    mono = adpcm_payload(speechlike(75, seed=9).reshape(-1, 1), 16, seed=2)
    for cut in (3, 4, 5, 15):
        out.append((f"adpcm_mono_part_{cut}", wav_file(0x11, 1, 8000, 16, 4, mono[: 32 + cut]), ref_adpcm_frames(mono[: 32 + cut], 1, 16), 8000))
    return out


def small_files():
    """One small mono and one small stereo ADPCM file (3 blocks of 16 bytes per channel, 25 frames each) for the truncation and bit-flip
    lists -> [(name, file bytes, the offset of the data chunk's body)]."""
    out = []
    for ch in (1, 2):
        x = np.stack([speechlike(75, seed=20 + c) for c in range(ch)], axis=1)
        data = wav_file(0x11, ch, 8000, 16 * ch, 4, adpcm_payload(x, 16 * ch, seed=ch), fact=75, samples_per_block=25)
        out.append((f"small_{ch}ch", data, data.index(b"data") + 8))
    return out


def bad_index_file(ch=1, block=2):
    """A 4-block ADPCM file at 8 kHz whose block ``block`` (the third) has a step index of 89 in its last channel -> (bytes, the byte)."""
    ba = 256 * ch
    spb = (ba // ch - 4) * 2 + 1
    x = np.stack([speechlike(4 * spb, seed=30 + c, sr=8000) for c in range(ch)], axis=1)
    data = bytearray(wav_file(0x11, ch, 8000, ba, 4, adpcm_payload(x, ba, seed=7), fact=4 * spb, samples_per_block=spb))
    at = data.index(b"data") + 8 + block * ba + 4 * (ch - 1) + 2
    data[at] = 89
    return bytes(data), at
