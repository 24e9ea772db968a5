"""AudioProcessor -- host-side audio plumbing of the hot path, behaviour-identical to the reference
(vietvoicetts/core/audio_processor.py) for every pure-numpy step: DC removal + peak 29491 + int16
truncation (:28-44), clip repair (:46-58), linear cross-fade (:69-120), RMS-matched cos^2 cross-fade
(:122-192).  Pinned by tests/golden/host_golden.npz (generated from the reference functions).

``load_audio`` (:15-26) is ``AudioSegment.from_file(..).set_channels(1).set_frame_rate(sr)`` followed by
``get_array_of_samples`` -> float32 -> ``normalize_to_int16``.  pydub (pin: >=0.25.0, pyproject.toml:38) is absent
offline; for RIFF/WAVE PCM input its two calls are integer arithmetic of CPython's stdlib ``audioop``
(pydub/audio_segment.py ``set_channels``: ``audioop.tomono(data, width, 0.5, 0.5)``; ``set_frame_rate``:
``audioop.ratecv(data, width, channels, src, dst, None)``), restated here in closed form with numpy:

  tomono : floor(l * 0.5 + r * 0.5)                                    = (l + r) >> 1
  ratecv : output m sits at input position m * I / O (I, O = rates / gcd); with n1 = ceil(m * I / O),
           d = n1 * O - m * I in [0, O):  out = trunc((x32[n1 - 1] * d + x32[n1] * (O - d)) / O) >> (32 - 8 * width)
           (x32 = sample << (32 - 8 * width), x32[-1] = 0; products, sum and the truncated quotient are exact in
           float64 for the 16-bit case and O < 65536, where the whole expression equals floor((p * d + c * (O - d)) / O));
           floor((N - 1) * O / I) + 1 outputs for N input frames.

Bit-exact against stdlib ``audioop`` (tests/test_ingest_cpu.py, tests/golden/ingest_golden.npz) for widths 1, 2, 4.
pydub's own glue is restated from its published source and is "parity unpinned": 8-bit WAV is unsigned and gets
``audioop.bias(-128)``; 24-bit samples are widened to 32 bit with the sign byte written FIRST (value * 256 + 0x00 / 0xFF);
more than two channels are mixed as ``sum(sample // channels)``.  Float WAVE goes through ffmpeg in the reference
(``-acodec pcm_s32le``): restated as ``clip(llrint(x * 2**31))`` and unpinned; other containers need ffmpeg and are
out of scope.  ``save_audio`` writes a WAVE_FORMAT_EXTENSIBLE PCM16 file by hand (soundfile 'WAVEX' bytes unpinned).
The polyphase resampler of earlier rounds stays available as an explicit opt-in (``resampler="polyphase"``).
"""
from __future__ import annotations

import io
import math
import struct
from fractions import Fraction
from math import gcd
from pathlib import Path
from typing import List, NamedTuple, Optional, Tuple, Union

import numpy as np

_PCM_GUID = bytes.fromhex("0100000000001000800000aa00389b71")
_INT_OF_WIDTH = {1: np.int8, 2: np.int16, 4: np.int32}


class WavStatus:
    """Reason codes of a refused G.711 / IMA ADPCM WAVE clip (N25): one enum for this mirror and csrc/vv_adpcm.hip (VV_WAV_* in include/vvtts.h)."""
    OK, STEP_INDEX, BLOCK_ALIGN, BITS, CHANNELS = range(5)
    NAMES = ("ok", "step index above 88", "block alignment", "bits per sample", "more than 2 ADPCM channels")


class WavError(ValueError):
    """``malformed WAVE: <reason> at byte <position>``; ``code`` is a WavStatus, ``position`` a byte offset into the data given."""

    def __init__(self, code: int, position: int, detail: str = ""):
        self.code, self.position = int(code), int(position)
        super().__init__(f"malformed WAVE: {detail or WavStatus.NAMES[self.code]} at byte {self.position}")


class WavInfo(NamedTuple):
    tag: int                         # after WAVE_FORMAT_EXTENSIBLE is resolved
    channels: int
    rate: int
    block_align: int
    bits: int
    fact: Optional[int]              # frames the fact chunk states, None without one
    fmt_at: int                      # the byte at which the fmt chunk's body starts
    data_at: int                     # the byte at which the data chunk's body starts
    data: bytes


def wav_container(data: bytes) -> WavInfo:
    """Byte parsing only: the RIFF chunks, the fields of ``fmt `` and, for the coded tags 6 / 7 / 0x11 (N25), the refusals that the header
    alone decides (position = the byte of the offending fmt field)."""
    if len(data) < 12 or data[:4] != b"RIFF" or data[8:12] != b"WAVE":
        raise ValueError("unsupported audio container: only RIFF/WAVE can be decoded in this build (no ffmpeg)")
    pos, fmt, pcm, fact, fmt_at, data_at = 12, None, None, None, 0, 0
    while pos + 8 <= len(data):
        cid, size = data[pos:pos + 4], struct.unpack("<I", data[pos + 4:pos + 8])[0]
        body = data[pos + 8: pos + 8 + size]
        if cid == b"fmt ":
            fmt, fmt_at = body, pos + 8
        elif cid == b"data":
            pcm, data_at = body, pos + 8
        elif cid == b"fact" and len(body) >= 4:
            fact = struct.unpack("<I", body[:4])[0]
        pos += 8 + size + (size & 1)
    if fmt is None or pcm is None or len(fmt) < 16:
        raise ValueError("malformed WAVE file: missing fmt or data chunk")
    tag, ch, rate, _br, align, bits = struct.unpack("<HHIIHH", fmt[:16])
    if tag == 0xFFFE and len(fmt) >= 26:
        tag = struct.unpack("<H", fmt[24:26])[0]
    if ch < 1 or rate < 1:
        raise ValueError("malformed WAVE file: zero channels or rate")
    if tag in (6, 7) and bits != 8:
        raise WavError(WavStatus.BITS, fmt_at + 14, f"{bits} bits per sample, G.711 has 8")
    if tag == 0x11:
        if bits != 4:
            raise WavError(WavStatus.BITS, fmt_at + 14, f"{bits} bits per sample, IMA ADPCM has 4")
        if ch > 2:
            raise WavError(WavStatus.CHANNELS, fmt_at + 2)
        if align < 8 * ch or align % (4 * ch):
            raise WavError(WavStatus.BLOCK_ALIGN, fmt_at + 12, f"block alignment {align}: a multiple of {4 * ch}, at least {8 * ch}")
    return WavInfo(tag, ch, int(rate), align, bits, fact, fmt_at, data_at, pcm)


def _decode_wav(data: bytes) -> Tuple[np.ndarray, int, int]:
    """RIFF/WAVE bytes -> (frames (n_frames, channels) of int8 / int16 / int32, sample width in bytes, rate): the
    samples pydub's AudioSegment holds after ``from_file`` (see the module docstring for the 8- / 24-bit / float glue).  Tags 6, 7
    (G.711) and 0x11 (IMA ADPCM) decode to int16 by audioop's arithmetic (N25, below); pydub hands these to ffmpeg: parity unpinned."""
    info = wav_container(data)
    tag, ch, rate, bits, pcm = info.tag, info.channels, info.rate, info.bits, info.data
    if tag in (6, 7, 0x11):
        return wav_coded_frames(info), 2, rate
    if tag == 1:
        if bits == 8:
            x, width = (np.frombuffer(pcm, dtype=np.uint8) ^ 0x80).view(np.int8), 1          # audioop.bias(data, 1, -128)
        elif bits == 16:
            x, width = np.frombuffer(pcm[: len(pcm) // 2 * 2], dtype="<i2"), 2
        elif bits == 24:
            b = np.frombuffer(pcm[: len(pcm) // 3 * 3], dtype=np.uint8).reshape(-1, 3)
            w = np.empty((b.shape[0], 4), np.uint8)
            w[:, 0] = np.where(b[:, 2] > 0x7F, 0xFF, 0x00)                                     # pydub writes the pad byte first
            w[:, 1:] = b
            x, width = w.reshape(-1).view("<i4"), 4
        elif bits == 32:
            x, width = np.frombuffer(pcm[: len(pcm) // 4 * 4], dtype="<i4"), 4
        else:
            raise ValueError(f"unsupported PCM width {bits}")
    elif tag == 3 and bits in (32, 64):
        f = np.frombuffer(pcm[: len(pcm) // (bits // 8) * (bits // 8)], dtype="<f4" if bits == 32 else "<f8").astype(np.float64)
        x, width = np.clip(np.rint(np.nan_to_num(f) * 2147483648.0), -2147483648.0, 2147483647.0).astype(np.int32), 4
    else:
        raise ValueError(f"unsupported WAVE format tag {tag}")
    x = x.astype(_INT_OF_WIDTH[width], copy=False)
    return np.ascontiguousarray(x[: len(x) // ch * ch].reshape(-1, ch)), width, int(rate)


def tomono(frames: np.ndarray) -> np.ndarray:
    """(n, channels) integer frames -> (n,) mono, pydub ``set_channels(1)``: 2 channels = audioop.tomono(.., 0.5, 0.5)
    (floor of the half sum), more = sum of floor-divided samples (OverflowError like pydub's array arithmetic when the
    floors add up below the range: only with every channel at negative full scale)."""
    ch = frames.shape[1]
    if ch == 1:
        return frames[:, 0]
    if ch == 2:
        return ((frames[:, 0].astype(np.int64) + frames[:, 1].astype(np.int64)) >> 1).astype(frames.dtype)
    mixed = (frames.astype(np.int64) // ch).sum(axis=1)
    info = np.iinfo(frames.dtype)
    if mixed.size and (mixed.min() < info.min or mixed.max() > info.max):     # pydub accumulates in an array.array of the width
        raise OverflowError("channel mix does not fit the sample width (every channel at negative full scale)")
    return mixed.astype(frames.dtype)


def ratecv_len(n_in: int, src: int, dst: int) -> int:
    """Frames audioop.ratecv(.., state=None) emits for n_in input frames."""
    if n_in <= 0:
        return 0
    g = gcd(src, dst)
    return (n_in - 1) * (dst // g) // (src // g) + 1


def ratecv(x: np.ndarray, src: int, dst: int) -> np.ndarray:
    """Mono integer samples at ``src`` Hz -> ``dst`` Hz, audioop.ratecv(data, width, 1, src, dst, None) (weights 1, 0):
    linear interpolation between the two neighbouring input samples, evaluated in float64 on the samples shifted to
    32 bit exactly as Modules/audioop.c does, truncated, shifted back."""
    if src == dst or x.size == 0:                      # pydub returns the segment itself / skips empty data
        return x
    g = gcd(src, dst)
    I, O = src // g, dst // g
    shift = 32 - 8 * x.dtype.itemsize
    m = np.arange(ratecv_len(x.size, src, dst), dtype=np.int64)
    n1 = (m * I + O - 1) // O
    d = (n1 * O - m * I).astype(np.float64)
    x32 = (x.astype(np.int64) << shift).astype(np.float64)
    prev = np.where(n1 > 0, x32[np.maximum(n1 - 1, 0)], 0.0)
    out = ((prev * d + x32[n1] * (float(O) - d)) / float(O)).astype(np.int64)        # C (int) cast: truncation
    return (out >> shift).astype(x.dtype)


def _resample_polyphase(x: np.ndarray, src: int, dst: int) -> np.ndarray:
    """Opt-in band-limited resampler (NOT the reference's arithmetic)."""
    if src == dst or x.size == 0:
        return x
    from scipy.signal import resample_poly
    g = gcd(src, dst)
    return resample_poly(x.astype(np.float64), dst // g, src // g).astype(np.float32)


OUTPUT_ENCODINGS = ("pcm16", "ulaw", "alaw", "flac", "adpcm")     # ModelConfig.output_encoding; G.711 = WAVE format tags 7 (mu-law) / 6 (A-law);
                                                          # "flac" = a complete FLAC file, lossless (N15); "adpcm" = a complete IMA ADPCM WAVE
                                                          # file, format tag 0x11, 4 bits per sample (N25)
_WAVE_TAG = {"pcm16": 1, "alaw": 6, "ulaw": 7}
_DESIGNS = {}


def output_design(src: int, dst: int):
    """(taps f64, up, down, skip) of the output-rate filter: voice_bank.resample_design(src, dst), designed once per rate pair."""
    key = (int(src), int(dst))
    if key not in _DESIGNS:
        from ..voice_bank import resample_design
        _DESIGNS[key] = resample_design(*key)
    return _DESIGNS[key]


def resample_len(n_in: int, up: int, down: int) -> int:
    """Samples scipy.signal.resample_poly returns for n_in input samples: ceil(n_in * up / down)."""
    return -(-int(n_in) * int(up) // int(down))


def resample_rows(x: np.ndarray, taps: np.ndarray, up: int, down: int, skip: int, m0: int, i0: int, n_out: int) -> np.ndarray:
    """Host mirror of vv_pcm_resample for one descriptor row: outputs m0 ... m0 + n_out - 1 of a signal whose samples
    i0 ... i0 + len(x) - 1 are ``x`` (int16); everything else contributes zero.  y[m] = clamp(rint(sum_i x[i] * taps[(m + skip) * down
    - i * up])), a float64 sum over ascending i (the kernel's order; it fuses each multiply-add, numpy rounds the product first: only a
    value on a tie can differ)."""
    x64 = np.asarray(x).reshape(-1).astype(np.float64)
    n_in, n_taps = x64.size, int(taps.size)
    if n_out <= 0:
        return np.zeros(0, np.int16)
    pos = (np.arange(m0, m0 + n_out, dtype=np.int64) + skip) * down
    i_hi = pos // up
    acc = np.zeros(n_out, np.float64)
    for k in range((n_taps + up - 1) // up, -1, -1):           # i = i_hi - k: ascending i
        i = i_hi - k
        t = pos - i * up
        ok = (t >= 0) & (t < n_taps) & (i >= i0) & (i < i0 + n_in)
        if not ok.any():
            continue
        xv = x64[np.clip(i - i0, 0, max(n_in - 1, 0))] if n_in else np.zeros(n_out)
        acc = acc + np.where(ok, xv * taps[np.clip(t, 0, n_taps - 1)], 0.0)
    return np.clip(np.rint(acc), -32768, 32767).astype(np.int16)


def resample_output(x: np.ndarray, src: int, dst: int) -> np.ndarray:
    """int16 PCM at ``src`` Hz -> int16 at ``dst`` Hz through the band-limited polyphase FIR of the voice bank (Kaiser beta 5, half length
    10 * max(up, down)): the host mirror of the device output stage.  NOT the reference's arithmetic (it has no output rate)."""
    x = np.asarray(x).reshape(-1)
    if int(src) == int(dst) or x.size == 0:
        return x
    taps, up, down, skip = output_design(src, dst)
    return resample_rows(x, taps, up, down, skip, 0, 0, resample_len(x.size, up, down))


def lin2ulaw(x: np.ndarray) -> np.ndarray:
    """int16 -> uint8 G.711 mu-law, audioop.lin2ulaw(data, 2): the segment arithmetic of CPython's Modules/audioop.c on sample >> 2
    (bias 0x21, clip 8159)."""
    v = np.asarray(x).reshape(-1).astype(np.int32) >> 2
    mask = np.where(v < 0, 0x7F, 0xFF)
    v = np.minimum(np.abs(v), 8159) + 0x21
    seg = np.zeros_like(v)
    for k in range(8):
        seg += v > ((0x40 << k) - 1)                       # seg_uend = 0x3F, 0x7F, ... 0x1FFF
    code = np.where(seg >= 8, 0x7F, (seg << 4) | ((v >> (np.minimum(seg, 7) + 1)) & 0xF))
    return (code ^ mask).astype(np.uint8)


def lin2alaw(x: np.ndarray) -> np.ndarray:
    """int16 -> uint8 G.711 A-law, audioop.lin2alaw(data, 2): the same source's st_linear2alaw on sample >> 3."""
    v = np.asarray(x).reshape(-1).astype(np.int32) >> 3
    mask = np.where(v >= 0, 0xD5, 0x55)
    v = np.where(v < 0, -v - 1, v)
    seg = np.zeros_like(v)
    for k in range(8):
        seg += v > ((0x20 << k) - 1)                       # seg_aend = 0x1F, 0x3F, ... 0xFFF
    s7 = np.minimum(seg, 7)
    code = np.where(seg >= 8, 0x7F, (seg << 4) | (np.where(seg < 2, v >> 1, v >> s7) & 0xF))
    return (code ^ mask).astype(np.uint8)


def encode_output(x: np.ndarray, encoding: str, sample_rate: int = 24000, lpc_order: int = 0) -> np.ndarray:
    """``x`` int16 -> the encoding's bytes.  "flac" gives the complete file (stream header + frames) as uint8 and is
    the one encoding that needs ``sample_rate``; ``lpc_order`` 1 ... 12 adds LPC subframes to it (N16) and is refused elsewhere."""
    if check_flac_lpc_order(lpc_order) and encoding != "flac":
        raise ValueError("lpc_order belongs to the encoding 'flac'")
    if encoding == "pcm16":
        return x
    if encoding == "ulaw":
        return lin2ulaw(x)
    if encoding == "alaw":
        return lin2alaw(x)
    if encoding == "flac":
        pcm = _flac_pcm(x)
        if pcm.size == 0:
            return np.frombuffer(flac_stream_header(sample_rate, 0), np.uint8).copy()
        frames, lo, hi = flac_encode_frames(pcm, sample_rate, lpc_order=lpc_order)
        return np.concatenate([np.frombuffer(flac_stream_header(sample_rate, pcm.size, lo, hi), np.uint8), frames])
    if encoding == "adpcm":
        pcm = _adpcm_pcm(x)
        return adpcm_wav(adpcm_encode_blocks(pcm, adpcm_samples_per_block(adpcm_block_align(sample_rate))), sample_rate, pcm.size)
    raise ValueError(f"output_encoding must be one of {list(OUTPUT_ENCODINGS)}")


# ---------------------------------------------------------------------- N25: IMA ADPCM output; IMA ADPCM and G.711 reference clips
# The arithmetic IS the specification: the quantiser and predictor of CPython's Modules/audioop.c (lin2adpcm / adpcm2lin,
# the Intel/DVI reference coder behind the IMA Digital Audio Focus Group's 1992 recommendation), in integers throughout, so this mirror,
# stdlib audioop and csrc/vv_adpcm.hip agree byte for byte.  Per sample, with the predictor p, the step s = ADPCM_STEPS[index]:
#     d = x - p; sign = d < 0; d = |d|; vp = s >> 3
#     d >= s      -> code |= 4, d -= s,      vp += s
#     d >= s >> 1 -> code |= 2, d -= s >> 1, vp += s >> 1
#     d >= s >> 2 -> code |= 1,              vp += s >> 2
#     p = clamp(p -/+ vp, int16); index = clamp(index + ADPCM_INDEX[code], 0, 88)
# A WAVE block (format tag 0x11, mono) is {int16 first sample, uint8 step index, uint8 0} and the codes of the samples behind the first, LOW
# nibble first (audioop packs the first code high).  The block header restarts the predictor, so blocks are independent -- and the step
# index of the header is free: every block tries all 89 and keeps the one with the smallest sum of (x - p)^2 over its real samples (p is what
# a decoder reconstructs; the padding of the last block, which repeats the last real sample, does not count), the smallest index of equals.
# The index a conventional encoder would carry over from the block before is one of the 89, so no block is worse than under that encoder.
ADPCM_STEPS = np.array([7, 8, 9, 10, 11, 12, 13, 14, 16, 17, 19, 21, 23, 25, 28, 31, 34, 37, 41, 45, 50, 55, 60, 66, 73, 80, 88, 97, 107, 118, 130, 143,
                        157, 173, 190, 209, 230, 253, 279, 307, 337, 371, 408, 449, 494, 544, 598, 658, 724, 796, 876, 963, 1060, 1166, 1282, 1411,
                        1552, 1707, 1878, 2066, 2272, 2499, 2749, 3024, 3327, 3660, 4026, 4428, 4871, 5358, 5894, 6484, 7132, 7845, 8630, 9493,
                        10442, 11487, 12635, 13899, 15289, 16818, 18500, 20350, 22385, 24623, 27086, 29794, 32767], np.int64)
ADPCM_INDEX = np.array([-1, -1, -1, -1, 2, 4, 6, 8] * 2, np.int64)
ADPCM_WAVE_TAG = 0x11
ADPCM_MAX_BLOCK_ALIGN = 4096         # VV_ADPCM_MAX_BLOCK_ALIGN: bytes of the largest block the encoder writes and the decoder follows (8185 samples)
ADPCM_HEADER_BYTES = 60              # RIFF 12, fmt 8 + 20, fact 8 + 4, data 8


def adpcm_block_align(sample_rate: int) -> int:
    """nBlockAlign of the output: 256 bytes per 11025 Hz of rate (256 at 8 / 16 kHz, 512 at 22.05 / 24 kHz, 1024 at 44.1 / 48 kHz)."""
    if isinstance(sample_rate, bool) or int(sample_rate) != sample_rate or int(sample_rate) < 1:
        raise ValueError("ADPCM: a positive integer sample rate is needed")
    align = 256 * max(1, int(sample_rate) // 11025)
    if align > ADPCM_MAX_BLOCK_ALIGN:
        raise ValueError(f"ADPCM: the rate {sample_rate} Hz needs blocks of {align} bytes, more than {ADPCM_MAX_BLOCK_ALIGN}")
    return align


def adpcm_samples_per_block(block_align: int, channels: int = 1) -> int:
    """wSamplesPerBlock: the header's sample and two per byte behind the headers, per channel."""
    return (int(block_align) // int(channels) - 4) * 2 + 1


def check_adpcm_block(samples_per_block) -> int:
    """Samples of a mono block the encoder writes: 8 k + 1 (whole 4-byte groups behind the header), 9 ... 8185."""
    spb = int(samples_per_block)
    if isinstance(samples_per_block, bool) or spb != samples_per_block or spb < 9 or (spb - 1) % 8 or (spb - 1) // 2 + 4 > ADPCM_MAX_BLOCK_ALIGN:
        raise ValueError(f"ADPCM: samples_per_block must be 8 k + 1 in 9 ... {(ADPCM_MAX_BLOCK_ALIGN - 4) * 2 + 1}")
    return spb


def _adpcm_pcm(pcm) -> np.ndarray:
    x = np.asarray(pcm).reshape(-1)
    if x.dtype != np.int16:
        raise ValueError("ADPCM: int16 PCM expected")
    return x


def _adpcm_quantise(x: np.ndarray, s0: np.ndarray, index: np.ndarray, n_real: np.ndarray, keep: bool):
    """lin2adpcm over the last axis of ``x`` [B][T] from the states (s0 [B][1], index [B][K]), all K candidates of all B blocks at once ->
    (sum of (x - p)^2 over each block's first n_real [B][1] samples as int64 [B][K], the codes uint8 [B][K][T] or None)."""
    T = x.shape[1]
    index = index.astype(np.int64)
    pred = np.broadcast_to(s0.astype(np.int64), index.shape)
    err = np.zeros(index.shape, np.int64)
    codes = np.empty(index.shape + (T,), np.uint8) if keep else None
    for t in range(T):
        step = ADPCM_STEPS[index]
        xt = x[:, t:t + 1]
        d = xt - pred
        sign = d < 0
        d = np.abs(d)
        b2 = d >= step
        d = d - b2 * step
        b1 = d >= step >> 1
        d = d - b1 * (step >> 1)
        b0 = d >= step >> 2
        vp = (step >> 3) + b2 * step + b1 * (step >> 1) + b0 * (step >> 2)
        pred = np.clip(np.where(sign, pred - vp, pred + vp), -32768, 32767)
        code = b2 * 4 + b1 * 2 + b0 * 1 + sign * 8
        index = np.clip(index + ADPCM_INDEX[code], 0, 88)
        err = err + (t < n_real) * (xt - pred) ** 2
        if keep:
            codes[..., t] = code
    return err, codes


def adpcm_choose(x, samples_per_block: int):
    """-> (blocks [B][spb] int64 with the padding, the step index of every block's header [B], its error [B])."""
    x, spb = _adpcm_pcm(x), check_adpcm_block(samples_per_block)
    nb = -(-x.size // spb)
    blocks = np.concatenate([x, np.full(nb * spb - x.size, x[-1] if x.size else 0, np.int16)]).reshape(nb, spb).astype(np.int64)
    n_real = np.clip(x.size - np.arange(nb) * spb - 1, 0, spb - 1)[:, None]
    best, best_err = np.zeros(nb, np.int64), np.zeros(nb, np.int64)
    for lo in range(0, nb, 512):                           # 512 blocks x 89 candidates at a time
        b = blocks[lo: lo + 512]
        err = _adpcm_quantise(b[:, 1:], b[:, :1], np.broadcast_to(np.arange(89), (b.shape[0], 89)), n_real[lo: lo + 512], False)[0]
        best[lo: lo + 512] = err.argmin(axis=1)            # the first of equals = the smallest index
        best_err[lo: lo + 512] = err.min(axis=1)
    return blocks, best, best_err


def adpcm_encode_blocks(x, samples_per_block: int) -> np.ndarray:
    """int16 mono PCM -> the uint8 bytes of ceil(n / samples_per_block) blocks of (samples_per_block - 1) / 2 + 4 bytes each (nothing for
    n = 0): the ``data`` chunk of the WAVE file.  The last block is padded with its last real sample."""
    blocks, best, _err = adpcm_choose(x, samples_per_block)
    nb, spb = blocks.shape
    if nb == 0:
        return np.zeros(0, np.uint8)
    codes = _adpcm_quantise(blocks[:, 1:], blocks[:, :1], best[:, None], np.zeros((nb, 1), np.int64), True)[1][:, 0, :]
    out = np.zeros((nb, (spb - 1) // 2 + 4), np.uint8)
    out[:, :2] = blocks[:, 0].astype("<i2").view(np.uint8).reshape(nb, 2)
    out[:, 2] = best
    out[:, 4:] = codes[:, 0::2] | (codes[:, 1::2] << 4)
    return out.reshape(-1)


def _adpcm_expand(codes: np.ndarray, s0: np.ndarray, index: np.ndarray) -> np.ndarray:
    """adpcm2lin over the last axis of the 4-bit ``codes`` [S][T] from the states (s0 [S], index [S]) -> int16 [S][T]."""
    pred, index = s0.astype(np.int64), index.astype(np.int64)
    out = np.empty(codes.shape, np.int16)
    for t in range(codes.shape[1]):
        step, c = ADPCM_STEPS[index], codes[:, t].astype(np.int64)
        vp = (step >> 3) + ((c >> 2) & 1) * step + ((c >> 1) & 1) * (step >> 1) + (c & 1) * (step >> 2)
        pred = np.clip(np.where(c & 8, pred - vp, pred + vp), -32768, 32767)
        index = np.clip(index + ADPCM_INDEX[c], 0, 88)
        out[:, t] = pred
    return out


def adpcm_block_frames(n_bytes: int, channels: int) -> int:
    """Frames the first n_bytes of a block hold: the header's, 8 per whole round of 4-byte groups, and what the LAST channel's group of
    a cut round still holds; 0 when the headers are not whole."""
    ch = int(channels)
    if n_bytes < 4 * ch:
        return 0
    q, rem = divmod(int(n_bytes) - 4 * ch, 4 * ch)
    return 1 + 8 * q + 2 * max(0, rem - 4 * (ch - 1))


def adpcm_frame_count(n_bytes: int, channels: int, block_align: int, fact: Optional[int] = None) -> int:
    """Frames of a data chunk of n_bytes: whole blocks, the trailing part of one, at most what a fact chunk states."""
    full, rem = divmod(int(n_bytes), int(block_align))
    n = full * adpcm_samples_per_block(block_align, channels) + adpcm_block_frames(rem, channels)
    return n if fact is None else min(n, int(fact))


def adpcm_decode_frames(data: bytes, channels: int, block_align: int, fact: Optional[int] = None, data_at: int = 0) -> np.ndarray:
    """The ``data`` bytes of an IMA ADPCM WAVE file -> int16 frames [n][channels], audioop.adpcm2lin per block and channel from the header
    state.  Stereo: one 4-byte header per channel, then groups of 4 bytes (8 samples) alternating left and right.  A step index above 88 in
    any block whose headers are whole is refused, the first one in file order (position = data_at + the byte of that index)."""
    ch, ba = int(channels), int(block_align)
    raw = np.frombuffer(bytes(data), np.uint8)
    full, rem = divmod(raw.size, ba)
    nb = full + (rem >= 4 * ch)
    n = adpcm_frame_count(raw.size, ch, ba, fact)
    if nb == 0:
        return np.zeros((0, ch), np.int16)
    blocks = np.zeros((nb, ba), np.uint8)
    blocks.reshape(-1)[: min(raw.size, nb * ba)] = raw[: nb * ba]
    head = blocks[:, : 4 * ch].reshape(nb, ch, 4)
    bad = np.argwhere(head[:, :, 2] > 88)
    if bad.size:
        b, c = (int(v) for v in bad[0])
        raise WavError(WavStatus.STEP_INDEX, data_at + b * ba + 4 * c + 2)
    s0 = np.ascontiguousarray(head[:, :, :2]).view("<i2").reshape(nb * ch)
    body = blocks[:, 4 * ch:].reshape(nb, -1, ch, 4).transpose(0, 2, 1, 3).reshape(nb * ch, -1)
    codes = np.stack([body & 15, body >> 4], axis=-1).reshape(nb * ch, -1)                    # low nibble first
    pcm = np.concatenate([s0[:, None].astype(np.int16), _adpcm_expand(codes, s0, head[:, :, 2].reshape(-1))], axis=1)
    return np.ascontiguousarray(pcm.reshape(nb, ch, -1).transpose(0, 2, 1).reshape(-1, ch)[:n])


def adpcm_decode_blocks(data, samples_per_block: int, n: Optional[int] = None) -> np.ndarray:
    """The inverse of adpcm_encode_blocks: mono blocks -> int16, the first n samples of them (None = all, padding included)."""
    spb = check_adpcm_block(samples_per_block)
    return adpcm_decode_frames(np.asarray(data, np.uint8).tobytes(), 1, (spb - 1) // 2 + 4, n)[:, 0]


def adpcm_wav(blocks, sample_rate: int, n_samples: Optional[int] = None) -> np.ndarray:
    """The blocks of adpcm_encode_blocks at ``sample_rate`` -> the uint8 bytes of the complete mono WAVE file: format tag 0x11, 4 bits,
    nBlockAlign = adpcm_block_align(rate), cbSize 2 and wSamplesPerBlock, a fact chunk with the true sample count (None = the blocks' own,
    padding included: what a collected stream knows), the data chunk."""
    payload = np.asarray(blocks, np.uint8).reshape(-1).tobytes()
    ba = adpcm_block_align(sample_rate)
    spb = adpcm_samples_per_block(ba)
    if len(payload) % ba:
        raise ValueError(f"ADPCM: whole blocks of {ba} bytes are needed at {sample_rate} Hz")
    n = len(payload) // ba * spb if n_samples is None else int(n_samples)
    if not len(payload) // ba * spb - spb < n <= len(payload) // ba * spb and not (n == 0 and not payload):
        raise ValueError("ADPCM: the sample count does not end in the last block")
    fmt = struct.pack("<HHIIHHHH", ADPCM_WAVE_TAG, 1, int(sample_rate), int(sample_rate) * ba // spb, ba, 4, 2, spb)
    body = b"WAVE" + b"fmt " + struct.pack("<I", len(fmt)) + fmt + b"fact" + struct.pack("<II", 4, n) + b"data" + struct.pack("<I", len(payload)) + payload
    return np.frombuffer(b"RIFF" + struct.pack("<I", len(body)) + body, np.uint8).copy()


def ulaw2lin(codes) -> np.ndarray:
    """uint8 G.711 mu-law -> int16, audioop.ulaw2lin(data, 2) in closed form for all 256 codes."""
    u = ~np.asarray(codes, np.uint8).astype(np.int32) & 0xFF
    t = (((u & 0x0F) << 3) + 0x84) << ((u & 0x70) >> 4)
    return np.where(u & 0x80, 0x84 - t, t - 0x84).astype(np.int16)


def alaw2lin(codes) -> np.ndarray:
    """uint8 G.711 A-law -> int16, audioop.alaw2lin(data, 2) in closed form for all 256 codes."""
    a = np.asarray(codes, np.uint8).astype(np.int32) ^ 0x55
    seg = (a & 0x70) >> 4
    t = ((a & 0x0F) << 4) + np.where(seg == 0, 8, 0x108)
    t = np.where(seg > 1, t << np.maximum(seg - 1, 0), t)
    return np.where(a & 0x80, t, -t).astype(np.int16)


def wav_coded_frame_count(info: "WavInfo") -> int:
    """Frames a coded clip (tag 6, 7 or 0x11) decodes to: what its bytes hold, at most what a fact chunk states."""
    if info.tag == ADPCM_WAVE_TAG:
        return adpcm_frame_count(len(info.data), info.channels, info.block_align, info.fact)
    n = len(info.data) // info.channels
    return n if info.fact is None else min(n, info.fact)


def wav_coded_frames(info: "WavInfo") -> np.ndarray:
    """The int16 frames [n][channels] of a WAVE clip with tag 7 (mu-law), 6 (A-law) or 0x11 (IMA ADPCM): what csrc/vv_adpcm.hip
    (vv_wav_decode) writes on the device.  G.711 has one code per sample; a fact chunk that states fewer frames cuts either."""
    ch = info.channels
    if info.tag == ADPCM_WAVE_TAG:
        return adpcm_decode_frames(info.data, ch, info.block_align, info.fact, info.data_at)
    codes = np.frombuffer(info.data, np.uint8)
    n = codes.size // ch if info.fact is None else min(codes.size // ch, info.fact)
    return np.ascontiguousarray((ulaw2lin if info.tag == 7 else alaw2lin)(codes[: n * ch]).reshape(n, ch))


# ---------------------------------------------------------------------- N15: FLAC output (RFC 9639), fixed predictors, mono, 16 bits
# The arithmetic below IS the specification: csrc/vv_flac.hip makes the same exhaustive, exact choice per frame and packs
# the same bits, so this mirror and the device agree byte for byte, and so does a request alone or in a batch.  Per frame of m samples:
#   constant   if and only if all m samples are equal (24 bits)
#   Fixed(o, po), o = 0 ... min(4, m - 1), po = 0 ... 4 with 2^po | m and (m >> po) > o: the o-th finite difference, Rice coded per
#              partition with the parameter k in 0 ... 14 that gives the fewest bits (the lowest such k):
#              8 + 16 o + 6 + sum over partitions (4 + min_k [count (k + 1) + sum (u >> k)]) bits, u = 2 r (r >= 0), -2 r - 1 (r < 0)
#   verbatim   8 + 16 m bits, only when strictly smaller than every Fixed candidate
# the fewest bits win; ties go to the lower o, then the lower po.  |order-4 difference of int16| < 2^20, so u < 2^21 and k <= 14 always
# suffices: the escape code is never written.  Every frame is independent: header (CRC-8), one subframe, zero bits to the byte, CRC-16.
# N16 (opt-in, ``lpc_order`` 1 ... 12; 0 is all of the above, untouched): LPC(p, po), p = 1 ... min(lpc_order, m - 1), beside the Fixed
# candidates, from flac_lpc_coefficients (integer Welch window and lags, float64 Levinson-Durbin with one rounding per operation, 12-bit
# coefficients): 8 + 16 p + 4 + 5 + 12 p + 6 + the same partition sums over x[n] - ((sum q[j] x[n - j]) >> shift).  The fewest bits win
# among constant / Fixed / LPC / verbatim; ties go to Fixed before LPC, then the lower order, then the lower po.
FLAC_BLOCK = 4096                    # VV_FLAC_BLOCK: samples per frame, the last one of a signal may be shorter
FLAC_MAX_ORDER = 4
FLAC_MAX_PART_ORDER = 4
FLAC_MAX_RICE = 14
FLAC_MAX_RATE = 655350               # 16 bits of tens of Hz in a frame header; STREAMINFO itself has 20 bits of Hz
FLAC_MAX_LPC_ORDER = 12              # ModelConfig.flac_lpc_order: the subset limit of the format at rates up to 48 kHz (N16)
FLAC_LPC_PRECISION = 12              # bits of a quantised predictor coefficient
_FLAC_RATE_CODE = {88200: 1, 176400: 2, 192000: 3, 8000: 4, 16000: 5, 22050: 6, 24000: 7, 32000: 8, 44100: 9, 48000: 10, 96000: 11}


def _crc_table(poly: int, width: int) -> List[int]:
    top, mask, table = 1 << (width - 1), (1 << width) - 1, []
    for b in range(256):
        c = b << (width - 8)
        for _ in range(8):
            c = ((c << 1) ^ poly) & mask if c & top else (c << 1) & mask
        table.append(c)
    return table


_CRC8_TABLE = _crc_table(0x07, 8)
_CRC16_TABLE = _crc_table(0x8005, 16)


def flac_crc8(data: bytes) -> int:
    """CRC-8 of a FLAC frame header: polynomial 0x07, initial value 0, not reflected."""
    c = 0
    for b in bytes(data):
        c = _CRC8_TABLE[c ^ b]
    return c


def flac_crc16(data: bytes) -> int:
    """CRC-16 of a FLAC frame: polynomial 0x8005, initial value 0, not reflected."""
    c = 0
    for b in bytes(data):
        c = ((c << 8) & 0xFFFF) ^ _CRC16_TABLE[(c >> 8) ^ b]
    return c


def flac_frame_bound(m: int) -> int:
    """vv_flac_frame_bound: no frame of m samples is longer -- 15 header bytes at most (4 fixed, 6 of frame number, 2 of block size,
    2 of rate, CRC-8), the subframe header, m verbatim samples, CRC-16."""
    return 15 + 1 + 2 * int(m) + 2 if m >= 1 else 0


def _flac_pcm(pcm) -> np.ndarray:
    x = np.asarray(pcm).reshape(-1)
    if x.dtype != np.int16:
        raise ValueError("FLAC: int16 PCM expected")
    return x


def _check_flac_rate(sample_rate) -> int:
    if isinstance(sample_rate, bool) or int(sample_rate) != sample_rate or not 1 <= int(sample_rate) <= FLAC_MAX_RATE:
        raise ValueError(f"FLAC: a sample rate in 1 ... {FLAC_MAX_RATE} Hz is needed")
    return int(sample_rate)


def check_flac_lpc_order(lpc_order) -> int:
    if isinstance(lpc_order, bool) or not isinstance(lpc_order, (int, np.integer)) or not 0 <= int(lpc_order) <= FLAC_MAX_LPC_ORDER:
        raise ValueError(f"flac_lpc_order must be an integer in 0 ... {FLAC_MAX_LPC_ORDER} (0 = fixed predictors only)")
    return int(lpc_order)


def flac_stream_header(sample_rate: int, total_samples: int, min_frame: int = 0, max_frame: int = 0) -> bytes:
    """The 42 bytes in front of the frames: ``fLaC`` and one STREAMINFO block (the last metadata block): block size 4096 / 4096, the
    smallest and largest frame in bytes (0 = not known), rate, mono, 16 bits, total samples (0 = not known: a stream), and an MD5 of
    zeros, which means "not computed"."""
    sr, n = _check_flac_rate(sample_rate), int(total_samples)
    if not 0 <= n < 1 << 36 or not 0 <= int(min_frame) < 1 << 24 or not 0 <= int(max_frame) < 1 << 24:
        raise ValueError("FLAC: total samples below 2^36 and frame sizes below 2^24 are needed")
    packed = (sr << 44) | (0 << 41) | (15 << 36) | n                       # 20 bits rate, 3 channels - 1, 5 bits - 1, 36 total samples
    return (b"fLaC" + bytes([0x80, 0, 0, 34]) + struct.pack(">HH", FLAC_BLOCK, FLAC_BLOCK) + int(min_frame).to_bytes(3, "big") +
            int(max_frame).to_bytes(3, "big") + packed.to_bytes(8, "big") + bytes(16))


def _flac_utf8(v: int) -> bytes:
    """The frame number in the extended UTF-8 coding: 1 to 6 bytes for up to 31 bits."""
    if v < 0x80:
        return bytes([v])
    n = 2
    while v >= 1 << (5 * n + 1):                                            # 2 bytes hold 11 bits, 3: 16, 4: 21, 5: 26, 6: 31
        n += 1
    lead = (0xFF << (8 - n)) & 0xFF | (v >> (6 * (n - 1)))
    return bytes([lead] + [0x80 | ((v >> (6 * i)) & 0x3F) for i in range(n - 2, -1, -1)])


def _flac_frame_header(m: int, sample_rate: int, number: int) -> bytes:
    code = _FLAC_RATE_CODE.get(sample_rate)
    tail = b""
    if code is None:
        if sample_rate <= 65535:
            code, tail = 13, struct.pack(">H", sample_rate)
        elif sample_rate % 10 == 0:
            code, tail = 14, struct.pack(">H", sample_rate // 10)
        else:
            code = 0                                                        # from STREAMINFO
    bs = 12 if m == FLAC_BLOCK else 7
    head = bytes([0xFF, 0xF8, (bs << 4) | code, 0x08]) + _flac_utf8(number) + (b"" if m == FLAC_BLOCK else struct.pack(">H", m - 1)) + tail
    return head + bytes([flac_crc8(head)])


def _flac_rice(u: np.ndarray, o: int, pmax: int):
    """The Rice search of one predictor: u = the zigzag values of all m positions, zeros at the o warm-up samples.  -> (po, ks, bits) of
    the partition order that needs the fewest bits (the lowest of equals), bits = the 6 of method and order, and per partition 4 and
    the codes under its best k (the lowest of equals); None if no partition order holds more than o samples."""
    m = u.size
    shifts = np.arange(FLAC_MAX_RICE + 1).reshape(-1, 1, 1)
    sums = (u.reshape(1, 1 << pmax, -1) >> shifts).sum(axis=2)              # [k][finest partition]
    best = None
    for po in range(pmax, -1, -1):
        if po < pmax:
            sums = sums[:, 0::2] + sums[:, 1::2]                            # additive over partitions
        if (m >> po) <= o:
            continue
        count = np.full(1 << po, m >> po, np.int64)
        count[0] -= o
        cost = count.reshape(1, -1) * (shifts.reshape(-1, 1) + 1) + sums
        bits = 6 + int((4 + cost.min(axis=0)).sum())
        if best is None or bits <= best[2]:                                 # descending po: the lowest of equals stays
            best = (po, [int(k) for k in cost.argmin(axis=0)], bits)        # the first minimum: the lowest k
    return best


def _flac_zigzag(r: np.ndarray, m: int) -> np.ndarray:
    u = np.zeros(m, np.int64)                                               # the warm-up samples count as u = 0: nothing in any sum
    u[m - r.size:] = np.where(r >= 0, 2 * r, -2 * r - 1)
    return u


def flac_lpc_coefficients(x: np.ndarray, max_order: int):
    """The quantised predictors of one frame: -> {p: (shift, [q1 ... qp])} for the orders 1 ... min(max_order, m - 1)
    that are candidates.  Welch window and autocorrelation in exact integers, Levinson-Durbin in float64 with one rounding per written
    operation (csrc/vv_flac.hip does the same operations in the same order), 12-bit coefficients with the error fed forward."""
    x = np.asarray(x).reshape(-1).astype(np.int64)
    m, out = x.size, {}
    if m < 3 or max_order < 1:
        return out
    h = (m - 1) // 2
    i = np.arange(m, dtype=np.int64)
    xw = x * (((i * (m - 1 - i)) << 10) // (h * ((m - 1) - h)))             # |xw| <= 2^25
    lags = min(int(max_order), m - 1)
    R = [int((xw[: m - lag] * xw[lag:]).sum()) for lag in range(lags + 1)]  # |R| <= 4096 * 2^50: exact in int64
    if R[0] == 0:
        return out
    Rf = [float(v) for v in R]
    a, err = [0.0], Rf[0]                                                   # a[1 ... p]: x[n] ~ sum a[j] x[n - j]
    for p in range(1, lags + 1):
        acc = Rf[p]
        for j in range(1, p):
            acc = acc - a[j] * Rf[p - j]
        k = acc / err
        a = [0.0] + [a[j] - k * a[p - j] for j in range(1, p)] + [k]
        err = err * (1.0 - k * k)
        if not err > 0.0:
            break
        cmax = max(abs(v) for v in a[1:])
        if cmax == 0.0:
            continue
        shift = min(FLAC_LPC_PRECISION - 1 - math.frexp(cmax)[1], 15)
        if shift < 0:
            continue
        fe, q = 0.0, []
        for j in range(1, p + 1):
            fe = fe + math.ldexp(a[j], shift)
            q.append(int(min(max(math.floor(fe + 0.5), -(1 << (FLAC_LPC_PRECISION - 1))), (1 << (FLAC_LPC_PRECISION - 1)) - 1)))
            fe = fe - q[-1]
        out[p] = (shift, q)
    return out


def _flac_lpc_residual(x: np.ndarray, shift: int, q) -> np.ndarray:
    """x[n] - ((sum q[j] x[n - j]) >> shift) for n >= p, x int64: the sum stays below 12 * 2^26, the shift is arithmetic."""
    p, m = len(q), x.size
    pred = np.zeros(m - p, np.int64)
    for j in range(1, p + 1):
        pred += int(q[j - 1]) * x[p - j: m - j]
    return x[p:] - (pred >> shift)


def flac_choose(x: np.ndarray, lpc_order: int = 0):
    """The subframe of one frame: -> (kind, o, po, ks, bits), kind = "constant" | "verbatim" | "fixed", ks = the Rice parameter of each
    of the 2^po partitions, bits = the subframe's exact size.  Exhaustive over (o, po) and, per partition, k.  With ``lpc_order`` 1 ...
    12 (N16) the predictors of flac_lpc_coefficients run as well: kind may be "lpc" and the tuple ends with (shift, [q1 ... qo])."""
    x = np.asarray(x).reshape(-1).astype(np.int64)
    m = x.size
    if m < 1 or m > FLAC_BLOCK:
        raise ValueError(f"a FLAC frame holds 1 ... {FLAC_BLOCK} samples")
    lpc_order = check_flac_lpc_order(lpc_order)
    tail = ((0, []),) if lpc_order else ()
    if (x == x[0]).all():
        return ("constant", 0, 0, [], 24) + tail
    pmax = 0
    while pmax < FLAC_MAX_PART_ORDER and m % (2 << pmax) == 0:
        pmax += 1
    best = None
    for o in range(min(FLAC_MAX_ORDER, m - 1) + 1):
        po, ks, bits = _flac_rice(_flac_zigzag(np.diff(x, n=o), m), o, pmax)
        if best is None or 8 + 16 * o + bits < best[4]:                     # ascending o: the lowest of equals stays
            best = ("fixed", o, po, ks, 8 + 16 * o + bits) + tail
    for p, (shift, q) in sorted(flac_lpc_coefficients(x, lpc_order).items()):
        po, ks, bits = _flac_rice(_flac_zigzag(_flac_lpc_residual(x, shift, q), m), p, pmax)
        bits += 8 + 16 * p + 4 + 5 + FLAC_LPC_PRECISION * p
        if bits < best[4]:                                                  # Fixed before LPC, then the lower order
            best = ("lpc", p, po, ks, bits, (shift, q))
    if 8 + 16 * m < best[4]:
        return ("verbatim", 0, 0, [], 8 + 16 * m) + tail
    return best


def _put(bits: np.ndarray, pos, value, n: int):
    """n bits of each value, most significant first, from bit position pos on."""
    pos, value = np.asarray(pos, np.int64), np.asarray(value, np.int64)
    for b in range(n):
        bits[pos + b] = (value >> (n - 1 - b)) & 1


def flac_encode_frame(x: np.ndarray, sample_rate: int, number: int, lpc_order: int = 0) -> bytes:
    """One complete frame of 1 ... 4096 int16 samples with frame number ``number``; ``lpc_order`` as for flac_choose."""
    x = np.asarray(x).reshape(-1).astype(np.int64)
    m = x.size
    kind, o, po, ks, n_bits, *lpc = flac_choose(x, lpc_order)
    bits = np.zeros(n_bits, np.uint8)
    if kind == "constant":
        _put(bits, 8, x[0] & 0xFFFF, 16)                                    # subframe header 0 000000 0
    elif kind == "verbatim":
        _put(bits, 0, 0x02, 8)
        _put(bits, 8 + 16 * np.arange(m), x & 0xFFFF, 16)
    else:
        _put(bits, 8 + 16 * np.arange(o), x[:o] & 0xFFFF, 16)
        base = 8 + 16 * o
        if kind == "lpc":
            shift, q = lpc[0]
            _put(bits, 0, (32 | (o - 1)) << 1, 8)
            _put(bits, base, FLAC_LPC_PRECISION - 1, 4)
            _put(bits, base + 4, shift, 5)
            _put(bits, base + 9 + FLAC_LPC_PRECISION * np.arange(o), np.asarray(q, np.int64) & ((1 << FLAC_LPC_PRECISION) - 1), FLAC_LPC_PRECISION)
            base += 9 + FLAC_LPC_PRECISION * o
            r = _flac_lpc_residual(x, shift, q)
        else:
            _put(bits, 0, (8 | o) << 1, 8)
            r = np.diff(x, n=o)
        _put(bits, base, po, 6)                                             # coding method 00, partition order
        u = np.where(r >= 0, 2 * r, -2 * r - 1)
        ps = m >> po
        count = np.full(1 << po, ps, np.int64)
        count[0] -= o
        k = np.repeat(np.asarray(ks, np.int64), count)
        first = np.concatenate([[0], np.cumsum(count)[:-1]])                # each partition's first residual carries its parameter
        q = u >> k
        lens = q + 1 + k
        lens[first] += 4
        stop = base + 6 + np.cumsum(lens) - 1 - k                           # the one bit that ends the run of q zeros
        _put(bits, stop[first] - q[first] - 4, np.asarray(ks, np.int64), 4)
        bits[stop] = 1
        for b in range(int(k.max())):
            sel = k > b
            bits[stop[sel] + 1 + b] = (u[sel] >> (k[sel] - 1 - b)) & 1
        assert stop[-1] + k[-1] + 1 == n_bits
    body = _flac_frame_header(m, sample_rate, number) + np.packbits(bits).tobytes()
    return body + struct.pack(">H", flac_crc16(body))


def flac_encode_frames(pcm, sample_rate: int, frame0: int = 0, last: bool = True, lpc_order: int = 0):
    """The frames of an int16 signal, the host mirror of vv_pcm_flac: ceil(n / 4096) frames numbered from ``frame0``,
    back to back.  ``last=False`` = a block of a stream: n must be a multiple of 4096.  ``lpc_order`` 1 ... 12 = the mirror of
    vv_pcm_flac_lpc (N16).  -> (uint8 frames, smallest frame, largest frame in bytes); (empty, 0, 0) for an empty signal."""
    pcm = _flac_pcm(pcm)
    sr, frame0, lpc_order = _check_flac_rate(sample_rate), int(frame0), check_flac_lpc_order(lpc_order)
    n_frames = -(-pcm.size // FLAC_BLOCK)
    if frame0 < 0 or frame0 + n_frames > 1 << 31:
        raise ValueError("FLAC: frame numbers run from 0 to 2^31 - 1")
    if not last and pcm.size % FLAC_BLOCK:
        raise ValueError(f"FLAC: a block that is not the last one holds whole frames of {FLAC_BLOCK} samples")
    frames = [flac_encode_frame(pcm[f * FLAC_BLOCK: (f + 1) * FLAC_BLOCK], sr, frame0 + f, lpc_order) for f in range(n_frames)]
    if not frames:
        return np.zeros(0, np.uint8), 0, 0
    return np.frombuffer(b"".join(frames), np.uint8).copy(), min(map(len, frames)), max(map(len, frames))


# ---------------------------------------------------------------------- N17: FLAC input (RFC 9639), the whole format at 8 / 16 / 24 bits
# The arithmetic below IS the specification: csrc/vv_flac_decode.hip runs the same checks in the same order, so this
# mirror and the device give the same samples for a valid stream and the same reason code and byte position for a malformed one.
#   container : optional ID3v2 tag, ``fLaC``, metadata blocks (STREAMINFO first, once; every other block skipped by its length)
#   chain     : frame 0 starts at the first byte after the metadata, every next frame at the byte after the previous CRC-16; a sync
#               pattern anywhere else is not a frame.  A known total ends the chain (bytes behind it are ignored) and must be met
#               exactly; with total 0 the chain must end exactly at the end of the data
#   header    : checked in this order -- sync, reserved bits and codes, syntax of the coded number (1 ... 7 bytes, its value is ignored),
#               the optional block-size / rate fields, CRC-8, then agreement with STREAMINFO (channels, depth, rate, block <= max block)
#               and with the first frame's blocking bit
#   measure   : the subframes are walked without restoring them (types, wasted bits, orders, precision, shift, partitions, Rice codes),
#               then zero padding to the byte and the CRC-16.  The walk reads nothing at or past min(end of data, frame start +
#               flac_decode_frame_bound): a read across that limit gives zeros and ends the frame with "overrun" (the data ended) or
#               "frame too long" (the bound did)
#   restore   : after EVERY frame of the chain has passed the above: 64-bit sums, arithmetic shift, every restored sample must fit its
#               subframe's depth less the wasted bits ("sample out of range"), then the wasted bits are shifted back
#   channels  : left/side, side/right, mid/side in integers; a result wraps to the stream's width as an integer cast does
# A refusal's position is the first byte of the frame that holds the problem (for a chain problem: where the next frame was expected).
# The MD5 of STREAMINFO is not verified.
FLAC_MAX_CLIP = 1 << 26              # VV_FLAC_MAX_CLIP: samples per channel of one decoded clip


class FlacStatus:
    """Reason codes of a refused FLAC stream: one enum for this mirror and csrc/vv_flac_decode.hip (VV_FLAC_* in include/vvtts.h)."""
    OK, BAD_HEADER, CRC8, CRC16, RESERVED, PARTITION, RANGE, OVERRUN, CHAIN, FRAME_TOO_LONG, CLIP_TOO_LONG = range(11)
    NAMES = ("ok", "bad header", "header CRC-8 mismatch", "frame CRC-16 mismatch", "reserved code", "partition misfit",
             "sample out of range", "overrun", "chain / total mismatch", "frame too long", "clip too long")


class FlacError(ValueError):
    """``malformed FLAC: <reason> at byte <position>``; ``code`` is a FlacStatus, ``position`` a byte offset into the data given."""

    def __init__(self, code: int, position: int, detail: str = ""):
        self.code, self.position = int(code), int(position)
        super().__init__(f"malformed FLAC: {detail or FlacStatus.NAMES[self.code]} at byte {self.position}")


class FlacInfo(NamedTuple):
    min_block: int
    max_block: int
    rate: int
    channels: int
    bits: int
    total: int                       # samples per channel, 0 = unknown
    start: int                       # the byte at which the frames start


def flac_container(data: bytes) -> FlacInfo:
    """Byte parsing only: ID3v2 tag (skipped by its sync-safe size), ``fLaC``, the metadata blocks.  The MD5 is not read."""
    data, pos = bytes(data), 0
    if data[:3] == b"ID3":
        if len(data) < 10 or any(b & 0x80 for b in data[6:10]):
            raise FlacError(FlacStatus.BAD_HEADER, 0, "truncated or malformed ID3v2 tag")
        pos = 10 + ((data[6] << 21) | (data[7] << 14) | (data[8] << 7) | data[9]) + (10 if data[5] & 0x10 else 0)
    if data[pos:pos + 4] != b"fLaC":
        raise FlacError(FlacStatus.BAD_HEADER, pos, "no fLaC marker")
    pos, info, last = pos + 4, None, False
    while not last:
        if pos + 4 > len(data):
            raise FlacError(FlacStatus.BAD_HEADER, pos, "truncated metadata block")
        last, kind, size = bool(data[pos] & 0x80), data[pos] & 0x7F, int.from_bytes(data[pos + 1:pos + 4], "big")
        if pos + 4 + size > len(data):
            raise FlacError(FlacStatus.BAD_HEADER, pos, "truncated metadata block")
        if (kind == 0) != (info is None) or (kind == 0 and size != 34):
            raise FlacError(FlacStatus.BAD_HEADER, pos, "STREAMINFO must be the first metadata block, 34 bytes, once")
        if kind == 0:
            b = data[pos + 4:pos + 38]
            packed = int.from_bytes(b[10:18], "big")
            info = (int.from_bytes(b[0:2], "big"), int.from_bytes(b[2:4], "big"), packed >> 44, ((packed >> 41) & 7) + 1,
                    ((packed >> 36) & 31) + 1, packed & ((1 << 36) - 1), pos)
        pos += 4 + size
    lo, hi, rate, ch, bits, total, at = info
    if rate == 0:
        raise FlacError(FlacStatus.BAD_HEADER, at, "sample rate 0")
    if bits not in (8, 16, 24):
        raise FlacError(FlacStatus.BAD_HEADER, at, f"{bits} bits per sample (8, 16 and 24 are decoded)")
    if lo > hi or hi < 16:
        raise FlacError(FlacStatus.BAD_HEADER, at, "block sizes (min <= max, max >= 16)")
    if total > FLAC_MAX_CLIP:
        raise FlacError(FlacStatus.CLIP_TOO_LONG, at)
    return FlacInfo(lo, hi, rate, ch, bits, total, pos)


def flac_decode_frame_bound(block: int, channels: int, bits: int) -> int:
    """vv_flac_decode_frame_bound: the longest frame the decoder follows -- twice the verbatim frame (16 header bytes, per channel a
    subframe header and ``block`` samples of bits + 1, CRC-16) plus 64.  No encoder emits more than verbatim."""
    return 2 * (16 + int(channels) * (2 + (int(block) * (int(bits) + 1) + 7) // 8) + 2) + 64


_FLAC_DEPTH_OF_CODE = {1: 8, 2: 12, 4: 16, 5: 20, 6: 24, 7: 32}
_FLAC_RATE_OF_CODE = {v: k for k, v in _FLAC_RATE_CODE.items()}
_FLAC_FIXED = ((), (1,), (2, -1), (3, -3, 1), (4, -6, 4, -1))


def _flac_header(data: bytes, p: int, end: int, info: FlacInfo, blocking: int):
    """The frame header expected at byte p: -> (status, header bytes with the CRC-8, block size, channel assignment code)."""
    S = FlacStatus
    if p + 4 > end:
        return S.OVERRUN, 0, 0, 0
    b1, b2, b3 = data[p + 1], data[p + 2], data[p + 3]
    if data[p] != 0xFF or (b1 & 0xFC) != 0xF8:
        return S.BAD_HEADER, 0, 0, 0
    bsc, rc, cc, dc = b2 >> 4, b2 & 15, b3 >> 4, (b3 >> 1) & 7
    if (b1 & 2) or bsc == 0 or rc == 15 or cc > 10 or dc == 3 or (b3 & 1):
        return S.RESERVED, 0, 0, 0
    q = p + 4
    if q + 1 > end:
        return S.OVERRUN, 0, 0, 0
    lead, n = data[q], 0
    while n < 8 and lead & (0x80 >> n):
        n += 1
    if n == 1 or n == 8:
        return S.BAD_HEADER, 0, 0, 0
    n = max(n, 1)
    if q + n > end:
        return S.OVERRUN, 0, 0, 0
    if any((data[q + i] & 0xC0) != 0x80 for i in range(1, n)):
        return S.BAD_HEADER, 0, 0, 0
    q += n
    extra = 1 if bsc == 6 else 2 if bsc == 7 else 0
    if q + extra > end:
        return S.OVERRUN, 0, 0, 0
    v = int.from_bytes(data[q:q + extra], "big")
    q += extra
    if bsc == 7 and v == 65535:
        return S.RESERVED, 0, 0, 0
    bs = 192 if bsc == 1 else 576 << (bsc - 2) if bsc <= 5 else v + 1 if bsc <= 7 else 256 << (bsc - 8)
    extra = 1 if rc == 12 else 2 if rc in (13, 14) else 0
    if q + extra > end:
        return S.OVERRUN, 0, 0, 0
    v = int.from_bytes(data[q:q + extra], "big")
    q += extra
    rate = info.rate if rc == 0 else v * 1000 if rc == 12 else v if rc == 13 else v * 10 if rc == 14 else _FLAC_RATE_OF_CODE[rc]
    if q + 1 > end:
        return S.OVERRUN, 0, 0, 0
    if flac_crc8(data[p:q]) != data[q]:
        return S.CRC8, 0, 0, 0
    if ((cc + 1 if cc < 8 else 2) != info.channels or (dc and _FLAC_DEPTH_OF_CODE[dc] != info.bits) or rate != info.rate
            or (b1 & 1) != blocking or bs > info.max_block):
        return S.BAD_HEADER, 0, 0, 0
    return S.OK, q + 1 - p, bs, cc


class _FlacBits:
    """The bit reader both sides share: nothing at or past ``limit`` (in bits) is read; a read across it gives zeros and sets ``over``."""

    def __init__(self, data: bytes, pos: int, limit: int):
        self.data, self.pos, self.limit, self.over = data, pos, limit, False

    def take(self, n: int) -> int:                     # n <= 32
        pos = self.pos
        self.pos = pos + n
        if pos + n > self.limit:
            self.over = True
            return 0
        if n == 0:
            return 0
        hi = (pos + n + 7) >> 3
        return (int.from_bytes(self.data[pos >> 3:hi], "big") >> (8 * hi - pos - n)) & ((1 << n) - 1)

    def signed(self, n: int) -> int:
        v = self.take(n)
        return v - (1 << n) if n and v >> (n - 1) else v

    def skip(self, n: int):
        self.pos += n
        if self.pos > self.limit:
            self.over = True

    def unary(self) -> int:
        n = 0
        while True:
            avail = min(32, self.limit - self.pos)
            if avail <= 0:
                self.over = True
                return n
            pos = self.pos
            hi = (pos + avail + 7) >> 3
            v = (int.from_bytes(self.data[pos >> 3:hi], "big") >> (8 * hi - pos - avail)) & ((1 << avail) - 1)
            if v:
                lz = avail - v.bit_length()
                self.pos = pos + lz + 1
                return n + lz
            n += avail
            self.pos = pos + avail


def _flac_subframe(r: _FlacBits, bs: int, depth: int, restore: bool):
    """One subframe at the reader's position.  restore = False: walk it (-> status, None); True: restore it (-> status, samples)."""
    S = FlacStatus
    h = r.take(8)
    if r.over:
        return S.OVERRUN, None
    if h & 0x80:
        return S.RESERVED, None
    t, w = (h >> 1) & 63, 0
    if h & 1:
        w = r.unary() + 1
        if r.over:
            return S.OVERRUN, None
    if w >= depth:
        return S.RESERVED, None
    de, out = depth - w, None
    lo, hi = -(1 << (de - 1)), (1 << (de - 1)) - 1
    if t == 0:
        if restore:
            out = [r.signed(de)] * bs
        else:
            r.skip(de)
    elif t == 1:
        if restore:
            out = [r.signed(de) for _ in range(bs)]
        else:
            r.skip(de * bs)
    elif 8 <= t <= 12 or t >= 32:
        lpc = t >= 32
        o = (t & 31) + 1 if lpc else t - 8
        if o > bs:
            return S.PARTITION, None
        if restore:
            out = [r.signed(de) for _ in range(o)]
        else:
            r.skip(o * de)
        if r.over:
            return S.OVERRUN, None
        coef, shift = _FLAC_FIXED[0 if lpc else o], 0
        if lpc:
            pq = r.take(9)
            if r.over:
                return S.OVERRUN, None
            prec, shift = (pq >> 5) + 1, pq & 15
            if prec == 16 or pq & 16:
                return S.RESERVED, None
            if restore:
                coef = [r.signed(prec) for _ in range(o)]
            else:
                r.skip(o * prec)
            if r.over:
                return S.OVERRUN, None
        m = r.take(6)
        if r.over:
            return S.OVERRUN, None
        method, po = m >> 4, m & 15
        if method > 1:
            return S.RESERVED, None
        if bs & ((1 << po) - 1) or (bs >> po) < o:
            return S.PARTITION, None
        pb = 4 + method
        for part in range(1 << po):
            n = (bs >> po) - (o if part == 0 else 0)
            k = r.take(pb)
            if r.over:
                return S.OVERRUN, None
            raw = -1
            if k == (1 << pb) - 1:
                raw = r.take(5)
                if r.over:
                    return S.OVERRUN, None
                if not restore:
                    r.skip(n * raw)
                    n = 0
            for _ in range(n):
                if raw >= 0:
                    res = r.signed(raw)
                else:
                    u = r.unary()
                    if restore:
                        u = (u << k) | r.take(k)
                        res = (u >> 1) ^ -(u & 1)
                    else:
                        r.skip(k)
                if r.over:
                    return S.OVERRUN, None
                if restore:
                    i, pred = len(out), 0
                    for j, c in enumerate(coef):
                        pred += c * out[i - 1 - j]
                    v = (pred >> shift) + res
                    if v < lo or v > hi:
                        return S.RANGE, None
                    out.append(v)
            if r.over:
                return S.OVERRUN, None
    else:
        return S.RESERVED, None
    if r.over:
        return S.OVERRUN, None
    if restore and w:
        out = [v << w for v in out]
    return S.OK, out


def _flac_depth(info: FlacInfo, assign: int, c: int) -> int:
    return info.bits + (1 if (assign == 8 and c == 1) or (assign == 9 and c == 0) or (assign == 10 and c == 1) else 0)


def _flac_measure(data: bytes, p: int, end: int, info: FlacInfo, hlen: int, bs: int, assign: int):
    """The frame at byte p behind its header: -> (status, the byte after its CRC-16, the subframes' first bits counted from p)."""
    S = FlacStatus
    bound = p + flac_decode_frame_bound(bs, info.channels, info.bits)
    over = S.FRAME_TOO_LONG if bound <= end else S.OVERRUN
    r = _FlacBits(data, 8 * (p + hlen), 8 * min(bound, end))
    subs = []
    for c in range(info.channels):
        subs.append(r.pos - 8 * p)
        st, _ = _flac_subframe(r, bs, _flac_depth(info, assign, c), False)
        if st:
            return (over if st == S.OVERRUN else st), 0, subs
    pad = r.take(-r.pos % 8)
    if r.over:
        return over, 0, subs
    if pad:
        return S.RESERVED, 0, subs
    crc = r.take(16)
    if r.over:
        return over, 0, subs
    e = r.pos >> 3
    if flac_crc16(data[p:e - 2]) != crc:
        return S.CRC16, 0, subs
    return S.OK, e, subs


def flac_frame_index(data: bytes, info: FlacInfo):
    """The chain of frames: -> [(byte, block size, channel assignment, subframe bits)], samples per channel.  Raises FlacError."""
    S = FlacStatus
    data, p, end, samples, frames = bytes(data), info.start, len(data), 0, []
    blocking = data[p + 1] & 1 if p + 1 < end else 0
    while not (info.total and samples == info.total):
        if p == end:
            if info.total:
                raise FlacError(S.CHAIN, p)
            break
        st, hlen, bs, assign = _flac_header(data, p, end, info, blocking)
        if st:
            raise FlacError(st, p)
        st, e, subs = _flac_measure(data, p, end, info, hlen, bs, assign)
        if st:
            raise FlacError(st, p)
        if samples + bs > FLAC_MAX_CLIP:
            raise FlacError(S.CLIP_TOO_LONG, p)
        if info.total and samples + bs > info.total:
            raise FlacError(S.CHAIN, p)
        frames.append((p, bs, assign, subs))
        samples += bs
        p = e
    return frames, samples


def flac_pcm_layout(planes: np.ndarray, bits: int) -> np.ndarray:
    """(n, channels) int64 samples of ``bits`` -> what ``_decode_wav`` holds for the same PCM: int8, int16, or int32 with the sample in
    the upper three bytes and the sign pad in the lowest.  A value outside the depth wraps, as an integer cast does."""
    if bits == 8:
        return planes.astype(np.int8)
    if bits == 16:
        return planes.astype(np.int16)
    v = planes & 0xFFFFFF
    return ((v << 8) | np.where(v & 0x800000, 0xFF, 0)).astype(np.uint32).view(np.int32)


def flac_decode(data: bytes) -> Tuple[np.ndarray, int, int]:
    """FLAC bytes -> (frames (n, channels) int8 | int16 | int32, sample width in bytes, rate): the triple ``_decode_wav`` gives for the
    WAV of the same PCM, so that decode(flac of x) == decode(wav of x) element for element.  The specification of vv_flac_index /
    vv_flac_decode, in Python integers.  The MD5 of STREAMINFO is NOT verified.  What pydub + ffmpeg would hold for a
    24-bit FLAC cannot be pinned offline (as for 24-bit WAV: the module docstring).  Raises FlacError (a ValueError)."""
    data = bytes(data)
    info = flac_container(data)
    frames, samples = flac_frame_index(data, info)
    out = np.zeros((samples, info.channels), np.int64)
    at = 0
    for p, bs, assign, subs in frames:
        ch = []
        for c in range(info.channels):
            st, x = _flac_subframe(_FlacBits(data, 8 * p + subs[c], 8 * len(data)), bs, _flac_depth(info, assign, c), True)
            if st:
                raise FlacError(st, p)
            ch.append(np.array(x, np.int64))
        if assign == 8:
            ch[1] = ch[0] - ch[1]
        elif assign == 9:
            ch[0] = ch[0] + ch[1]
        elif assign == 10:
            mid = (ch[0] << 1) | (ch[1] & 1)
            ch[0], ch[1] = (mid + ch[1]) >> 1, (mid - ch[1]) >> 1
        out[at:at + bs] = np.stack(ch, axis=1)
        at += bs
    return np.ascontiguousarray(flac_pcm_layout(out, info.bits)), {8: 1, 16: 2, 24: 4}[info.bits], info.rate


def is_flac(data: bytes) -> bool:
    return data[:4] == b"fLaC" or data[:3] == b"ID3"


# ---------------------------------------------------------------------- N12: loudness normalisation (ITU-R BS.1770-4 integrated, gated)
# The arithmetic below IS the specification: the device kernels (csrc/vv_loudness.hip) compute the same float64
# operations in the same order, so this mirror and the device agree bit for bit, and so does a request alone or in a batch.
LOUD_RUN = 128                       # VV_LOUD_RUN: samples per independent run of the recurrence, counted from a sub-block's first sample
LOUD_TABLE_DOUBLES = 43              # b1[3] a1[2] | b2[3] a2[2] | M_full[4][4] | M_last[4][4] | ABS
LOUDNESS_RANGE = (-60.0, -5.0)       # accepted targets, LUFS
PEAK_DBFS_RANGE = (-20.0, 0.0)       # accepted sample-peak ceilings, dBFS
_LOUD_TABLES = {}


def check_loudness(loudness, peak_dbfs=-1.0):
    """Validate a loudness target (LUFS, None = off) and a sample-peak ceiling (dBFS): -> (float or None, float)."""
    if loudness is not None:
        if isinstance(loudness, bool) or not isinstance(loudness, (int, float, np.integer, np.floating)):
            raise ValueError("output_loudness must be a number of LUFS or None")
        loudness = float(loudness)
        if not LOUDNESS_RANGE[0] <= loudness <= LOUDNESS_RANGE[1]:             # NaN fails both comparisons
            raise ValueError("output_loudness must be between -60 and -5 LUFS")
    if isinstance(peak_dbfs, bool) or not isinstance(peak_dbfs, (int, float, np.integer, np.floating)):
        raise ValueError("output_peak_dbfs must be a number of dBFS")
    peak_dbfs = float(peak_dbfs)
    if not PEAK_DBFS_RANGE[0] <= peak_dbfs <= PEAK_DBFS_RANGE[1]:
        raise ValueError("output_peak_dbfs must be between -20 and 0 dBFS")
    return loudness, peak_dbfs


def k_weighting(sr: int):
    """(b1, a1, b2, a2) of the K-weighting at ``sr`` Hz: the shelf and the high-pass of BS.1770 from their analogue prototypes through the
    bilinear transform (a = [a1, a2] without the leading 1).  At 48 kHz this is the Recommendation's table to 14 digits."""
    sr = int(sr)
    f0, G, Q = 1681.974450955533, 3.999843853973347, 0.7071752369554196
    K = np.tan(np.pi * f0 / sr)
    Vh = np.power(10.0, G / 20.0)
    Vb = np.power(Vh, 0.4996667741545416)
    a0 = 1.0 + K / Q + K * K
    b1 = np.array([(Vh + Vb * K / Q + K * K) / a0, 2.0 * (K * K - Vh) / a0, (Vh - Vb * K / Q + K * K) / a0], np.float64)
    a1 = np.array([2.0 * (K * K - 1.0) / a0, (1.0 - K / Q + K * K) / a0], np.float64)
    f0, Q = 38.13547087602444, 0.5003270373238773
    K = np.tan(np.pi * f0 / sr)
    a0 = 1.0 + K / Q + K * K
    b2 = np.array([1.0, -2.0, 1.0], np.float64)
    a2 = np.array([2.0 * (K * K - 1.0) / a0, (1.0 - K / Q + K * K) / a0], np.float64)
    return b1, a1, b2, a2


def _loud_step(u, s, b1, a1, b2, a2):
    """One sample of the two biquads, direct form II transposed; u and the four states are arrays over runs.  Every product and sum is
    rounded separately (numpy never fuses), in the order of the specification.  -> (y2, new states)."""
    s0, s1, s2, s3 = s
    y1 = b1[0] * u + s0
    n0 = (b1[1] * u - a1[0] * y1) + s1
    n1 = b1[2] * u - a1[1] * y1
    y2 = b2[0] * y1 + s2
    n2 = (b2[1] * y1 - a2[0] * y2) + s3
    n3 = b2[2] * y1 - a2[1] * y2
    return y2, (n0, n1, n2, n3)


def _loud_run_lengths(sub: int):
    """(runs per sub-block, length of the last one): 2400 = 18 * 128 + 96 -> (19, 96)."""
    rps = -(-int(sub) // LOUD_RUN)
    return rps, int(sub) - (rps - 1) * LOUD_RUN


def loudness_tables(sr: int) -> np.ndarray:
    """The float64 table the device reads (LOUD_TABLE_DOUBLES values): coefficients, M_full, M_last (row major; column j = the state
    after a run's length of zero input from unit state j, computed with the step above), ABS = 10^((-70 + 0.691) / 10)."""
    sr = int(sr)
    if sr not in _LOUD_TABLES:
        if sr < 10 * LOUD_RUN or sr % 10:
            raise ValueError(f"loudness: the sample rate must be a multiple of 10 Hz and at least {10 * LOUD_RUN} Hz, got {sr}")
        b1, a1, b2, a2 = k_weighting(sr)
        _rps, last = _loud_run_lengths(sr // 10)

        def transition(length):
            s = tuple(np.eye(4, dtype=np.float64)[i].copy() for i in range(4))      # s[i][j] = state i when started from unit state j
            zero = np.zeros(4, np.float64)
            for _ in range(length):
                _y, s = _loud_step(zero, s, b1, a1, b2, a2)
            return np.stack(s)                                                     # [i][j]

        t = np.concatenate([b1, a1, b2, a2, transition(LOUD_RUN).reshape(-1), transition(last).reshape(-1),
                            [np.power(10.0, (-70.0 + 0.691) / 10.0)]]).astype(np.float64)
        assert t.size == LOUD_TABLE_DOUBLES
        t.setflags(write=False)
        _LOUD_TABLES[sr] = t
    return _LOUD_TABLES[sr]


def loudness_target(target) -> float:
    """T = 10^((target + 0.691) / 10): the mean square a signal of ``target`` LUFS has after K-weighting; 0 = measure only."""
    return 0.0 if target is None else float(np.power(10.0, (float(target) + 0.691) / 10.0))


def loudness_ceiling(peak_dbfs: float) -> float:
    """c = 32767 * 10^(peak_dbfs / 20): the largest sample magnitude the gain may produce."""
    return float(32767.0 * np.power(10.0, float(peak_dbfs) / 20.0))


def loudness_gate(q, sub: int):
    """Gated mean of BS.1770 from the sub-block sums q_j (100 ms each, ``sub`` samples), linear domain only: 400 ms blocks
    z_j = (((q_j + q_j+1) + q_j+2) + q_j+3) / (4 sub); absolute gate z > ABS; relative gate z > 0.1 * mean of those; both strict.
    Every mean is a sequential ascending sum over a count.  -> (zbar, kept); (0.0, 0) when nothing is kept."""
    q = np.asarray(q, np.float64).reshape(-1)
    if q.size < 4:
        return 0.0, 0
    z = (((q[:-3] + q[1:-2]) + q[2:-1]) + q[3:]) / np.float64(4 * int(sub))
    ABS = np.power(10.0, (-70.0 + 0.691) / 10.0)
    a = z[z > ABS]
    if a.size == 0:
        return 0.0, 0
    gamma = 0.1 * (np.cumsum(a)[-1] / np.float64(a.size))            # np.cumsum accumulates strictly in order
    k = a[a > gamma]
    if k.size == 0:
        return 0.0, 0
    return float(np.cumsum(k)[-1] / np.float64(k.size)), int(k.size)


def _loud_subblock_sums(x: np.ndarray, sr: int) -> np.ndarray:
    """q_j of the complete 100 ms sub-blocks of int16 ``x`` by the run decomposition of the specification (passes A, B, C)."""
    t = loudness_tables(sr)
    b1, a1, b2, a2 = t[0:3], t[3:5], t[5:8], t[8:10]
    M = (t[10:26].reshape(4, 4), t[26:42].reshape(4, 4))
    sub = int(sr) // 10
    rps, last = _loud_run_lengths(sub)
    J = x.size // sub
    if J == 0:
        return np.zeros(0, np.float64)
    u = (x[: J * sub].astype(np.float64) / 32768.0).reshape(J, sub)
    full = u[:, : (rps - 1) * LOUD_RUN].reshape(J, rps - 1, LOUD_RUN)              # the full runs and the last run of every sub-block
    tail = u[:, (rps - 1) * LOUD_RUN:]

    def run(block, s, power):
        """block [..., L]; s = four arrays [...]; -> (end states, sum of y2^2 in sample order)."""
        p = np.zeros(block.shape[:-1], np.float64)
        for i in range(block.shape[-1]):
            y2, s = _loud_step(block[..., i], s, b1, a1, b2, a2)
            if power:
                p = p + y2 * y2
        return s, p

    z4 = lambda shape: tuple(np.zeros(shape, np.float64) for _ in range(4))
    Ef, _ = run(full, z4(full.shape[:-1]), False)                                  # pass A: zero-state end states
    El, _ = run(tail, z4((J,)), False)
    E = np.empty((J, rps, 4), np.float64)
    for i in range(4):
        E[:, : rps - 1, i] = Ef[i]
        E[:, rps - 1, i] = El[i]
    E = E.reshape(J * rps, 4)
    S0 = np.empty_like(E)                                                          # pass B: every run's start state, in ascending run order
    S = np.zeros(4, np.float64)
    for r in range(J * rps):
        S0[r] = S
        m = M[1] if r % rps == rps - 1 else M[0]
        S = ((((m[:, 0] * S[0] + m[:, 1] * S[1]) + m[:, 2] * S[2]) + m[:, 3] * S[3]) + E[r])
    S0 = S0.reshape(J, rps, 4)
    _, pf = run(full, tuple(S0[:, : rps - 1, i] for i in range(4)), True)          # pass C: from the true start states
    _, pl = run(tail, tuple(S0[:, rps - 1, i] for i in range(4)), True)
    q = np.zeros(J, np.float64)
    for k in range(rps - 1):                                                       # ascending sum of the sub-block's runs
        q = q + pf[:, k]
    return q + pl


def _as_pcm16(pcm) -> np.ndarray:
    x = np.asarray(pcm).reshape(-1)
    if x.dtype != np.int16:
        raise ValueError("loudness: int16 PCM expected")
    return x


def measure_loudness(pcm, sr: int):
    """Integrated loudness of int16 ``pcm`` at ``sr`` Hz (BS.1770-4 gating, K-weighting by the bilinear transform at ``sr``; the incomplete
    last 100 ms are not measured).  -> (L in LUFS or -inf when no block is kept, zbar, kept, sample peak max |x|)."""
    x = _as_pcm16(pcm)
    zbar, kept = loudness_gate(_loud_subblock_sums(x, sr), int(sr) // 10)
    peak = int(np.abs(x.astype(np.int32)).max(initial=0))
    return (float(-0.691 + 10.0 * np.log10(zbar)) if kept else float("-inf")), zbar, kept, peak


def loudness_gain(zbar: float, kept: int, peak: int, T: float, c: float) -> float:
    """The gain of the specification: sqrt(T / zbar), limited so that peak * g <= c; exactly 1 when nothing is kept, T <= 0 or peak == 0."""
    if kept < 1 or not T > 0.0 or peak == 0:
        return 1.0
    g = np.sqrt(np.float64(T) / np.float64(zbar))
    if np.float64(peak) * g > np.float64(c):
        g = np.float64(c) / np.float64(peak)
    return float(g)


def normalize_loudness(pcm, sr: int, target, peak_dbfs: float = -1.0, limiter=None) -> np.ndarray:
    """int16 ``pcm`` scaled to ``target`` LUFS under a sample-peak ceiling of ``peak_dbfs``: the host mirror of vv_pcm_loudness, bit for
    bit.  y = clamp(rint(x * g)) in float64, ties to even; target None = a copy.  ``limiter`` = "sample" | "true" (N13): the gain is NOT
    capped by the peak; the look-ahead limiter (limit_peaks) holds the ceiling instead, so a peaky voice reaches the target too."""
    x = _as_pcm16(pcm)
    _L, zbar, kept, peak = measure_loudness(x, sr)
    if limiter is not None:
        return limit_peaks(x, sr, peak_dbfs, limiter, gain=limiter_pregain(zbar, kept, peak, loudness_target(target)))[0]
    g = loudness_gain(zbar, kept, peak, loudness_target(target), loudness_ceiling(peak_dbfs))
    return np.clip(np.rint(x.astype(np.float64) * np.float64(g)), -32768.0, 32767.0).astype(np.int16)


# ---------------------------------------------------------------------- N13: look-ahead peak limiter (sample or 4x oversampled true peak)
# As with N12 the arithmetic below IS the specification and csrc/vv_limiter.hip computes the same float64 operations in
# the same order.  Every quantity is a finite-window function of the input (a sliding minimum and a window average, no recursion), so a
# sample's value depends on the 2L + H samples on either side only: alone, in a batch or cut into stream blocks it is the same.
LIMIT_H = 12                         # VV_LIMIT_H: half length of the 4x interpolator in input samples (24 taps per phase)
LIMIT_MAX_L = 1024                   # VV_LIMIT_MAX_L: the largest look-ahead in samples
LIMITER_LOOKAHEAD_S = 0.005          # look-ahead in seconds: L = round(sr * 0.005) = 120 samples at 24 kHz
LIMITER_MODES = ("sample", "true")   # mode 0 / 1 of vv_pcm_limit
_LIMIT_TAPS = []
_LIMIT_WINDOWS = {}


def check_limiter(mode):
    """Validate ``output_limiter``: None (off), "sample" or "true".  -> the value."""
    if mode is not None and (not isinstance(mode, str) or mode not in LIMITER_MODES):
        raise ValueError('output_limiter must be None, "sample" or "true"')
    return mode


def limiter_lookahead(sr: int) -> int:
    """L = round(sr * LIMITER_LOOKAHEAD_S) samples, which must lie in 1 ... LIMIT_MAX_L."""
    L = int(round(int(sr) * LIMITER_LOOKAHEAD_S))
    if not 1 <= L <= LIMIT_MAX_L:
        raise ValueError(f"limiter: a look-ahead of {LIMITER_LOOKAHEAD_S} s at {sr} Hz is {L} samples, outside 1 ... {LIMIT_MAX_L}")
    return L


def _check_lookahead(L) -> int:
    if isinstance(L, bool) or not isinstance(L, (int, np.integer)) or not 1 <= int(L) <= LIMIT_MAX_L:
        raise ValueError(f"limiter: the look-ahead L must be an integer in 1 ... {LIMIT_MAX_L}")
    return int(L)


def limiter_taps() -> np.ndarray:
    """h[k + 4H] = sinc(k / 4) * kaiser(8H + 1, 8.0)[k + 4H], k = -4H ... 4H: the 4x interpolator (8H + 1 float64; phase 0 is the sample
    itself).  The device reads this table and never recomputes it."""
    if not _LIMIT_TAPS:
        k = np.arange(-4 * LIMIT_H, 4 * LIMIT_H + 1, dtype=np.float64)
        h = (np.sinc(k / 4.0) * np.kaiser(8 * LIMIT_H + 1, 8.0)).astype(np.float64)
        h.setflags(write=False)
        _LIMIT_TAPS.append(h)
    return _LIMIT_TAPS[0]


def limiter_window(L: int) -> np.ndarray:
    """w[k] = 0.5 (1 + cos(pi k / (L + 1))), k = -L ... L, divided by its numpy sum (2L + 1 float64): the average of step 5."""
    L = _check_lookahead(L)
    if L not in _LIMIT_WINDOWS:
        k = np.arange(-L, L + 1, dtype=np.float64)
        w = 0.5 * (1.0 + np.cos(np.pi * k / np.float64(L + 1)))
        w = (w / w.sum()).astype(np.float64)
        w.setflags(write=False)
        _LIMIT_WINDOWS[L] = w
    return _LIMIT_WINDOWS[L]


def limiter_pregain(zbar: float, kept: int, peak: int, T: float) -> float:
    """The pre-gain of the limiter under a loudness target: sqrt(T / zbar), NOT capped by the peak; exactly 1 when nothing is kept,
    T <= 0 or peak == 0."""
    if kept < 1 or not T > 0.0 or peak == 0:
        return 1.0
    return float(np.sqrt(np.float64(T) / np.float64(zbar)))


def limiter_gains(pcm, c: float, mode: str, gain: float = 1.0, L: int = 120):
    """Steps 1 to 6 of the specification on int16 ``pcm`` as a whole signal: -> (v, e, s), float64 arrays of its length."""
    x = _as_pcm16(pcm)
    check_limiter(mode)
    if mode is None:
        raise ValueError("limiter: a mode is needed")
    L = _check_lookahead(L)
    n, H = x.size, LIMIT_H
    v = x.astype(np.float64) * np.float64(gain)                                    # 1
    e = np.abs(v)                                                                  # 2
    if mode == "true" and n:
        h = limiter_taps()
        vp = np.concatenate([np.zeros(H, np.float64), v, np.zeros(H, np.float64)])  # vp[i + H] = v[i], zero outside
        for p in (1, 2, 3):
            u = np.zeros(n, np.float64)
            for j in range(-H + 1, H + 1):
                u = u + h[4 * H + p - 4 * j] * vp[j + H: j + H + n]
            e = np.maximum(e, np.abs(u))
    c = np.float64(c)
    over = e > c
    s = np.ones(n, np.float64)
    if not over.any():                                   # A is a sum of exact zeros: s is exactly 1 everywhere
        return v, e, s
    r = np.ones(n, np.float64)                                                     # 3
    r[over] = c / e[over]
    rp = np.concatenate([np.full(L, r[0]), r, np.full(L, r[-1])])                  # 4: r[clamp(j, 0, n - 1)]
    m = rp[0: n].copy()
    for k in range(1, 2 * L + 1):
        np.minimum(m, rp[k: k + n], out=m)
    d = 1.0 - m                                                                    # 5
    dp = np.concatenate([np.full(L, d[0]), d, np.full(L, d[-1])])
    w = limiter_window(L)
    A = np.zeros(n, np.float64)
    for k in range(2 * L + 1):
        A = A + w[k] * dp[k: k + n]
    return v, e, np.minimum(1.0 - A, r)                                            # 6


def limit_peaks(pcm, sr: int, peak_dbfs: float = -1.0, mode: str = "true", gain: float = 1.0, L: Optional[int] = None):
    """The look-ahead limiter of DESIGN §8 N13 on int16 ``pcm`` at ``sr`` Hz: the host mirror of vv_pcm_limit, bit for bit.
    y = clamp(rint((x * gain) * s)) with the gain curve s of limiter_gains, so that max |y| <= ceil(c), c = loudness_ceiling(peak_dbfs).
    mode "sample" limits the samples, "true" the 4x oversampled estimate of the peak between them.  L = the look-ahead in samples
    (None = limiter_lookahead(sr)).  -> (int16 array, stats {g, e_max, s_min, n_limited})."""
    x = _as_pcm16(pcm)
    _t, peak_dbfs = check_loudness(None, peak_dbfs)
    if isinstance(gain, bool) or not isinstance(gain, (int, float, np.integer, np.floating)) or not 0.0 < float(gain) < float("inf"):
        raise ValueError("limiter: the gain must be a positive finite number")
    L = limiter_lookahead(sr) if L is None else _check_lookahead(L)
    v, e, s = limiter_gains(x, loudness_ceiling(peak_dbfs), mode, float(gain), L)
    y = np.clip(np.rint(v * s), -32768.0, 32767.0).astype(np.int16)               # 7
    stats = {"g": float(gain), "e_max": float(e.max(initial=0.0)), "s_min": float(s.min(initial=1.0)), "n_limited": int((s < 1.0).sum())}
    return y, stats


# ---------------------------------------------------------------------- N14: pitch and tempo (WSOLA time stretch, then a rate conversion)
# The arithmetic below IS the specification and csrc/vv_prosody.hip computes the same operations: an exact integer
# cross-correlation search per frame and one float64 two-term blend per output sample, so the device equals this mirror bit for bit
# and a request is the same alone or in a batch.
WSOLA_N = 512                        # VV_WSOLA_N: frame length
WSOLA_HS = 256                       # VV_WSOLA_HS: synthesis hop
WSOLA_D = 128                        # VV_WSOLA_D: search radius, candidates -D ... D - 1
WSOLA_MAX_PQ = 2048                  # p and q of a stretch ratio lie in 1 ... 2048, p / q in [1/4, 4]
PITCH_RANGE = (-12.0, 12.0)          # accepted output_pitch, semitones
TEMPO_RANGE = (0.5, 2.0)             # accepted output_tempo
PROSODY_MAX_DEN = 32                 # both ratios are rounded to a fraction of at most this denominator
_WSOLA_WINDOW = []


class ProsodyPlan(NamedTuple):
    """What prosody_plan decides for one request of n samples: the stretch ratio p / q (lowest terms), the pitch ratio p_r / q_r, the
    stretched length n_s and the final length n_f."""
    p: int
    q: int
    p_r: int
    q_r: int
    n_s: int
    n_f: int


def check_prosody(pitch=None, tempo=None):
    """Validate ``output_pitch`` (semitones, -12 ... 12) and ``output_tempo`` (0.5 ... 2.0); None = off.  -> (float or None, float or None)."""
    out = []
    for name, v, (lo, hi), unit in (("output_pitch", pitch, PITCH_RANGE, "semitones"), ("output_tempo", tempo, TEMPO_RANGE, "times the speed")):
        if v is not None:
            if isinstance(v, bool) or not isinstance(v, (int, float, np.integer, np.floating)):
                raise ValueError(f"{name} must be a number ({unit}) or None")
            v = float(v)
            if not lo <= v <= hi:                                                  # NaN fails both comparisons
                raise ValueError(f"{name} must be between {lo:g} and {hi:g} ({unit})")
        out.append(v)
    return out[0], out[1]


def prosody_plan(n: int, pitch=None, tempo=None) -> Optional[ProsodyPlan]:
    """The one place where the options become ratios.  r = Fraction(2 ** (pitch / 12)).limit_denominator(32) = p_r / q_r (within 3.8 cents
    of the ideal at every integer semitone), tau = Fraction(tempo).limit_denominator(32); the signal is stretched by p / q = r / tau to
    n_s = ceil(n p / q) samples and then converted from rate p_r to rate q_r, of which the first n_f = ceil(n / tau) samples are kept.
    None when both ratios reduce to 1: nothing is to be done."""
    pitch, tempo = check_prosody(pitch, tempo)
    r = Fraction(2.0 ** (pitch / 12.0)).limit_denominator(PROSODY_MAX_DEN) if pitch is not None else Fraction(1)
    tau = Fraction(tempo).limit_denominator(PROSODY_MAX_DEN) if tempo is not None else Fraction(1)
    if r == 1 and tau == 1:
        return None
    s = r / tau
    n = int(n)
    return ProsodyPlan(s.numerator, s.denominator, r.numerator, r.denominator, -(-n * s.numerator // s.denominator),
                       -(-n * tau.denominator // tau.numerator))


def wsola_window() -> np.ndarray:
    """w[k] = 0.5 - 0.5 cos(2 pi k / N), k = 0 ... N - 1 (float64).  The device reads this table and never evaluates a cosine."""
    if not _WSOLA_WINDOW:
        w = (0.5 - 0.5 * np.cos(2.0 * np.pi * np.arange(WSOLA_N, dtype=np.float64) / np.float64(WSOLA_N))).astype(np.float64)
        w.setflags(write=False)
        _WSOLA_WINDOW.append(w)
    return _WSOLA_WINDOW[0]


def check_stretch_ratio(p, q) -> Tuple[int, int]:
    """A stretch ratio p / q as vv_pcm_stretch takes it: integers in 1 ... 2048, p != q, 1/4 <= p / q <= 4."""
    if any(isinstance(v, bool) or not isinstance(v, (int, np.integer)) for v in (p, q)):
        raise ValueError("time_stretch: p and q must be integers")
    p, q = int(p), int(q)
    if not (1 <= p <= WSOLA_MAX_PQ and 1 <= q <= WSOLA_MAX_PQ) or p == q or 4 * p < q or p > 4 * q:
        raise ValueError(f"time_stretch: p and q in 1 ... {WSOLA_MAX_PQ}, p != q, 1/4 <= p / q <= 4")
    return p, q


def time_stretch(pcm, p: int, q: int):
    """WSOLA time stretch of int16 ``pcm`` by p / q: the host mirror of vv_pcm_stretch, bit for bit.
    -> (int16 [ceil(n p / q)], pos int32 [M + 1]).  Frame m >= 1 is taken from x at pos_m = a_m + delta, a_m = floor((m - 1) HS q / p),
    where delta in -D ... D - 1 maximises the integer correlation with the natural continuation of frame m - 1 (x[pos_{m-1} + HS + k]);
    among equal maxima the smallest |delta| wins, the negative one first.  x is zero outside [0, n).  Output sample i of hop m - 1 is
    rint(w[k + HS] x[pos_{m-1} + HS + k] + w[k] x[pos_m + k]), k = i - (m - 1) HS: two products rounded on their own, one sum."""
    x = _as_pcm16(pcm)
    p, q = check_stretch_ratio(p, q)
    N, HS, D = WSOLA_N, WSOLA_HS, WSOLA_D
    n = x.size
    n_s = -(-n * p // q)
    M = -(-n_s // HS)
    left, right = HS + D, N + HS + D + 8                    # pos_0 = -HS, pos_m >= -D after it; a_m <= n, so pos_m + HS + N <= n + D + HS + N
    xp = np.zeros(left + n + right, np.int64)
    xp[left: left + n] = x
    pos = np.zeros(M + 1, np.int64)
    pos[0] = -HS
    delta = np.arange(-D, D, dtype=np.int64)
    rank = 2 * np.abs(delta) - (delta < 0)                  # 0, -1, 1, -2, 2, ...: the order among equal maxima
    for m in range(1, M + 1):
        a = (m - 1) * HS * q // p
        t = xp[left + pos[m - 1] + HS: left + pos[m - 1] + HS + N]
        span = xp[left + a - D: left + a - D + N + 2 * D]
        c = np.lib.stride_tricks.sliding_window_view(span, N)[: 2 * D] @ t       # int64: exact, |c| < 2^40
        pos[m] = a + delta[np.argmax(c * 512 + (511 - rank))]
    if n_s == 0:
        return np.zeros(0, np.int16), pos.astype(np.int32)
    w = wsola_window()
    i = np.arange(n_s, dtype=np.int64)
    m, k = i // HS + 1, i % HS
    tail = w[k + HS] * xp[left + pos[m - 1] + HS + k].astype(np.float64)
    head = w[k] * xp[left + pos[m] + k].astype(np.float64)
    return np.clip(np.rint(tail + head), -32768.0, 32767.0).astype(np.int16), pos.astype(np.int32)


def shift_prosody(pcm, pitch=None, tempo=None, formants="shift") -> np.ndarray:
    """Pitch (semitones) and tempo of int16 ``pcm`` after prosody_plan: the stretch by p / q, then resample_rows through
    resample_design(src = p_r, dst = q_r) for the first n_f samples.  The host mirror of the prosody step of HipSynth.finish_output
    (the stretch bit for bit; the rate conversion to the bound of resample_rows).  formants = "keep" (N18): where the pitch ratio is not
    1, keep_formants puts the spectral envelope of ``pcm`` back on the result."""
    keep = check_formants(formants) == "keep"
    src = x = _as_pcm16(pcm)
    plan = prosody_plan(x.size, pitch, tempo)
    if plan is None:
        return x
    if plan.p != plan.q:
        x = time_stretch(x, plan.p, plan.q)[0]
    if plan.p_r != plan.q_r:
        taps, up, down, skip = output_design(plan.p_r, plan.q_r)
        x = resample_rows(x, taps, up, down, skip, 0, 0, plan.n_f)
        if keep:
            x = keep_formants(src, x, *prosody_tempo(plan))
    return x


# ---------------------------------------------------------------------- N18: formant-preserving pitch shift (LPC envelope correction)
# The arithmetic below IS the specification and csrc/vv_formant.hip computes the same operations in the same order: per
# hop of H samples an all-pole envelope of the shifted signal y and of the source x at the same moment (windowed first difference, exact
# integer autocorrelation, the Levinson-Durbin recurrence of flac_lpc_coefficients), the filter gain A_y(z) / A_x(z) cut at L taps, and
# the two filters of a hop blended under the WSOLA window.  Every floating-point operation is one float64 operation, rounded on its own.
FORMANT_MODES = ("shift", "keep")    # ModelConfig.output_formants: "shift" = the envelope moves with the pitch (N14 as ever)
FORMANT_P = 24                       # VV_FORMANT_P: LPC order
FORMANT_NA = 1024                    # VV_FORMANT_NA: analysis window length
FORMANT_H = WSOLA_HS                 # VV_FORMANT_H: hop
FORMANT_L = 2048                     # VV_FORMANT_L: filter taps (gamma^L = 3.5e-5: what is cut off lies 89 dB below the response's start)
FORMANT_GAMMA = 0.995                # bandwidth expansion: A[k] = -(a[k] gamma^k); 0.99 left the 2500 Hz resonance of the test vowel shifted at -4 semitones
FORMANT_NOISE = 2.0 ** -20           # white-noise term: R[0] += R[0] 2^-20
_FORMANT_TABLES = []


def check_formants(formants):
    """Validate ``output_formants``: "shift" | "keep"; None = "shift".  -> the mode."""
    if formants is None:
        return "shift"
    if not isinstance(formants, str) or formants not in FORMANT_MODES:
        raise ValueError(f"output_formants must be one of {FORMANT_MODES}")
    return formants


def prosody_tempo(plan: ProsodyPlan) -> Tuple[int, int]:
    """The tempo fraction tn / td (lowest terms) of a plan: tau = (p_r / q_r) / (p / q), so that n_f = ceil(n td / tn)."""
    tau = Fraction(plan.p_r * plan.q, plan.q_r * plan.p)
    return tau.numerator, tau.denominator


def formant_tables():
    """(wa, g): wa[k] = 0.5 - 0.5 cos(2 pi k / NA), k < NA; g[0] = 1, g[k] = g[k - 1] * gamma, k <= P (float64).  The device reads these
    tables and evaluates neither a cosine nor a power."""
    if not _FORMANT_TABLES:
        wa = (0.5 - 0.5 * np.cos(2.0 * np.pi * np.arange(FORMANT_NA, dtype=np.float64) / np.float64(FORMANT_NA))).astype(np.float64)
        g = np.ones(FORMANT_P + 1, np.float64)
        for k in range(1, FORMANT_P + 1):
            g[k] = g[k - 1] * np.float64(FORMANT_GAMMA)
        wa.setflags(write=False)
        g.setflags(write=False)
        _FORMANT_TABLES.append((wa, g))
    return _FORMANT_TABLES[0]


def _formant_analysis(s: np.ndarray, centres: np.ndarray):
    """Step 1 for every frame of one signal at once (each operation elementwise over the frames, so each frame sees the written order):
    -> (A [F][P + 1], err [F], flat [F])."""
    P, NA = FORMANT_P, FORMANT_NA
    wa, g = formant_tables()
    F, left = centres.size, NA // 2 + 1
    sp = np.zeros(left + max(s.size, int(centres.max(initial=0)) + NA // 2) + 1, np.int64)
    sp[left: left + s.size] = s
    idx = left + centres[:, None] - NA // 2 + np.arange(NA, dtype=np.int64)[None, :]
    d = sp[idx] - sp[idx - 1]
    xw = np.rint(wa[None, :] * d.astype(np.float64)).astype(np.int64)                  # |xw| < 2^17
    R = np.stack([(xw[:, lag:] * xw[:, : NA - lag]).sum(axis=1) for lag in range(P + 1)], axis=1)      # exact: every sum below 2^44
    flat = R[:, 0] == 0
    Rf = R.astype(np.float64)
    Rf[:, 0] = Rf[:, 0] + Rf[:, 0] * FORMANT_NOISE
    a, err = np.zeros((F, P + 1), np.float64), Rf[:, 0].copy()
    with np.errstate(all="ignore"):                         # a flat frame goes on as 0 / 0: its numbers are never used
        for p in range(1, P + 1):
            acc = Rf[:, p].copy()
            for j in range(1, p):
                acc = acc - a[:, j] * Rf[:, p - j]
            k = acc / err
            new = a.copy()
            for j in range(1, p):
                new[:, j] = a[:, j] - k * a[:, p - j]
            new[:, p] = k
            a = new
            err = err * (1.0 - k * k)
            flat = flat | ~(err > 0.0)
    A = -(a * g[None, :])
    A[:, 0] = 1.0
    return A, err, flat


def _formant_frames(n: int, n_f: int, tn: int, td: int):
    if isinstance(tn, bool) or isinstance(td, bool) or int(tn) != tn or int(td) != td or not (1 <= tn <= WSOLA_MAX_PQ and 1 <= td <= WSOLA_MAX_PQ):
        raise ValueError(f"keep_formants: tn and td are integers in 1 ... {WSOLA_MAX_PQ}")
    tn, td = int(tn), int(td)
    if n_f != -(-n * td // tn):
        raise ValueError(f"keep_formants: y holds {n_f} samples, ceil(n td / tn) = {-(-n * td // tn)} are needed")
    m = np.arange(-(-n_f // FORMANT_H) + 1, dtype=np.int64)
    return m * FORMANT_H, (m * FORMANT_H * tn) // td


def formant_filters(x, y, tn: int = 1, td: int = 1, parts: bool = False):
    """Steps 1 and 2: -> (h float64 [M + 1][L], flat bool [M + 1]), M = ceil(n_f / H).  Frame m looks at y around m H and
    at x around floor(m H tn / td); h_m = gain * the first L samples of the impulse response of A_y(z) / A_x(z), gain = sqrt(err_x /
    err_y); a frame with a flat analysis on either side keeps the unit impulse.  parts: also (A_y, A_x, err_y, err_x) for a test."""
    x, y = _as_pcm16(x).astype(np.int64), _as_pcm16(y).astype(np.int64)
    P, L = FORMANT_P, FORMANT_L
    c_y, c_x = _formant_frames(x.size, y.size, tn, td)
    Ay, ey, fy = _formant_analysis(y, c_y)
    Ax, ex, fx = _formant_analysis(x, c_x)
    flat = fy | fx
    F = c_y.size
    r = np.zeros((F, L), np.float64)
    with np.errstate(all="ignore"):
        gain = np.sqrt(ex / ey)
        for t in range(L):
            acc = Ay[:, t].copy() if t <= P else np.zeros(F, np.float64)
            for k in range(1, min(t, P) + 1):
                acc = acc - Ax[:, k] * r[:, t - k]
            r[:, t] = acc
        h = gain[:, None] * r
    h[flat] = 0.0
    h[flat, 0] = 1.0
    return (h, flat, (Ay, Ax, ey, ex)) if parts else (h, flat)


def apply_formant_filters(y, h: np.ndarray) -> np.ndarray:
    """Step 3: z[i] = clamp(rint(w[k + H] v_a + w[k] v_b)), v_a = sum_j h_{m-1}[j] y[i - j], v_b the same with h_m, m = i // H + 1,
    k = i % H; each sum takes j ascending from +0.0, every product rounded on its own, y zero in front of the signal."""
    y = _as_pcm16(y)
    H, L, n_f = FORMANT_H, FORMANT_L, y.size
    w = wsola_window()
    yp = np.concatenate([np.zeros(L - 1, np.float64), y.astype(np.float64)])
    z = np.zeros(n_f, np.int16)
    for m1 in range(-(-n_f // H)):
        lo, hi = m1 * H, min(n_f, (m1 + 1) * H)
        Y = np.lib.stride_tricks.sliding_window_view(yp[lo: hi + L - 1], L)[:, ::-1]          # Y[i][j] = y[lo + i - j]
        va = np.cumsum(Y * h[m1][None, :], axis=1)[:, -1]                                      # cumsum adds in order, one rounding each
        vb = np.cumsum(Y * h[m1 + 1][None, :], axis=1)[:, -1]
        k = np.arange(hi - lo)
        z[lo: hi] = np.clip(np.rint(w[k + H] * va + w[k] * vb), -32768.0, 32767.0).astype(np.int16)
    return z


def keep_formants(x, y, tn: int = 1, td: int = 1) -> np.ndarray:
    """The envelope correction of a pitch shift: the host mirror of vv_pcm_formant, bit for bit.  x = the int16 signal
    before the prosody step (n samples), y = what the step made of it (n_f = ceil(n td / tn) samples, tn / td the tempo fraction).
    -> int16 [n_f]: y filtered so that its LPC envelope is x's again, its harmonics where the shift put them."""
    h, _flat = formant_filters(x, y, tn, td)
    return apply_formant_filters(y, h)


# ---------------------------------------------------------------------------- vocoder-bias denoiser
# Spectral subtraction against a stationary profile, the "denoiser" of the public HiFi-GAN / WaveGlow inference code: the magnitude spectrum
# the vocoder emits for an empty mel (the bias) times a strength is taken off the STFT magnitudes of an utterance, clamped at zero, the
# phases kept.  The arithmetic below is the specification of vv_pcm_denoise (csrc/vv_denoise.hip), which equals it bit for bit: float64,
# every operation rounded on its own, and a transform whose butterflies are written out -- radix-2 decimation in time behind a bit
# reversal, stages of half-length h = 1, 2, ... N / 2; per butterfly (a, b) of a stage with tw = (c, s) = twiddle[j N / (2 h)]:
#     tr = br c - bi s;  ti = br s + bi c;  a' = a + t;  b' = a - t                 (four products, two sums, then the two results)
# with the products of the first stages (c = 1, s = 0) carried out like all others.  The inverse is the same with s negated, unscaled.
DENOISE_N = 1024                     # VV_DENOISE_N: frame length and transform size, independent of the model's n_fft
DENOISE_H = 256                      # VV_DENOISE_H: hop; every sample lies under four frames, sum of w^2 = 1.5 there
DENOISE_BINS = DENOISE_N // 2 + 1    # entries of a bias profile
DENOISE_SCALE = 1536.0               # N * 1.5: the unscaled inverse transform times the window's overlap sum
DENOISE_MAX_STRENGTH = 16.0
DENOISE_BIAS_MAX_N = 1 << 20         # the longest signal denoise_bias / vv_pcm_denoise_bias measure
_DENOISE_TABLES = []


def check_denoise(strength):
    """Validate ``output_denoise``: None = off, else a strength s with 0 < s <= 16.  -> None or the float."""
    if strength is None:
        return None
    if isinstance(strength, bool) or not isinstance(strength, (int, float)) or not 0.0 < float(strength) <= DENOISE_MAX_STRENGTH:
        raise ValueError(f"output_denoise must be None or a strength in (0, {DENOISE_MAX_STRENGTH:g}]")
    return float(strength)


def check_denoise_bias(bias):
    """Validate a bias profile: DENOISE_BINS finite non-negative numbers.  -> float64 [513] (None stays None)."""
    if bias is None:
        return None
    try:
        b = np.asarray(bias, dtype=np.float64)
    except (TypeError, ValueError):
        raise ValueError(f"output_denoise_bias must be a sequence of {DENOISE_BINS} numbers") from None
    if b.shape != (DENOISE_BINS,) or not np.all(np.isfinite(b)) or np.any(b < 0.0):
        raise ValueError(f"output_denoise_bias must be a sequence of {DENOISE_BINS} finite non-negative numbers")
    return b


def denoise_tables():
    """(w, tw): w[k] = 0.5 - 0.5 cos(2 pi k / N), k < N; tw [2][N / 2] = cos(2 pi k / N), -sin(2 pi k / N) (float64).  The device reads
    these tables and evaluates neither a cosine nor a sine."""
    if not _DENOISE_TABLES:
        N = DENOISE_N
        w = (0.5 - 0.5 * np.cos(2.0 * np.pi * np.arange(N, dtype=np.float64) / np.float64(N))).astype(np.float64)
        a = 2.0 * np.pi * np.arange(N // 2, dtype=np.float64) / np.float64(N)
        tw = np.stack([np.cos(a), -np.sin(a)]).astype(np.float64)
        rev = np.zeros(N, np.int64)
        for b in range(N.bit_length() - 1):
            rev |= ((np.arange(N) >> b) & 1) << (N.bit_length() - 2 - b)
        for t in (w, tw, rev):
            t.setflags(write=False)
        _DENOISE_TABLES.append((w, tw, rev))
    return _DENOISE_TABLES[0][:2]


def denoise_fft(re: np.ndarray, im: np.ndarray, inverse: bool = False):
    """The transform of the specification on every row of re, im [F][N] at once (each operation elementwise over the rows, so each row
    sees the written order) -> (re, im) [F][N], unscaled in both directions."""
    denoise_tables()
    _w, tw, rev = _DENOISE_TABLES[0]
    N = DENOISE_N
    F = re.shape[0]
    c, s = tw[0], (-tw[1] if inverse else tw[1])
    re, im = np.ascontiguousarray(re[:, rev]), np.ascontiguousarray(im[:, rev])
    h = 1
    while h < N:
        step = N // (2 * h)
        cj, sj = c[::step][None, None, :], s[::step][None, None, :]                   # twiddle[j step], j < h
        R, I = re.reshape(F, N // (2 * h), 2, h), im.reshape(F, N // (2 * h), 2, h)
        ar, ai, br, bi = R[:, :, 0, :], I[:, :, 0, :], R[:, :, 1, :], I[:, :, 1, :]
        tr = br * cj - bi * sj
        ti = br * sj + bi * cj
        re = np.stack([ar + tr, ar - tr], axis=2).reshape(F, N)
        im = np.stack([ai + ti, ai - ti], axis=2).reshape(F, N)
        h *= 2
    return re, im


def _denoise_frames(x: np.ndarray, starts: np.ndarray) -> np.ndarray:
    """w[k] x[start + k] for every start, x zero outside the signal -> float64 [F][N]."""
    N = DENOISE_N
    w = denoise_tables()[0]
    xp = np.zeros(x.size + 2 * N + int(starts.max(initial=0)) + 1, np.float64)
    xp[N: N + x.size] = x
    return w[None, :] * xp[N + starts[:, None] + np.arange(N, dtype=np.int64)[None, :]]


def denoise_bias(pcm) -> np.ndarray:
    """The bias profile of a signal, the mirror of vv_pcm_denoise_bias: per bin 0 ... N / 2 the mean magnitude over the
    full frames, those that start at a multiple of H at or behind sample 0 and end inside the signal, summed from +0.0 with the frame
    ascending and divided by their count.  -> float64 [513]; a signal without a full frame is refused."""
    x = _as_pcm16(pcm)
    N, H = DENOISE_N, DENOISE_H
    if x.size < N or x.size > DENOISE_BIAS_MAX_N:
        raise ValueError(f"denoise_bias: a signal of {N} ... {DENOISE_BIAS_MAX_N} samples is needed (one full frame), got {x.size}")
    starts = np.arange((x.size - N) // H + 1, dtype=np.int64) * H
    fr = _denoise_frames(x, starts)
    re, im = denoise_fft(fr, np.zeros_like(fr))
    re, im = re[:, :DENOISE_BINS], im[:, :DENOISE_BINS]
    mag = np.sqrt(re * re + im * im)
    acc = np.zeros(DENOISE_BINS, np.float64)
    for f in range(starts.size):
        acc = acc + mag[f]
    return acc / np.float64(starts.size)


def denoise_pcm(pcm, bias, strength, mags: bool = False):
    """The denoiser: the host mirror of vv_pcm_denoise, bit for bit.  pcm int16 [n]; bias = 513 non-negative float64
    (denoise_bias of the vocoder's output for an empty mel, or the caller's own); strength 0 ... 16 (0 is computed like any other and
    gives the input back).  With M = ceil(n / H), frames f = 0 ... M + 2 starting at (f - 3) H: forward transform of w u, per bin
    mag = sqrt(re re + im im), d = mag - s bias, g = d > 0 ? d / mag : 0, re g and im g, inverse transform, real part times w; hop i
    adds frames i ... i + 3 in that order from +0.0 and z = clamp(rint(acc / 1536)).  -> int16 [n], with ``mags`` also float64 [M + 3][N]."""
    x = _as_pcm16(pcm)
    N, H = DENOISE_N, DENOISE_H
    b = check_denoise_bias(bias)
    if b is None:
        raise ValueError("denoise_pcm: a bias profile is needed")
    if isinstance(strength, bool) or not isinstance(strength, (int, float)) or not 0.0 <= float(strength) <= DENOISE_MAX_STRENGTH:
        raise ValueError(f"denoise_pcm: the strength is a number in 0 ... {DENOISE_MAX_STRENGTH:g}")
    s = float(strength)
    n = x.size
    M = -(-n // H)
    starts = (np.arange(M + 3, dtype=np.int64) - 3) * H
    fr = _denoise_frames(x, starts)                                                   # starts from -3 H on: the padding in front covers them
    re, im = denoise_fft(fr, np.zeros_like(fr))
    full = np.concatenate([b, b[N // 2 - 1: 0: -1]])                                  # bin k > N / 2 uses bias[N - k]
    mag = np.sqrt(re * re + im * im)
    d = mag - np.float64(s) * full[None, :]
    g = np.zeros_like(mag)
    np.divide(d, mag, out=g, where=d > 0.0)
    re, _im = denoise_fft(re * g, im * g, inverse=True)
    c = (re * denoise_tables()[0][None, :]).reshape(M + 3, 4, H)
    acc = np.zeros((M, H), np.float64)
    for j in range(4):                                                                # frame i + j lies (3 - j) hops into itself at hop i
        acc = acc + c[j: j + M, 3 - j]
    z = np.clip(np.rint(acc / DENOISE_SCALE), -32768.0, 32767.0).astype(np.int16).reshape(-1)[:n]
    return (z, mag) if mags else z


# ---------------------------------------------------------------------------- keyed audio watermark
# A multiplicative spread-spectrum mark (Cox et al. 1997; for audio Kirovski & Malvar 2003) on the denoiser's frames: every cell (frame f,
# band bin k) of the STFT is scaled by 1 + a or 1 - a as its keyed chip and its message bit agree or not, and a detector that knows the key
# correlates the chips with a per-cell contrast of the magnitude against its neighbours in time, at each of 256 whole-hop alignments.  The
# arithmetic below is the specification of vv_pcm_watermark and vv_pcm_watermark_detect (csrc/vv_watermark.hip), which equal it bit for
# bit: the transform and the frames are denoise_fft's, every float64 operation is rounded on its own, and behind the cell value
# everything is an integer.
#     cell (f, k) at alignment q: group g = ((f + q) // G) % P, bit index j = (k - LO + 7 g) % NB, chip = table[g][k - LO]
#     embed (q = 0)  : gain = chip (2 bit_j - 1) > 0 ? 1 + a : 1 - a on bins k and N - k of the band, 1.0 elsewhere; then as the denoiser
#     detect         : m = magnitude; r = 0.5 (m[max(f - G, 0)] + m[min(f + G, F - 1)]); d = int(rint(32768 (m - r) / (m + r + 1.0)));
#                      num[q][j] = sum chip d, den[q][j] = sum d d over the cells of bit j (int64)
#     host           : z = num / sqrt(den) (0 where den = 0); score[q] = sqrt(mean_j z^2); the smallest q with the largest score
WATERMARK_LO = 22                    # VV_WATERMARK_LO: first band bin (about 0.5 kHz at 24 kHz)
WATERMARK_K = 320                    # VV_WATERMARK_K: band bins LO ... LO + K - 1 (to about 8 kHz)
WATERMARK_G = 4                      # VV_WATERMARK_G: frames that share a chip
WATERMARK_P = 64                     # VV_WATERMARK_P: groups in a pattern period (65 536 samples)
WATERMARK_NB = 24                    # VV_WATERMARK_NB: message bits: 16 of payload, MSB first, then the CRC-8 of its two bytes, MSB first
WATERMARK_Q = WATERMARK_P * WATERMARK_G                  # alignments searched (whole hops)
WATERMARK_MAX_STRENGTH = 0.5
WATERMARK_DETECT_MAX_N = 1 << 24     # the longest clip watermark_stats / vv_pcm_watermark_detect take
WATERMARK_THRESHOLD = 2.6153          # 1.3 x 2.0118, the largest score of the null pool measured on this mirror (profiles/watermark/notes.md)
_WATERMARK_CHIPS = {}


def check_watermark_key(key):
    """Validate ``output_watermark_key``: None = no watermark, else an integer 0 ... 2^64 - 1.  -> None or the int."""
    if key is None:
        return None
    if isinstance(key, bool) or not isinstance(key, (int, np.integer)) or not 0 <= int(key) < 1 << 64:
        raise ValueError("output_watermark_key must be None or an integer in 0 ... 2^64 - 1")
    return int(key)


def check_watermark_payload(payload):
    """Validate a watermark payload: None stays None (the engine's), else an integer 0 ... 65535.  -> None or the int."""
    if payload is None:
        return None
    if isinstance(payload, bool) or not isinstance(payload, (int, np.integer)) or not 0 <= int(payload) <= 0xFFFF:
        raise ValueError("the watermark payload must be an integer in 0 ... 65535")
    return int(payload)


def check_watermark_strength(strength, zero: bool = False):
    """Validate ``output_watermark_strength``: a number a with 0 < a <= 0.5 (``zero``: 0 as well, which returns the input).  -> the float."""
    ok = not isinstance(strength, bool) and isinstance(strength, (int, float)) and 0.0 <= float(strength) <= WATERMARK_MAX_STRENGTH
    if not ok or (float(strength) == 0.0 and not zero):
        raise ValueError(f"output_watermark_strength must be a number in {'0 ... ' if zero else '(0, '}{WATERMARK_MAX_STRENGTH:g}{'' if zero else ']'}")
    return float(strength)


def watermark_message(payload: int) -> int:
    """The 24 message bits as one integer: payload << 8 | CRC-8 of its two big-endian bytes; bit j of the message is bit 23 - j of it."""
    p = check_watermark_payload(payload)
    if p is None:
        raise ValueError("the watermark payload must be an integer in 0 ... 65535")
    return p << 8 | flac_crc8(bytes([p >> 8, p & 0xFF]))


def watermark_words(key: int, count: int) -> List[int]:
    """The first ``count`` outputs of SplitMix64 from the state ``key``."""
    mask, s, out = (1 << 64) - 1, check_watermark_key(key), []
    if s is None:
        raise ValueError("a watermark key is needed")
    for _ in range(count):
        s = (s + 0x9E3779B97F4A7C15) & mask
        z = s
        z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & mask
        z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & mask
        out.append(z ^ (z >> 31))
    return out


def watermark_chips(key: int) -> np.ndarray:
    """The chip table of a key: int8 [P][K] of +-1; cell e = g K + (k - LO) takes bit e % 64 (LSB first) of word e // 64.  Made on the
    host only: the device reads the table and hashes nothing."""
    key = check_watermark_key(key)
    if key not in _WATERMARK_CHIPS:
        cells = WATERMARK_P * WATERMARK_K
        words = np.array(watermark_words(key, cells // 64), dtype=np.uint64)
        bits = (words[:, None] >> np.arange(64, dtype=np.uint64)[None, :]) & np.uint64(1)
        table = (2 * bits.astype(np.int8) - 1).reshape(WATERMARK_P, WATERMARK_K)
        table.setflags(write=False)
        if len(_WATERMARK_CHIPS) >= 16:
            _WATERMARK_CHIPS.clear()
        _WATERMARK_CHIPS[key] = table
    return _WATERMARK_CHIPS[key]


def _watermark_starts(n: int) -> np.ndarray:
    return (np.arange(-(-n // DENOISE_H) + 3, dtype=np.int64) - 3) * DENOISE_H


def watermark_embed(pcm, key: int, payload: int, strength: float = 0.2) -> np.ndarray:
    """The embedder: the host mirror of vv_pcm_watermark, bit for bit.  pcm int16 [n] -> int16 [n]: the denoiser's
    loop with the gain (chip (2 bit_j - 1) > 0) ? gp : gm on the band bins and their mirrors at alignment 0, gp = 1.0 + a and
    gm = 1.0 - a; a = 0 is computed like any other and gives the input back."""
    x = _as_pcm16(pcm)
    a = check_watermark_strength(strength, zero=True)
    chips, msg = watermark_chips(key), watermark_message(payload)
    N, H, LO, K = DENOISE_N, DENOISE_H, WATERMARK_LO, WATERMARK_K
    gp, gm = np.float64(1.0) + np.float64(a), np.float64(1.0) - np.float64(a)
    n = x.size
    M = -(-n // H)
    fr = _denoise_frames(x, _watermark_starts(n))
    re, im = denoise_fft(fr, np.zeros_like(fr))
    g = (np.arange(M + 3) // WATERMARK_G) % WATERMARK_P
    j = (np.arange(K)[None, :] + 7 * g[:, None]) % WATERMARK_NB
    sign = 2 * ((msg >> (WATERMARK_NB - 1 - j)) & 1) - 1
    band = np.where(chips[g] * sign > 0, gp, gm)
    gain = np.ones((M + 3, N), np.float64)
    gain[:, LO: LO + K] = band
    gain[:, N - LO - K + 1: N - LO + 1] = band[:, ::-1]                               # bin N - k carries the gain of bin k
    re, _im = denoise_fft(re * gain, im * gain, inverse=True)
    c = (re * denoise_tables()[0][None, :]).reshape(M + 3, 4, H)
    acc = np.zeros((M, H), np.float64)
    for q in range(4):
        acc = acc + c[q: q + M, 3 - q]
    return np.clip(np.rint(acc / DENOISE_SCALE), -32768.0, 32767.0).astype(np.int16).reshape(-1)[:n]


def watermark_cells(pcm) -> np.ndarray:
    """The detector's cell values (the mirror of vv_pcm_watermark_detect's second kernel): int32 [F][K], F = ceil(n / H) + 3."""
    x = _as_pcm16(pcm)
    if x.size > WATERMARK_DETECT_MAX_N:
        raise ValueError(f"watermark_cells: at most {WATERMARK_DETECT_MAX_N} samples, got {x.size}")
    fr = _denoise_frames(x, _watermark_starts(x.size))
    re, im = denoise_fft(fr, np.zeros_like(fr))
    re, im = re[:, WATERMARK_LO: WATERMARK_LO + WATERMARK_K], im[:, WATERMARK_LO: WATERMARK_LO + WATERMARK_K]
    m = np.sqrt(re * re + im * im)
    f = np.arange(m.shape[0])
    r = 0.5 * (m[np.maximum(f - WATERMARK_G, 0)] + m[np.minimum(f + WATERMARK_G, m.shape[0] - 1)])
    return np.rint(32768.0 * (m - r) / (m + r + 1.0)).astype(np.int32)


def watermark_stats(pcm, key: int, cells: Optional[np.ndarray] = None) -> np.ndarray:
    """The detector's integer statistic (the mirror of vv_pcm_watermark_detect): int64 [256][24][2] = {num, den} per alignment q and bit j.
    Integers, so the order of the sums is free: the frames that share a group at alignment q = 4 a + b are summed first."""
    d = (watermark_cells(pcm) if cells is None else np.asarray(cells)).astype(np.int64)
    chips = watermark_chips(key).astype(np.int64)
    F, K, G, P, NB = d.shape[0], WATERMARK_K, WATERMARK_G, WATERMARK_P, WATERMARK_NB
    out = np.zeros((WATERMARK_Q, NB, 2), np.int64)
    fold = lambda v: np.pad(v, ((0, 0), (0, -K % NB))).reshape(v.shape[0], -1, NB).sum(axis=1)  # noqa: E731  [T][K] -> [T][(k - LO) % NB]
    jj = np.arange(NB)[None, :]
    for b in range(G):
        t = (np.arange(F) + b) // G                                                   # frame f lies in block t; its group is (t + a) % P
        T = int(t[-1]) + 1
        D, E = np.zeros((T, K), np.int64), np.zeros((T, K), np.int64)
        np.add.at(D, t, d)
        np.add.at(E, t, d * d)
        E, rows = fold(E), np.arange(T)[:, None]
        for a in range(P):
            g = (np.arange(T) + a) % P
            src = (jj - 7 * g[:, None]) % NB                                          # bit j of group g collects the bins with (k - LO) % NB = j - 7 g
            out[G * a + b, :, 0] = fold(chips[g] * D)[rows, src].sum(axis=0)
            out[G * a + b, :, 1] = E[rows, src].sum(axis=0)
    return out


class WatermarkResult(NamedTuple):
    """What the detector says of one clip: ``payload`` is None unless ``crc_ok``; ``offset`` = the alignment q of the largest score."""
    score: float
    present: bool
    offset: int
    payload: Optional[int]
    crc_ok: bool
    z: Tuple[float, ...]


def watermark_decide(stats) -> WatermarkResult:
    """The host step behind the statistic: stats int64 [256][24][2] -> the result record."""
    s = np.asarray(stats, dtype=np.int64).reshape(WATERMARK_Q, WATERMARK_NB, 2)
    num, den = s[..., 0].astype(np.float64), s[..., 1].astype(np.float64)
    z = np.zeros_like(num)
    np.divide(num, np.sqrt(den), out=z, where=den > 0.0)
    score = np.sqrt(np.mean(z * z, axis=1))
    q = int(np.argmax(score))                                                         # the first of the largest
    bits = 0
    for v in z[q]:
        bits = bits << 1 | int(v > 0.0)
    payload = bits >> 8
    crc_ok = watermark_message(payload) == bits
    present = bool(score[q] >= WATERMARK_THRESHOLD)
    return WatermarkResult(float(score[q]), present, q, payload if crc_ok else None, crc_ok, tuple(float(v) for v in z[q]))


def watermark_detect(pcm, key: int) -> WatermarkResult:
    """The detector on the host: watermark_decide(watermark_stats(pcm, key))."""
    return watermark_decide(watermark_stats(pcm, key))


class AudioProcessor:
    """Static helpers, same names and semantics as the reference class."""

    @staticmethod
    def _read_bytes(path_or_bytes: Union[str, bytes]) -> bytes:
        if isinstance(path_or_bytes, str):
            if not Path(path_or_bytes).exists():
                raise FileNotFoundError(f"Audio file not found: {path_or_bytes}")
            with open(path_or_bytes, "rb") as fh:
                return fh.read()
        return bytes(path_or_bytes)

    @staticmethod
    def decode(path_or_bytes: Union[str, bytes]) -> Tuple[np.ndarray, int, int]:
        """-> (integer frames (n, channels), sample width, rate); container parsing only, no arithmetic on samples."""
        data = AudioProcessor._read_bytes(path_or_bytes)
        if data[:4] != b"RIFF" and is_flac(data):          # N17: ``fLaC``, or an ID3v2 tag in front of it
            return flac_decode(data)
        if data[:4] != b"RIFF":
            raise ValueError("unsupported audio container: only RIFF/WAVE and FLAC can be decoded in this build (no ffmpeg)")
        return _decode_wav(data)

    @staticmethod
    def probe_duration(path_or_bytes: Union[str, bytes]) -> float:
        data = AudioProcessor._read_bytes(path_or_bytes)
        if data[:4] != b"RIFF" and is_flac(data):          # a FLAC with a known total: STREAMINFO alone, nothing is decoded
            info = flac_container(data)
            if info.total:
                return info.total / float(info.rate)
        frames, _w, rate = AudioProcessor.decode(data)
        return frames.shape[0] / float(rate)

    @staticmethod
    def load_samples(path_or_bytes: Union[str, bytes], sample_rate: int) -> np.ndarray:
        """The integer samples ``audio_segment.get_array_of_samples()`` holds in the reference (:22-25): mono, at sample_rate."""
        frames, _w, rate = AudioProcessor.decode(path_or_bytes)
        return ratecv(tomono(frames), rate, sample_rate)

    @staticmethod
    def load_audio(path_or_bytes: Union[str, bytes], sample_rate: int, resampler: str = "ratecv") -> np.ndarray:
        if resampler == "ratecv":
            return AudioProcessor.normalize_to_int16(AudioProcessor.load_samples(path_or_bytes, sample_rate).astype(np.float32))
        if resampler != "polyphase":
            raise ValueError(f"unknown resampler {resampler!r}")
        frames, _w, rate = AudioProcessor.decode(path_or_bytes)
        x = frames.astype(np.float32).mean(axis=1)              # the normalisation below is scale-free
        return AudioProcessor.normalize_to_int16(_resample_polyphase(x, rate, sample_rate))

    @staticmethod
    def normalize_to_int16(audio: np.ndarray) -> np.ndarray:
        centred = audio - np.mean(audio)
        peak = np.max(np.abs(centred))
        if peak > 0:
            centred = centred * (29491.0 / peak)        # 90 % of full scale
        return centred.astype(np.int16)

    @staticmethod
    def fix_clipped_audio(audio: np.ndarray) -> np.ndarray:
        audio = np.nan_to_num(audio, nan=0.0, posinf=0.0, neginf=0.0)
        peak = np.max(np.abs(audio))
        if peak >= 32767:
            return (audio * (26214.0 / peak)).astype(np.int16)   # 80 % of full scale
        return audio

    @staticmethod
    def _g711_wav(flat: np.ndarray, sample_rate: int, encoding: str) -> bytes:
        """RIFF/WAVE bytes of G.711 data: format tag 7 (mu-law) / 6 (A-law), 8 bits, an 18-byte fmt chunk and a fact chunk."""
        payload = np.asarray(flat, dtype=np.uint8).tobytes()
        pad = b"\0" * (len(payload) & 1)
        fmt = struct.pack("<HHIIHHH", _WAVE_TAG[encoding], 1, sample_rate, sample_rate, 1, 8, 0)
        fact = struct.pack("<I", len(payload))
        body = b"WAVE" + b"fmt " + struct.pack("<I", len(fmt)) + fmt + b"fact" + struct.pack("<I", 4) + fact + \
            b"data" + struct.pack("<I", len(payload)) + payload + pad
        return b"RIFF" + struct.pack("<I", len(body)) + body

    @staticmethod
    def _flac_bytes(flat: np.ndarray) -> bytes:
        if flat.dtype != np.uint8 or flat.size < 42 or flat[:4].tobytes() != b"fLaC":
            raise ValueError("flac audio must be the uint8 bytes of a FLAC file (encode_output(x, 'flac', rate))")
        return flat.tobytes()

    @staticmethod
    def _adpcm_bytes(flat: np.ndarray) -> bytes:
        """The complete IMA ADPCM WAVE file the output stage made (N25), as it is; raw blocks (a collected stream) need adpcm_wav first."""
        if flat.dtype != np.uint8 or flat.size < ADPCM_HEADER_BYTES or flat[:4].tobytes() != b"RIFF":
            raise ValueError("adpcm audio must be the uint8 bytes of an IMA ADPCM WAVE file (encode_output(x, 'adpcm', rate), or adpcm_wav of a stream's blocks)")
        return flat.tobytes()

    @staticmethod
    def save_audio(audio: np.ndarray, file_path: str, sample_rate: int, encoding: str = "pcm16") -> None:
        if audio.size == 0:
            raise ValueError("Cannot save empty audio.")
        if encoding not in OUTPUT_ENCODINGS:
            raise ValueError(f"output_encoding must be one of {list(OUTPUT_ENCODINGS)}")
        Path(file_path).parent.mkdir(parents=True, exist_ok=True)
        flat = np.asarray(audio).reshape(-1)
        if encoding in ("flac", "adpcm"):            # already a complete file (N15, N25): written as it is
            with open(file_path, "wb") as fh:
                fh.write(AudioProcessor._flac_bytes(flat) if encoding == "flac" else AudioProcessor._adpcm_bytes(flat))
            return
        if encoding != "pcm16":                      # already companded (uint8) by the output stage
            if flat.dtype != np.uint8:
                raise ValueError(f"{encoding} audio must be uint8 G.711 codes")
            with open(file_path, "wb") as fh:
                fh.write(AudioProcessor._g711_wav(flat, sample_rate, encoding))
            return
        if flat.dtype != np.int16:
            if np.issubdtype(flat.dtype, np.floating):
                flat = np.clip(flat * 32768.0 if np.max(np.abs(flat)) <= 1.0 else flat, -32768, 32767)
            flat = flat.astype(np.int16)
        payload = flat.astype("<i2").tobytes()
        fmt = struct.pack("<HHIIHHHHI", 0xFFFE, 1, sample_rate, sample_rate * 2, 2, 16, 22, 16, 0x4) + _PCM_GUID
        with open(file_path, "wb") as fh:
            fh.write(b"RIFF" + struct.pack("<I", 4 + 8 + len(fmt) + 8 + len(payload)) + b"WAVE")
            fh.write(b"fmt " + struct.pack("<I", len(fmt)) + fmt)
            fh.write(b"data" + struct.pack("<I", len(payload)) + payload)

    @staticmethod
    def to_wav_bytes(audio: np.ndarray, sample_rate: int, encoding: str = "pcm16") -> bytes:
        if encoding != "pcm16":
            if encoding not in OUTPUT_ENCODINGS:
                raise ValueError(f"output_encoding must be one of {list(OUTPUT_ENCODINGS)}")
            if encoding == "flac":                   # not a WAVE file: the FLAC file the output stage made, as it is
                return AudioProcessor._flac_bytes(np.asarray(audio).reshape(-1))
            if encoding == "adpcm":                  # the IMA ADPCM WAVE file the output stage made (N25), as it is
                return AudioProcessor._adpcm_bytes(np.asarray(audio).reshape(-1))
            return AudioProcessor._g711_wav(np.asarray(audio).reshape(-1), sample_rate, encoding)
        buf = io.BytesIO()
        flat = np.asarray(audio).reshape(-1).astype("<i2")
        buf.write(b"RIFF" + struct.pack("<I", 36 + flat.nbytes) + b"WAVEfmt " + struct.pack("<IHHIIHH", 16, 1, 1, sample_rate, sample_rate * 2, 2, 16))
        buf.write(b"data" + struct.pack("<I", flat.nbytes) + flat.tobytes())
        return buf.getvalue()

    # ------------------------------------------------------------------ chunk joining
    @staticmethod
    def concatenate_with_crossfade(generated_waves: List[np.ndarray], cross_fade_duration: float, sample_rate: int) -> np.ndarray:
        if not generated_waves:
            return np.array([])
        if len(generated_waves) == 1:
            return generated_waves[0].reshape(-1)
        flat = [w.reshape(-1) for w in generated_waves]
        if cross_fade_duration <= 0:
            return np.concatenate(flat)
        out = flat[0]
        for nxt in flat[1:]:
            n = min(int(cross_fade_duration * sample_rate), len(out), len(nxt))
            if n <= 0:
                out = np.concatenate([out, nxt])
                continue
            ramp_down, ramp_up = np.linspace(1, 0, n), np.linspace(0, 1, n)
            out = np.concatenate([out[:-n], out[-n:] * ramp_down + nxt[:n] * ramp_up, nxt[n:]])
        return out

    @staticmethod
    def concatenate_with_crossfade_improved(generated_waves: List[np.ndarray], cross_fade_duration: float, sample_rate: int) -> np.ndarray:
        if not generated_waves:
            return np.array([])
        if len(generated_waves) == 1:
            return generated_waves[0].reshape(-1)
        flat = [AudioProcessor.fix_clipped_audio(w.reshape(-1)) for w in generated_waves]
        if cross_fade_duration <= 0:
            return np.concatenate(flat)
        out = flat[0]
        for nxt in flat[1:]:
            n = min(int(cross_fade_duration * sample_rate), len(out), len(nxt))
            if n <= 0:
                out = np.concatenate([out, nxt])
                continue
            tail, head = out[-n:], nxt[:n]
            rms_prev = np.sqrt(np.mean(tail.astype(np.float32) ** 2))
            rms_next = np.sqrt(np.mean(head.astype(np.float32) ** 2))
            if rms_prev > 100 and rms_next > 100:
                gain = np.clip(rms_prev / rms_next, 0.7, 1.5)          # level-match, bounded
                nxt = (nxt.astype(np.float32) * gain).astype(np.int16)
                head = nxt[:n]
            theta = np.linspace(0, np.pi / 2, n)
            mixed = (tail.astype(np.float32) * np.cos(theta) ** 2 + head.astype(np.float32) * np.sin(theta) ** 2).astype(np.int16)
            out = np.concatenate([out[:-n], mixed, nxt[n:]])
        return out


class CrossfadeStream:
    """Incremental form of ``concatenate_with_crossfade_improved`` for streaming output.

    The buffered join (reference core/audio_processor.py:122-192) repairs clipping once per RAW chunk and then, per
    junction, rewrites only the last ``n = min(cross_fade, len(out), len(next))`` samples of what has been joined.
    This class keeps exactly that state -- the not-yet-final tail of ``out`` and its total length -- so every chunk goes
    through ``fix_clipped_audio`` once, already-emitted samples are never touched again, and the concatenation of the
    blocks returned by ``push`` equals the buffered result sample for sample.  ``n_chunks`` is needed up front because
    the buffered function returns a single chunk untouched (no clip repair when there is nothing to join)."""

    def __init__(self, n_chunks: int, cross_fade_duration: float, sample_rate: int):
        self.n_chunks = int(n_chunks)
        self.cf = int(cross_fade_duration * sample_rate) if cross_fade_duration > 0 else 0
        self.fade = cross_fade_duration > 0
        self.held = None          # un-emitted tail of the joined signal
        self.total = 0            # samples joined so far (emitted + held)
        self.seen = 0

    def push(self, wave: np.ndarray) -> np.ndarray:
        """Add the next raw chunk; returns the samples that became final (possibly empty)."""
        self.seen += 1
        last = self.seen >= self.n_chunks
        w = np.asarray(wave).reshape(-1)
        if self.n_chunks == 1:
            return w
        nxt = AudioProcessor.fix_clipped_audio(w)
        if self.held is None:
            joined = nxt
        else:
            n = min(self.cf, self.total, len(nxt)) if self.fade else 0
            if n <= 0:
                joined = np.concatenate([self.held, nxt])
            else:
                tail, head = self.held[-n:], nxt[:n]
                rms_prev = np.sqrt(np.mean(tail.astype(np.float32) ** 2))
                rms_next = np.sqrt(np.mean(head.astype(np.float32) ** 2))
                if rms_prev > 100 and rms_next > 100:
                    gain = np.clip(rms_prev / rms_next, 0.7, 1.5)
                    nxt = (nxt.astype(np.float32) * gain).astype(np.int16)
                    head = nxt[:n]
                theta = np.linspace(0, np.pi / 2, n)
                mixed = (tail.astype(np.float32) * np.cos(theta) ** 2 + head.astype(np.float32) * np.sin(theta) ** 2).astype(np.int16)
                joined = np.concatenate([self.held[:-n], mixed, nxt[n:]])
        self.total += len(joined) - (0 if self.held is None else len(self.held))
        keep = 0 if last else min(self.cf, len(joined))       # the next junction may rewrite at most the last cf samples
        out, self.held = joined[: len(joined) - keep], joined[len(joined) - keep:]
        return np.ascontiguousarray(out)


class OutputStream:
    """Output rate and encoding for a STREAM of final 24 kHz blocks (``synthesize_stream``): carries the position (m0, i0) and the input
    history the filter still needs, so that the concatenation of the blocks it returns equals the buffered result bit for bit --
    every output sample is the same ascending float64 sum over the same input samples, whichever block delivers it.

    ``resample(x, m0, i0, n_out)`` and ``encode(y)`` are the two back ends: the host mirrors above, or the device kernels
    (HipSynth.output_stream_backends).  ``push`` returns what became final, ``flush`` the rest (inputs past the end are zeros)."""

    def __init__(self, src: int, dst, encoding: str = "pcm16", resample=None, encode=None):
        if encoding == "flac":
            raise ValueError("OutputStream: FLAC frames span blocks; put a FlacStream behind an OutputStream with encoding 'pcm16'")
        if encoding == "adpcm":
            raise ValueError("OutputStream: ADPCM blocks span blocks; put an AdpcmStream behind an OutputStream with encoding 'pcm16'")
        self.rate = None if dst is None or int(dst) == int(src) else int(dst)
        self.encoding = encoding
        if self.rate is not None:
            self.taps, self.up, self.down, self.skip = output_design(src, self.rate)
            self._resample = resample or (lambda x, m0, i0, n: resample_rows(x, self.taps, self.up, self.down, self.skip, m0, i0, n))
        self._encode = encode or (lambda y: encode_output(y, encoding))
        self.hist = np.zeros(0, np.int16)     # input samples i0 ... n_seen - 1
        self.i0 = 0
        self.n_seen = 0
        self.m_done = 0

    def _i_lo(self, m: int) -> int:
        lo = (m + self.skip) * self.down - int(self.taps.size) + 1
        return 0 if lo <= 0 else -(-lo // self.up)

    def _emit(self, m_end: int) -> np.ndarray:
        n_out = m_end - self.m_done
        if n_out <= 0:
            return np.zeros(0, np.int16)
        y = self._resample(self.hist, self.m_done, self.i0, n_out)
        self.m_done = m_end
        keep_from = min(self._i_lo(self.m_done), self.n_seen)      # the oldest sample the next output reads
        if keep_from > self.i0:
            self.hist, self.i0 = self.hist[keep_from - self.i0:], keep_from
        return y

    def push(self, block: np.ndarray) -> np.ndarray:
        block = np.asarray(block).reshape(-1)
        if self.rate is None:
            return self._encode(block) if self.encoding != "pcm16" else block
        self.hist = np.concatenate([self.hist, block.astype(np.int16, copy=False)])
        self.n_seen += block.size
        # outputs whose newest input is in hand: (m + skip) * down // up <= n_seen - 1
        m_end = max(self.m_done, resample_len(self.n_seen, self.up, self.down) - self.skip)
        y = self._emit(m_end)
        return self._encode(y) if self.encoding != "pcm16" else y

    def flush(self) -> np.ndarray:
        if self.rate is None:
            return np.zeros(0, np.uint8 if self.encoding != "pcm16" else np.int16)
        y = self._emit(resample_len(self.n_seen, self.up, self.down))
        return self._encode(y) if self.encoding != "pcm16" else y


class FlacStream:
    """FLAC for a STREAM of final int16 blocks at the output rate (``synthesize_stream``), behind the OutputStream.  Frames
    are independent, so it carries only the fewer-than-4096 samples that do not fill a frame yet and the next frame number.  The first
    ``push`` starts with the stream header (total samples 0 = not known), every ``push`` returns the whole frames in hand, ``flush`` the
    remainder as the final short frame.  The concatenation is a valid stream whose frames equal ``flac_encode_frames`` of the whole
    signal.  ``encode(pcm, frame0, last)`` returns the frames' bytes: the host mirror, or the device kernel
    (HipSynth.output_stream_backends).  With ``lpc_order`` 1 ... 12 (N16) the back end is called as
    ``encode(pcm, frame0, last, lpc_order)``."""

    def __init__(self, sample_rate: int, encode=None, lpc_order: int = 0):
        self.rate, self.lpc_order = _check_flac_rate(sample_rate), check_flac_lpc_order(lpc_order)
        encode = encode or (lambda pcm, frame0, last, order=0: flac_encode_frames(pcm, self.rate, frame0, last, order)[0])
        self._encode = encode if not self.lpc_order else (lambda pcm, frame0, last: encode(pcm, frame0, last, self.lpc_order))
        self.left = np.zeros(0, np.int16)
        self.frame = 0
        self.started = False

    def _out(self, pcm: np.ndarray, last: bool) -> np.ndarray:
        parts = []
        if not self.started:
            parts.append(np.frombuffer(flac_stream_header(self.rate, 0), np.uint8))
            self.started = True
        if pcm.size:
            parts.append(np.asarray(self._encode(pcm, self.frame, last), np.uint8).reshape(-1))
            self.frame += -(-pcm.size // FLAC_BLOCK)
        return np.concatenate(parts) if parts else np.zeros(0, np.uint8)

    def push(self, block: np.ndarray) -> np.ndarray:
        have = np.concatenate([self.left, _flac_pcm(block)])
        whole = have.size - have.size % FLAC_BLOCK
        self.left = have[whole:]
        return self._out(have[:whole], False)

    def flush(self) -> np.ndarray:
        rest, self.left = self.left, np.zeros(0, np.int16)
        return self._out(rest, True)


class AdpcmStream:
    """IMA ADPCM for a STREAM of final int16 blocks at the output rate (``synthesize_stream``), behind the OutputStream.
    Blocks are independent, so it carries only the samples that do not fill a block yet: ``push`` returns the bytes of every complete
    block, ``flush`` pads the rest and returns the last one.  The blocks come raw, as uint8 without a RIFF header (as the G.711 stream's
    codes do): their concatenation equals the ``data`` chunk of the file ``synthesize`` returns, byte for byte, and ``adpcm_wav`` puts a
    header in front of them.  ``encode(pcm)`` returns the blocks' bytes: the host mirror, or the device kernel
    (HipSynth.output_stream_backends)."""

    def __init__(self, sample_rate: int, encode=None):
        self.spb = adpcm_samples_per_block(adpcm_block_align(sample_rate))
        self._encode = encode or (lambda pcm: adpcm_encode_blocks(pcm, self.spb))
        self.left = np.zeros(0, np.int16)

    def _out(self, pcm: np.ndarray) -> np.ndarray:
        return np.asarray(self._encode(pcm), np.uint8).reshape(-1) if pcm.size else np.zeros(0, np.uint8)

    def push(self, block: np.ndarray) -> np.ndarray:
        have = np.concatenate([self.left, _adpcm_pcm(block)])
        whole = have.size - have.size % self.spb
        self.left = have[whole:]
        return self._out(have[:whole])

    def flush(self) -> np.ndarray:
        rest, self.left = self.left, np.zeros(0, np.int16)
        return self._out(rest)


class LimiterStream:
    """The limiter of DESIGN §8 N13 for a STREAM of joined blocks at the model rate (``synthesize_stream``).  A sample depends on the
    W = 2L + H samples on either side only, so ``push`` holds the newest W samples back, keeps W samples of context before them (2W of
    history in all) and returns what became final; ``flush`` returns the rest.  The concatenation equals ``limit_peaks`` of the whole
    signal bit for bit.  ``backend(hist, out_lo, out_n)`` computes the limiter over ``hist`` as a whole signal and returns
    y[out_lo, out_lo + out_n): the host mirror, or the device kernel (HipSynth.limiter_stream_backend)."""

    def __init__(self, sr: int, peak_dbfs: float = -1.0, mode: str = "true", backend=None, L: Optional[int] = None):
        if check_limiter(mode) is None:
            raise ValueError("LimiterStream: a mode is needed")
        self.L = limiter_lookahead(sr) if L is None else _check_lookahead(L)
        self.W = 2 * self.L + LIMIT_H
        self._backend = backend or (lambda hist, lo, n: limit_peaks(hist, sr, peak_dbfs, mode, 1.0, self.L)[0][lo: lo + n])
        self.hist = np.zeros(0, np.int16)     # input samples i0 ... n_seen - 1
        self.i0 = 0
        self.n_seen = 0
        self.done = 0                         # samples returned so far

    def _emit(self, end: int) -> np.ndarray:
        if end <= self.done:
            return np.zeros(0, np.int16)
        y = np.asarray(self._backend(self.hist, self.done - self.i0, end - self.done), np.int16).reshape(-1)
        self.done = end
        keep_from = max(self.done - self.W, 0)                    # the oldest sample the next output depends on
        if keep_from > self.i0:
            self.hist, self.i0 = self.hist[keep_from - self.i0:], keep_from
        return y

    def push(self, block: np.ndarray) -> np.ndarray:
        block = _as_pcm16(block)
        self.hist = np.concatenate([self.hist, block])
        self.n_seen += block.size
        return self._emit(self.n_seen - self.W)

    def flush(self) -> np.ndarray:
        return self._emit(self.n_seen)
