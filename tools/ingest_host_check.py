#!/usr/bin/env python3
"""The kernels of csrc/vv_ingest.hip on the CPU under sanitizers (N3 / a8), against the mirrors the GPU tests use.

Builds tools/ingest_host_check.cpp (the kernel source on tools/hip_host_shim.h, exact-size heap buffers) twice, with
-fsanitize=address,undefined and with -fsanitize=thread, and runs
  ingest    : the 25 fixture clips in one batch (== the fixture's audioop samples); the 3 to 6 channel and 8 / 32-bit clips of
              test_many_channels_and_widths_on_device with clips of 1 and 2 frames and same-rate clips (I == O) in one batch, and one
              clip of 4096 * 256 + 257 outputs, past the device's grid (== tomono + ratecv of the host loader).  The PCM bytes start with
              the first clip and end with the last one; 2 workgroups along x where the device has up to 4096
  normalize : per length of test_normalize_clips_bit_exact_numpy up to 16385 (with --reduced not, also 24000 and 65537) its four clips,
              the degenerate clips (silence, pure DC, one sample), and a zero-length clip between two others == normalize_to_int16; the
              scratch is one block of exactly vv_normalize_scratch_bytes, the only check its slot arithmetic off / 8192 + clip gets
  resample  : the four rates of test_resample_poly_matches_host_mirror, within that test's bound of the host's polyphase resampler
Needs no GPU.

    python tools/ingest_host_check.py [--cxx clang++] [--keep DIR] [--san asan|tsan|both] [--reduced]"""
import importlib.util
import json
import os
import struct
import sys
from math import gcd

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import host_check_common as H  # noqa: E402
import numpy as np  # noqa: E402

NAME = "ingest"
SR = 24000
GOLDEN = os.path.join(H.ROOT, "tests", "golden")
LENGTHS = [1, 5, 7, 8, 9, 127, 128, 129, 130, 143, 144, 255, 257, 1000, 4097, 8191, 8192, 8193, 16384, 16385]
BIG = 4096 * 256 + 257


def find_cxx():
    return H.find_cxx()


def build(cxx, work, san="asan"):
    return H.build(NAME, cxx, work, san)


def _generator():
    spec = importlib.util.spec_from_file_location("make_ingest_golden", os.path.join(GOLDEN, "make_ingest_golden.py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


def mirror_samples(frames, rate):
    from vietvoice_tts_amd.core.audio_processor import ratecv, tomono
    return ratecv(tomono(frames), rate, SR).astype(np.float32)


def run_ingest(exe, work, clips):
    """clips = [(frames (n, ch) int8 | int16 | int32, rate, want f32)] in one launch -> the clips that differ"""
    from vietvoice_tts_amd.core.audio_processor import ratecv_len
    parts, desc, pos, out_pos = [], [], 0, 0
    for j, (frames, rate, _want) in enumerate(clips):
        raw = frames.tobytes()
        g = gcd(rate, SR)
        n = frames.shape[0]
        n_out = ratecv_len(n, rate, SR) if rate != SR else n
        desc.append([pos, frames.dtype.itemsize, frames.shape[1], n, rate // g, SR // g, out_pos, n_out])
        pad = -len(raw) % 4 if j + 1 < len(clips) else 0                 # the last clip ends the buffer
        parts.append(raw + b"\0" * pad)
        pos, out_pos = pos + len(raw) + pad, out_pos + n_out
    bx = min((max(d[7] for d in desc) + 255) // 256, 4096)
    fin, fout = os.path.join(work, "ingest_in.bin"), os.path.join(work, "ingest_out.bin")
    with open(fin, "wb") as f:
        f.write(struct.pack("<4q", pos, len(desc), out_pos, min(bx, 2)) + np.array(desc, np.int64).tobytes() + b"".join(parts))
    H.run(exe, ["ingest", fin, fout])
    y = np.fromfile(fout, np.float32)
    return [j for j, (d, c) in enumerate(zip(desc, clips))
            if not (c[2].size == d[7] and np.array_equal(y[d[6]: d[6] + d[7]].view(np.uint32), c[2].view(np.uint32)))]


def ingest_checks(exe, work, reduced):
    from vietvoice_tts_amd.core import AudioProcessor
    gold = json.load(open(os.path.join(GOLDEN, "ingest_golden.json")))
    npz = np.load(os.path.join(GOLDEN, "ingest_golden.npz"))
    gen = _generator()
    clips = []
    for c in gold["cases"]:
        frames, _w, rate = AudioProcessor.decode(gen.wav_bytes(gen.make_clip(c["seed"], c["n_frames"], c["channels"], c["rate"], c["width"]), c["rate"], c["width"]))
        clips.append((frames, rate, npz[c["key"] + "_samples"].astype(np.float32)))
    yield H.check("ingest the 25 fixture clips in one batch", not run_ingest(exe, work, clips))
    rng = np.random.default_rng(3)
    clips = []

    def clip(n, ch, rate, width):
        info = np.iinfo({1: np.int8, 2: np.int16, 4: np.int32}[width])
        frames = rng.integers(info.min // 2, info.max // 2, size=(n, ch)).astype(info.dtype)
        clips.append((frames, rate, mirror_samples(frames, rate)))
    for ch, rate, width in ((3, 48000, 2), (6, 44100, 2), (4, 16000, 1), (5, 22050, 4), (3, 24000, 2)):      # test_many_channels_and_widths_on_device
        clip(3001, ch, rate, width)
    for n in (1, 2):
        for ch, rate, width in ((1, 8000, 2), (2, 48000, 2), (1, 24000, 1), (3, 24000, 4), (2, 44100, 1)):
            clip(n, ch, rate, width)
    clip(777, 1, 24000, 2)                                               # I == O
    clip(1, 1, 44100, 1)                                                 # the last byte of the buffer is the only frame of a clip
    yield H.check("ingest channels 3..6, widths 1 / 2 / 4, clips of 1 and 2 frames, I == O", not run_ingest(exe, work, clips))
    clips = []
    clip((BIG - 1) // 2 + 1, 1, 12000, 2)
    assert clips[0][2].size == BIG
    clip(3, 2, 16000, 2)
    yield H.check(f"ingest a clip of {BIG} outputs (a second trip on the device's grid)", not run_ingest(exe, work, clips))


def run_normalize(exe, work, clips):
    from vietvoice_tts_amd.core import AudioProcessor
    off = np.concatenate([[0], np.cumsum([len(c) for c in clips])]).astype(np.int64)
    max_len = max(len(c) for c in clips)
    n_chunks = (max_len + 8191) // 8192
    bx = min((max_len + 2047) // 2048, 256)
    fin, fout = os.path.join(work, "norm_in.bin"), os.path.join(work, "norm_out.bin")
    with open(fin, "wb") as f:
        f.write(struct.pack("<5q", len(clips), int(off[-1]), max_len, min(n_chunks, 2), min(bx, 2)) + off.tobytes())
        f.write(np.concatenate(clips).astype(np.float32).tobytes())
    H.run(exe, ["normalize", fin, fout])
    out = np.fromfile(fout, np.int16)
    return [j for j, c in enumerate(clips) if len(c) and not np.array_equal(out[off[j]: off[j + 1]], AudioProcessor.normalize_to_int16(c))]


def normalize_checks(exe, work, reduced):
    for n in LENGTHS + ([] if reduced else [24000, 65537]):
        rng = np.random.default_rng(n)
        clips = [(rng.standard_normal(n) * s + o).astype(np.float32) for s, o in ((3000.0, 120.0), (0.1, 0.0), (9000.0, -400.0))]
        clips.append(np.rint(rng.standard_normal(n) * 8000 + 500).astype(np.float32))
        yield H.check(f"normalize four clips of {n}", not run_normalize(exe, work, clips))
    clips = [np.zeros(500, np.float32), np.full(300, 7.0, np.float32), np.array([5.0], np.float32)]
    yield H.check("normalize silence, pure DC, one sample", not run_normalize(exe, work, clips))
    rng = np.random.default_rng(5)
    clips = [(rng.standard_normal(8193) * 3000).astype(np.float32), np.zeros(0, np.float32), (rng.standard_normal(8191) * 500 + 40).astype(np.float32)]
    yield H.check("normalize a zero-length clip between two others", not run_normalize(exe, work, clips))
    yield H.check("normalize a zero-length clip first and last", not run_normalize(exe, work, [clips[1], clips[2], clips[1]]))


def resample_checks(exe, work, reduced):
    from vietvoice_tts_amd.core.audio_processor import _resample_polyphase
    from vietvoice_tts_amd.voice_bank import resample_design
    fin, fout = os.path.join(work, "poly_in.bin"), os.path.join(work, "poly_out.bin")
    for src in (48000, 16000, 44100, 22050):
        rng = np.random.default_rng(src)
        x = (rng.standard_normal(src // 3 + 17) * 5000).astype(np.float32)
        want = _resample_polyphase(x, src, SR)
        taps, up, down, skip = resample_design(src, SR)
        n_out = -(-(x.size * up) // down)
        with open(fin, "wb") as f:
            f.write(struct.pack("<6q", x.size, taps.size, up, down, skip, n_out) + np.ascontiguousarray(taps, np.float64).tobytes() + x.tobytes())
        H.run(exe, ["resample", fin, fout])
        got = np.fromfile(fout, np.float32)
        ok = got.shape == want.shape and np.abs(got - want).max() <= 2e-3 * 1 + 1e-6 * np.abs(want).max()       # the GPU test's bound
        yield H.check(f"resample_poly {src} Hz", ok)


def cases(exe, work, reduced=False):
    yield from ingest_checks(exe, work, reduced)
    yield from normalize_checks(exe, work, reduced)
    yield from resample_checks(exe, work, reduced)


if __name__ == "__main__":
    H.main(NAME, cases, __doc__)
