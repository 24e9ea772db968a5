#!/usr/bin/env python3
"""The kernels of csrc/vv_output.hip on the CPU under sanitizers, against the mirrors the GPU test uses.

Builds tools/output_host_check.cpp (the kernel source on tools/hip_host_shim.h, exact-size heap buffers) twice, with
-fsanitize=address,undefined and with -fsanitize=thread, and runs
  join     : the edge sets below at junction sizes 0, 1, 16 (exactly the ring C), 100 and 2400; with --reduced not, also the fixture's
             join_cases() grouped per (rate, duration) into one call each and the random sets of
             test_join_of_random_chunk_sets_equals_the_host_mirror.  Every result must equal
             AudioProcessor.concatenate_with_crossfade_improved, and no sample outside a request's slice may be written.
             Edge sets (n = the junction size asked for): chunks of 1, 2, 7, 8 and 9 samples between long ones; a chunk shorter than n
             and one shorter than 2 n; a single-chunk request; a 32767 as the first and as the last sample of a chunk; eight chunks
             that start 0 ... 7 samples past a 16-byte boundary, each with its 32767 in another part of the flag pass (head, vectors,
             tail); and a junction of 8191 samples, whose pairwise tree is 7 deep.  The plane starts with the first chunk and ends with the last one; out ends with the last request.
  resample : every rate of RATES, n in {1, 2, down - 1, down, down + 1, 3001} as ragged rows of one call, the whole fixture signal, and
             the signal in blocks of 997 through the (m0, i0) rows OutputStream hands over: within 1 LSB of the mirror at no more than
             1 sample in 10^4 (the kernel fuses each multiply-add, numpy does not), and the blocks equal to the whole bit for bit
  encode   : both laws, all 65536 inputs as one row, and the 36 rows of source offset 0 to 3 by length 1 to 9: equal to audioop's table
Every launch with a grid-stride loop has 2 workgroups along x where the device has more.  Needs no GPU.

    python tools/output_host_check.py [--cxx clang++] [--keep DIR] [--san asan|tsan|both] [--reduced]"""
import os
import struct
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import host_check_common as H  # noqa: E402
import numpy as np  # noqa: E402

NAME = "output"
RATES = [8000, 16000, 22050, 44100, 48000]
SENTINEL = -21846     # 0xAAAA: what the program fills every block with


def find_cxx():
    return H.find_cxx()


def build(cxx, work, san="asan"):
    return H.build(NAME, cxx, work, san)


# ------------------------------------------------------------------ join
def pack(chunk_sets, residues=None):
    """The chunks into one plane, the first at element 0, the last ending the plane, 32767 junk between them; residues = {(set, chunk):
    the chunk's start modulo 8}.  -> (plane, requests)"""
    parts, reqs, pos = [], [], 0
    for i, chunks in enumerate(chunk_sets):
        spans = []
        for k, c in enumerate(chunks):
            c = np.asarray(c).reshape(-1)
            gap = 0 if pos == 0 else 5
            if residues and (i, k) in residues:
                gap = (residues[(i, k)] - pos) % 8
            parts.append(np.full(gap, 32767, np.int16))
            pos += gap
            parts.append(c)
            spans.append((pos, c.size))
            pos += c.size
        reqs.append(spans)
    return np.concatenate(parts), reqs


def edge_sets(n, seed):
    """Chunk sets around a junction size of n samples (the docstring's list) -> (sets, residues)."""
    rng = np.random.default_rng(seed)

    def L(m, amp=3000):
        return np.clip(rng.standard_normal(m) * amp, -32768, 32766).astype(np.int16)
    first, last = L(n + 8), L(n + 9)
    first[0], last[-1] = 32767, 32767
    eight = [L(24 + 3 * k, 9000) for k in range(8)]
    for k, c in enumerate(eight):
        c[(0, c.size - 1, 9, 3, 17, 1, c.size - 2, 12)[k]] = 32767        # in the head, the vectors and the tail of the flag pass
    sets = [[L(3 * n + 5), L(1), L(2), L(7), L(8), L(9), L(3 * n + 1, 400)],
            [L(4 * n + 3), L(max(n - 1, 1)), L(max(2 * n - 1, 1)), L(3 * n + 2, 12000)],
            [L(5)],
            [first, last, L(40)],
            eight,
            [L(1)],
            [L(1), L(1)]]
    return sets, {(4, k): k for k in range(8)}


DEEP = (8191, 24000, 8191 / 24000 + 1e-9)      # a junction whose pairwise tree is 7 deep: the only lengths at which np_buffer_sum's first
                                               # barrier orders anything (below, the barriers of the empty tree levels do)


def deep_tree_sets(seed=8191):
    rng = np.random.default_rng(seed)
    return [[np.clip(rng.standard_normal(m) * a, -32768, 32766).astype(np.int16) for m, a in ((8200, 3000), (8195, 9000), (8191, 400))],
            [np.clip(rng.standard_normal(5) * 3000, -32768, 32766).astype(np.int16)]]


def run_join(exe, work, sets, d, sr, residues=None):
    from vietvoice_tts_amd.core import AudioProcessor
    from vietvoice_tts_amd.pcm_stage import plan_join
    plane, requests = pack(sets, residues)
    rows, reqs, lens, ns, total = plan_join(requests, d, sr, n_pcm=plane.size)
    off, tabs, at = {}, [], 0
    for n in ns:
        theta = np.linspace(0, np.pi / 2, n)
        off[n] = at
        tabs += [np.cos(theta) ** 2, np.sin(theta) ** 2]
        at += 2 * n
    for row in rows:
        row[5] = off[row[3]] if row[3] > 0 else 0
    fade = np.concatenate(tabs) if tabs else np.zeros(0)
    max_len = max(r[1] for r in rows)
    bx = min(max((max_len // 4 + 256) // 256, 1), 1024)
    fin, fout = os.path.join(work, "join_in.bin"), os.path.join(work, "join_out.bin")
    with open(fin, "wb") as f:
        f.write(struct.pack("<7q", plane.size, len(rows), len(reqs), fade.size, total, max(ns, default=0), min(bx, 2)))
        f.write(np.array(rows, np.int64).tobytes() + np.array(reqs, np.int64).tobytes() + fade.astype(np.float64).tobytes() + plane.tobytes())
    H.run(exe, ["join", fin, fout])
    out = np.fromfile(fout, np.int16, offset=8 * len(rows))
    written = np.zeros(total, bool)
    bad = []
    for i, (chunks, rq, n) in enumerate(zip(sets, reqs, lens)):
        want = np.asarray(AudioProcessor.concatenate_with_crossfade_improved([c.copy() for c in chunks], d, sr)).reshape(-1)
        written[rq[2]: rq[2] + n] = True
        if not (want.size == n and np.array_equal(out[rq[2]: rq[2] + n], want)):
            bad.append(i)
    if not (out[~written] == SENTINEL).all():
        bad.append("a sample outside a request's slice was written")
    return bad


def join_checks(exe, work, reduced):
    for n, sr, d in ((0, 8000, 0.0), (1, 8000, 1 / 8000 + 1e-9), (16, 8000, 0.002 + 1e-9), (100, 16000, 100 / 16000 + 1e-9), (2400, 24000, 0.1)):
        assert int(d * sr) == n
        sets, res = edge_sets(n, seed=n)
        yield H.check(f"join edges n {n}", not run_join(exe, work, sets, d, sr, res))
        yield H.check(f"join edges n {n}, the single chunks alone", not run_join(exe, work, [sets[2], sets[5]], d, sr))
    n, sr, d = DEEP
    assert int(d * sr) == n
    yield H.check(f"join a junction of {n} samples (a 7-deep pairwise tree)", not run_join(exe, work, deep_tree_sets(), d, sr))
    if reduced:
        return
    from tests.output_util import join_cases
    groups = {}
    for case in join_cases():
        groups.setdefault((case[1], case[2]), []).append(case)
    for (sr, d), cs in groups.items():
        bad = run_join(exe, work, [c[3] for c in cs], d, sr)
        yield H.check(f"join fixture {sr} Hz {d:.6f} s ({len(cs)} requests)", not bad)
    rng = np.random.default_rng(77)                                      # test_join_of_random_chunk_sets_equals_the_host_mirror
    for sr, d in ((24000, 0.1), (16000, 0.01), (8000, 0.0)):
        n = int(d * sr)
        sets = []
        for _ in range(12):
            k = int(rng.integers(1, 7))
            lens = [int(rng.choice([1, 2, max(n - 1, 1), n + 1, 2 * n + 3, 3000, 5001])) for _ in range(k)]
            chunks = [np.clip(rng.standard_normal(m) * rng.choice([20, 400, 3000, 12000]), -32768, 32767).astype(np.int16) for m in lens]
            if rng.random() < 0.3:
                chunks[int(rng.integers(k))][0] = 32767
            sets.append(chunks)
        yield H.check(f"join random sets {sr} Hz {d} s", not run_join(exe, work, sets, d, sr))


# ------------------------------------------------------------------ output rate
def run_resample(exe, work, parts, dst):
    """parts = [(x, m0, i0, n_out)] as the rows of one call, inputs and outputs back to back -> the outputs"""
    from vietvoice_tts_amd.core.audio_processor import output_design
    taps, up, down, skip = output_design(24000, dst)
    rows, so, do = [], 0, 0
    for x, m0, i0, n_out in parts:
        rows.append([so, x.size, do, n_out, m0, i0])
        so, do = so + x.size, do + n_out
    max_out = max(r[3] for r in rows)
    bx = min((max_out + 255) // 256, 4096)
    fin, fout = os.path.join(work, "rs_in.bin"), os.path.join(work, "rs_out.bin")
    with open(fin, "wb") as f:
        f.write(struct.pack("<8q", so, len(rows), taps.size, up, down, skip, do, max(min(bx, 2), 1)))
        f.write(np.array(rows, np.int64).tobytes() + np.ascontiguousarray(taps, np.float64).tobytes())
        f.write(np.concatenate([p[0] for p in parts]).astype(np.int16).tobytes())
    H.run(exe, ["resample", fin, fout])
    y = np.fromfile(fout, np.int16)
    return [y[r[2]: r[2] + r[3]] for r in rows]


def within_lsb(got, want):
    d = np.abs(got.astype(np.int64) - want.astype(np.int64))
    return got.shape == want.shape and d.max(initial=0) <= 1 and int((d > 0).sum()) * 10000 <= max(got.size, 1)


def resample_checks(exe, work, reduced):
    from tests.output_util import golden
    from vietvoice_tts_amd.core.audio_processor import OutputStream, output_design, resample_len, resample_rows
    x = golden()[1]["poly_x"]
    for dst in RATES:
        taps, up, down, skip = output_design(24000, dst)
        sizes = sorted({n for n in (1, 2, down - 1, down, down + 1, 3001) if n >= 1})
        parts = [(x[k: k + n], 0, 0, resample_len(n, up, down)) for k, n in enumerate(sizes)]
        got = run_resample(exe, work, parts, dst)
        ok = all(within_lsb(g, resample_rows(p[0], taps, up, down, skip, 0, 0, p[3])) for g, p in zip(got, parts))
        yield H.check(f"resample {dst} Hz sizes {sizes}", ok)
        xs = x if not reduced else x[:2991]                              # three blocks of 997
        whole = run_resample(exe, work, [(xs, 0, 0, resample_len(xs.size, up, down))], dst)[0]
        yield H.check(f"resample {dst} Hz {xs.size} samples", within_lsb(whole, resample_rows(xs, taps, up, down, skip, 0, 0, whole.size)))
        blocks = []

        def record(h, m0, i0, n):
            blocks.append((h.copy(), m0, i0, n))
            return np.zeros(n, np.int16)
        s = OutputStream(24000, dst, "pcm16", record, None)
        for i in range(0, xs.size, 997):
            s.push(xs[i: i + 997])
        s.flush()
        got = np.concatenate(run_resample(exe, work, blocks, dst))
        yield H.check(f"resample {dst} Hz blocks of 997 ({len(blocks)} rows)", np.array_equal(got, whole))


# ------------------------------------------------------------------ G.711
def encode_checks(exe, work, reduced):
    from tests.output_util import golden
    every = np.arange(-32768, 32768, dtype=np.int16)
    fin, fout = os.path.join(work, "enc_in.bin"), os.path.join(work, "enc_out.bin")
    for kind, enc in ((1, "ulaw"), (2, "alaw")):
        table = golden()[1][f"g711_{enc}"]
        small, pos = [], 3
        for so in range(4):
            for n in range(1, 10):
                small.append([30000 + 1000 * len(small) + so, n, pos])
                pos += n + ((len(small) + 1) % 3 if len(small) < 36 else 0)
        for label, rows, n_y in (("all 65536 inputs", [[0, 65536, 0]], 65536), ("36 rows of offset 0..3 x length 1..9", small, pos)):
            max_n = max(r[1] for r in rows)
            bx = min((max_n // 8 + 256) // 256, 2048)
            with open(fin, "wb") as f:
                f.write(struct.pack("<5q", every.size, len(rows), kind, n_y, min(bx, 2)) + np.array(rows, np.int64).tobytes() + every.tobytes())
            H.run(exe, ["encode", fin, fout])
            y = np.fromfile(fout, np.uint8)
            written = np.zeros(n_y, bool)
            ok = y.size == n_y
            for so, n, do in rows:
                written[do: do + n] = True
                ok = ok and np.array_equal(y[do: do + n], table[so: so + n])
            yield H.check(f"encode {enc} {label}", ok and (y[~written] == 0xAA).all())


def cases(exe, work, reduced=False):
    yield from join_checks(exe, work, reduced)
    yield from resample_checks(exe, work, reduced)
    yield from encode_checks(exe, work, reduced)


if __name__ == "__main__":
    H.main(NAME, cases, __doc__)
