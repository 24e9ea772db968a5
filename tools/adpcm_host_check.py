#!/usr/bin/env python3
"""The kernels of csrc/vv_adpcm.hip on the CPU under sanitizers, against the mirror of core/audio_processor.py.

Builds tools/adpcm_host_check.cpp (the kernel source on tools/hip_host_shim.h, exact-size heap buffers, its own main) twice, with
-fsanitize=address,undefined and with -fsanitize=thread, and runs:
  encoder   the inputs of tests/adpcm_util.py (the speech stand-in at n = 1, 2, spb - 1, spb, spb + 1, 2 spb, 3 spb + 7; silence; the
            full-scale square wave; the ramp) at spb = 505, 1017, 2041 as ONE ragged launch per block size: x is one exact block with 3
            samples of junk between the signals, y one exact block with 4 to 16 untouched bytes between the rows' blocks, which must keep
            their 0xAA fill; the grid has fewer workgroups than blocks, so that the block loop takes further trips
  decoder   the files of tests/adpcm_util.py (mu-law, A-law, mono and stereo ADPCM, a fact cap, partial last blocks) as ONE launch of the
            header check, the ADPCM decoder and the G.711 decoder; data and pcm are exact blocks, the gaps between the clips keep the fill
  damaged   every single-byte truncation of the data chunk of one small mono and one small stereo file, and every single-bit flip of
            their block headers: frames equal the mirror's, or the status equals the mirror's refusal {reason, byte}; a refused clip
            writes nothing outside its own frames
The reduced list (the suite's) keeps spb = 505 of the encoder and every 3rd truncation; every edge stays.  Needs no GPU.

    python tools/adpcm_host_check.py [--cxx clang++] [--keep DIR] [--san asan|tsan|both] [--reduced]"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import host_check_common as H  # noqa: E402
import numpy as np  # noqa: E402

NAME = "adpcm"


def find_cxx():
    return H.find_cxx()


def build(cxx, work, san="asan"):
    return H.build(NAME, cxx, work, san)


def _mods():
    from vietvoice_tts_amd.core import audio_processor as ap
    from tests import adpcm_util as U
    return ap, U


def encoder_launch(bt, sigs, spb):
    """One ragged launch -> (launch id, per signal (byte offset in y, bytes), y's size)."""
    ba = (spb - 1) // 2 + 4
    plane, offs = H.pack_signals(sigs)
    rows, at, spans = [], 0, []
    for k, (s, so) in enumerate(zip(sigs, offs)):
        nb = -(-len(s) // spb)
        if k:
            at += 4 * (1 + k % 4)                         # untouched bytes between the rows, dst_off stays a multiple of 4
        rows.append([so, len(s), at])
        spans.append((at, nb * ba))
        at += nb * ba
    most = max(n for _o, n in spans) // ba
    lid = bt.add("adpcm_encode", (max(1, min(most - 1, 2)), len(sigs)), 128,
                 [plane, plane.size, np.array(rows, np.int64), spb, H.filled((at,), np.uint8), at])
    return lid, spans, at


def decoder_launch(bt, ap, infos):
    """The three decoder launches over the WavInfo ``infos`` -> (ids, rows, pcm size)."""
    rows, parts, pos, ppos = [], [], 0, 0
    for k, fi in enumerate(infos):
        n = len(fi.data)
        frames = ap.wav_coded_frame_count(fi)
        ppos = -(-ppos // 16) * 16 + (16 if k % 2 else 0)  # gaps of 16 bytes before every other clip
        rows.append([pos, n, fi.tag, fi.channels, fi.block_align, frames, ppos, 0])
        parts.append(np.frombuffer(fi.data, np.uint8))
        pad = -n % 16
        if k + 1 < len(infos):
            parts.append(np.full(pad, 0x5A, np.uint8))
            pos += n + pad
        else:
            pos += n                                       # the last clip ends the data block: nothing behind it may be read
        ppos += frames * fi.channels * 2
    data = np.concatenate(parts) if pos else np.zeros(0, np.uint8)
    rows_a = np.array(rows, np.int64)
    n_pcm = max(ppos, 0)
    heads = max([(r[1] // r[4] + (r[1] % r[4] >= 4 * r[3])) * r[3] for r in rows if r[2] == 0x11], default=0)
    codes = max([r[5] * r[3] for r in rows if r[2] != 0x11], default=0)
    pcm = H.filled((n_pcm,), np.uint8)
    ids = [bt.add("wav_check", len(rows), 256, [data, data.size, rows_a, n_pcm, H.filled((len(rows), 2), np.int64)])]
    ids.append(bt.add("adpcm_decode", (max(1, min(2, -(-heads // 256))), len(rows)), 256, [data, data.size, rows_a, pcm, n_pcm]) if heads else None)
    ids.append(bt.add("g711_decode", (max(1, min(2, -(-(codes // 8 + 1) // 256))), len(rows)), 256, [data, data.size, rows_a, pcm, n_pcm]) if codes else None)
    return ids, rows, n_pcm


def decoder_verdict(ap, infos, rows, n_pcm, status, pcm_a, pcm_g):
    """status [R][2] and the pcm blocks after the ADPCM and the G.711 launch (either may be None) -> everything equals the mirror."""
    good, owned = True, np.zeros(n_pcm, bool)
    for fi, r, st in zip(infos, rows, status):
        lo, nbytes = r[6], r[5] * r[3] * 2
        owned[lo: lo + nbytes] = True
        pcm = pcm_a if fi.tag == 0x11 else pcm_g
        try:
            want = ap.wav_coded_frames(fi)
        except ap.WavError as e:
            good &= (int(st[0]), int(st[1])) == (e.code, e.position - fi.data_at)
            continue
        good &= (int(st[0]), int(st[1])) == (0, 0)
        good &= nbytes == 0 or (pcm is not None and np.array_equal(pcm[lo: lo + nbytes].view("<i2").reshape(-1, r[3]), want))
    for pcm in (pcm_a, pcm_g):
        good &= pcm is None or H.still_filled(pcm[~owned])
    return bool(good)


def cases(exe, work, reduced=False):
    """Runs every case through exe; yields (label, equal to the mirror)."""
    ap, U = _mods()
    bt = H.Batch(exe, work, NAME)
    # ---- encoder
    enc = []
    for spb in (U.SPBS[:1] if reduced else U.SPBS):
        names, sigs = zip(*U.encoder_inputs(spb))
        enc.append((spb, names, sigs) + encoder_launch(bt, sigs, spb))
    # ---- decoder: the files, then the damaged ones
    files = U.decoder_files()
    infos = [ap.wav_container(d) for _n, d, _w, _r in files]
    dec = [("files", infos) + decoder_launch(bt, ap, infos)]
    for name, data, data_at in U.small_files():
        fi = ap.wav_container(data)
        cuts = [fi._replace(data=fi.data[:k], fact=None) for k in range(0, len(fi.data), 3 if reduced else 1)]
        dec.append((f"{name} truncations", cuts) + decoder_launch(bt, ap, cuts))
        flips = []
        for b in range(len(fi.data) // fi.block_align):
            for byte in range(4 * fi.channels):
                for bit in range(8):
                    d = bytearray(fi.data)
                    d[b * fi.block_align + byte] ^= 1 << bit
                    flips.append(fi._replace(data=bytes(d)))
        for lo in range(0, len(flips), 64):
            dec.append((f"{name} header bit flips {lo}", flips[lo: lo + 64]) + decoder_launch(bt, ap, flips[lo: lo + 64]))
    bad, _at = U.bad_index_file(2)
    mixed = [infos[0], ap.wav_container(bad), infos[-1], infos[5]]
    dec.append(("a bad step index among good clips", mixed) + decoder_launch(bt, ap, mixed))
    res = bt.run()
    for spb, names, sigs, lid, spans, total in enc:
        y = res[lid][4]
        owned = np.zeros(total, bool)
        for name, s, (lo, n) in zip(names, sigs, spans):
            owned[lo: lo + n] = True
            yield H.check(f"encode spb {spb} {name}", np.array_equal(y[lo: lo + n], ap.adpcm_encode_blocks(s, spb)))
        yield H.check(f"encode spb {spb}: bytes between the rows untouched", H.still_filled(y[~owned]))
    for label, fis, ids, rows, n_pcm in dec:
        status = res[ids[0]][4]
        pcm_a = res[ids[1]][3] if ids[1] is not None else None
        pcm_g = res[ids[2]][3] if ids[2] is not None else None
        yield H.check(f"decode {label} ({len(fis)} clips)", decoder_verdict(ap, fis, rows, n_pcm, status, pcm_a, pcm_g))


if __name__ == "__main__":
    H.main(NAME, cases, __doc__)
