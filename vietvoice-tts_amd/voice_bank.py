"""Device-resident voice bank: reference clips are decoded once, mixed to mono, rate-converted and
DC/peak-normalised ON THE GPU with the reference's own arithmetic, and kept in HBM keyed by content, so a request for a
known voice costs a dictionary lookup.

The reference re-opens the model tar, re-decodes and re-normalises the clip on every call
(core/model.py:204-211, core/audio_processor.py:15-44) and carries an unused ``sample_cache``
(core/tts_engine.py:30).  Here:

  host   : RIFF/WAVE and FLAC container parsing (no arithmetic on samples), one descriptor row per clip
  device : vv_flac_index + vv_flac_decode = a FLAC clip's frames -> the same interleaved PCM bytes a WAV clip uploads (N17, RFC 9639)
  device : vv_wav_decode = a G.711 or IMA ADPCM WAVE clip's data chunk -> interleaved int16 frames in that same buffer (N25, audioop's arithmetic)
  device : vv_ingest_pcm  = pydub set_channels(1) / set_frame_rate = audioop.tomono + audioop.ratecv, -> float32
           vv_normalize_clips = numpy-ordered float32 mean / peak / scale / int16 truncation
           -- bit-exact to AudioProcessor.load_audio (tests/test_ingest_gpu.py); clips of one ``ingest_many`` call batched on grid.y
  opt-in : ``resampler="polyphase"`` keeps the band-limited FIR of earlier rounds (vv_resample_poly; not the reference's arithmetic)

An entry keeps the int16 clip on the device (what vv_preprocess reads) plus one host copy (what the reference-style
session path and the duration model read).  LRU eviction by a byte budget; 239 built-in voices of ~8 s are ~90 MB.
"""
from __future__ import annotations

import hashlib
import os
from collections import OrderedDict
from math import gcd
from typing import Dict, List, Tuple, Union

import numpy as np

from .core.audio_processor import AudioProcessor, WavError, is_flac, ratecv_len, tomono, wav_coded_frame_count, wav_container


def resample_design(src: int, dst: int) -> Tuple[np.ndarray, int, int, int]:
    """(taps f64 with the leading zero pad, up, down, skip): the filter the host mirror's polyphase resampler uses
    (Kaiser beta 5, half length 10 * max(up, down), gain = up), cut so that y[n] = sum_i x[i] * taps[(n+skip)*down - i*up]."""
    from scipy.signal import firwin
    g = gcd(src, dst)
    up, down = dst // g, src // g
    max_rate = max(up, down)
    half_len = 10 * max_rate
    h = firwin(2 * half_len + 1, 1.0 / max_rate, window=("kaiser", 5.0)) * up
    n_pre_pad = down - half_len % down
    skip = (half_len + n_pre_pad) // down
    return np.concatenate([np.zeros(n_pre_pad), h]).astype(np.float64), up, down, skip


def _coded_wav(data: bytes):
    """The WavInfo of a RIFF/WAVE file whose format tag (WAVE_FORMAT_EXTENSIBLE resolved) is 6, 7 or 0x11 (N25), else None; what is
    malformed is AudioProcessor.decode's to refuse, with the same error."""
    if data[:4] != b"RIFF":
        return None
    try:
        info = wav_container(data)
    except WavError:
        raise
    except ValueError:
        return None
    return info if info.tag in (6, 7, 0x11) else None


class VoiceEntry:
    __slots__ = ("key", "pcm_dev", "pcm_host", "n_samples", "nbytes")

    def __init__(self, key, pcm_dev, pcm_host):
        self.key, self.pcm_dev, self.pcm_host = key, pcm_dev, pcm_host
        self.n_samples = int(pcm_host.shape[0])
        self.nbytes = self.n_samples * 2


class VoiceBank:
    def __init__(self, synth, sample_rate: int, max_bytes: int = 1 << 30, resampler: str = "ratecv"):
        if resampler not in ("ratecv", "polyphase"):
            raise ValueError(f"unknown resampler {resampler!r}")
        self.synth, self.sample_rate, self.max_bytes, self.resampler = synth, int(sample_rate), int(max_bytes), resampler
        self._entries: "OrderedDict[str, VoiceEntry]" = OrderedDict()
        self._by_host: Dict[int, VoiceEntry] = {}
        self._taps = {}
        self.bytes = 0
        self.hits = self.misses = 0

    @staticmethod
    def key_of(path_or_bytes: Union[str, bytes]) -> str:
        if isinstance(path_or_bytes, str):
            st = os.stat(path_or_bytes)           # FileNotFoundError propagates like the reference's check (:19-20)
            return f"file:{os.path.abspath(path_or_bytes)}:{st.st_mtime_ns}:{st.st_size}"
        return "sha1:" + hashlib.sha1(bytes(path_or_bytes)).hexdigest()

    def get(self, path_or_bytes: Union[str, bytes]) -> VoiceEntry:
        return self.ingest_many([path_or_bytes])[0]

    def entry_for_host(self, pcm_host: np.ndarray):
        """The entry whose host copy is this very array (how _synthesize_device finds the device clip of an input tuple)."""
        base = pcm_host.base if pcm_host.base is not None else pcm_host
        return self._by_host.get(id(base))

    def ingest_many(self, items: List[Union[str, bytes]]) -> List[VoiceEntry]:
        import torch
        keys = []
        for it in items:
            if isinstance(it, str) and not os.path.exists(it):
                raise FileNotFoundError(f"Audio file not found: {it}")
            keys.append(self.key_of(it))
        todo: Dict[str, Union[str, bytes]] = {}
        for k, it in zip(keys, items):
            if k in self._entries:
                self.hits += 1
                self._entries.move_to_end(k)
            elif k not in todo:
                self.misses += 1
                todo[k] = it
            else:
                self.hits += 1                    # repeated inside this call: ingested once
        if todo:
            dev = self.synth.device
            raw = [AudioProcessor._read_bytes(it) for it in todo.values()]
            flac = {j: d for j, d in enumerate(raw) if d[:4] != b"RIFF" and is_flac(d)}        # N17: decoded on the device
            if flac and self.resampler != "ratecv":                                 # opt-in path: device-decoded frames come back
                back = self._flac_frames(list(flac.values()))
                flac = dict(zip(flac, back))
            coded = {j: fi for j, fi in enumerate(_coded_wav(d) for d in raw) if fi is not None}      # N25: G.711 / IMA ADPCM, decoded on the device
            if coded and self.resampler != "ratecv":
                back = self._wav_frames(list(coded.values()))
                coded = dict(zip(coded, back))
            on_dev = {**flac, **coded}
            decoded = [on_dev[j] if j in on_dev and self.resampler != "ratecv" else None if j in on_dev else AudioProcessor.decode(d)
                       for j, d in enumerate(raw)]                                   # host: container parsing only
            if any(d is not None and d[0].shape[0] == 0 for d in decoded):
                raise ValueError("empty audio clip")
            if self.resampler == "ratecv":
                x, lens = self._ingest_ratecv(decoded, dev, flac, coded)
            else:
                x, lens = self._ingest_polyphase(decoded, dev)
            off = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
            pcm = self.synth.normalize_clips(x, torch.from_numpy(off).to(dev), max_len=max(lens))
            host = pcm.cpu().numpy()
            for j, k in enumerate(todo):
                e = VoiceEntry(k, pcm[off[j]: off[j + 1]].clone(), host[off[j]: off[j + 1]].copy())
                self._entries[k] = e
                self._by_host[id(e.pcm_host)] = e
                self.bytes += e.nbytes
            while self.bytes > self.max_bytes and len(self._entries) > len(set(keys)):
                k0 = next(iter(self._entries))
                if k0 in keys:
                    self._entries.move_to_end(k0)
                    continue
                old = self._entries.pop(k0)
                self._by_host.pop(id(old.pcm_host), None)
                self.bytes -= old.nbytes
        return [self._entries[k] for k in keys]

    def _flac_frames(self, files):
        """FLAC files -> [(frames (n, channels), width, rate)] through the device decoder, copied back (the opt-in polyphase path)."""
        pcm, res = self.synth.flac_clips(files)
        host, out = pcm.cpu().numpy(), []
        for r in res:
            if isinstance(r, Exception):
                raise r
            off, n, width, rate, ch = r
            out.append((host[off: off + n * ch * width].view({1: np.int8, 2: np.int16, 4: np.int32}[width]).reshape(n, ch).copy(), width, rate))
        return out

    def _wav_frames(self, infos):
        """Coded WAVE clips (N25) -> [(frames (n, channels), 2, rate)] through the device decoder, copied back (the opt-in polyphase path)."""
        pcm, res = self.synth.wav_clips(infos)
        host, out = pcm.cpu().numpy(), []
        for r in res:
            if isinstance(r, Exception):
                raise r
            off, n, _width, rate, ch = r
            out.append((host[off: off + n * ch * 2].view(np.int16).reshape(n, ch).copy(), 2, rate))
        return out

    def _ingest_ratecv(self, decoded, dev, flac=None, coded=None):
        """One vv_ingest_pcm launch for all clips: interleaved PCM bytes back to back (4-byte aligned) + descriptor rows.  A FLAC clip
        (``decoded[j] is None``, its file in ``flac[j]``) is decoded on the device (vv_flac_index / vv_flac_decode) into the same byte
        buffer, behind the uploaded WAV clips: no decoded sample crosses the bus.  So is a G.711 or IMA ADPCM WAVE clip (its WavInfo in
        ``coded[j]``; vv_wav_decode, N25): its size is the host's to know, so it lies between the two, on 16-byte boundaries."""
        import torch
        parts, clips, pos = [], {}, 0
        for j, d in enumerate(decoded):
            if d is None:
                continue
            frames, width, rate = d
            if frames.shape[1] > 2:
                tomono(frames)                    # range check only (OverflowError like the reference); the mix itself runs on the device
            raw = frames.tobytes()
            clips[j] = (pos, width, frames.shape[1], frames.shape[0], rate)
            pad = -len(raw) % 4
            parts.append(raw + b"\0" * pad)
            pos += len(raw) + pad
        coded = coded or {}
        c_offs, base = [], pos                            # the coded clips' places; ``base`` = where FLAC clips may start
        for j in sorted(coded):
            base = -(-base // 16) * 16
            c_offs.append(base)
            base += wav_coded_frame_count(coded[j]) * coded[j].channels * 2
        base = -(-base // 4) * 4

        def alloc(end):
            buf = torch.empty((max(end, 16),), dtype=torch.uint8, device=dev)
            if pos:
                buf[:pos] = torch.frombuffer(bytearray(b"".join(parts)), dtype=torch.uint8).to(dev)
            return buf
        if flac:
            def place(sizes):
                offs, at = [], base
                for n in sizes:
                    offs.append(at)
                    at += n + (-n % 4)
                return alloc(at), offs
            buf, res = self.synth.flac_clips([flac[j] for j in sorted(flac)], pcm_offsets=place)
            for j, r in zip(sorted(flac), res):
                if isinstance(r, Exception):
                    raise r
                off, n, width, rate, ch = r
                if n == 0:
                    raise ValueError("empty audio clip")
                if ch > 2:                        # the same range check, on a copy of this clip alone
                    tomono(buf[off: off + n * ch * width].cpu().numpy().view({1: np.int8, 2: np.int16, 4: np.int32}[width]).reshape(n, ch))
                clips[j] = (off, width, ch, n, rate)
        elif coded:
            buf = alloc(base)
        else:
            buf = torch.frombuffer(bytearray(b"".join(parts)), dtype=torch.uint8).to(dev)
        if coded:
            _pcm, res = self.synth.wav_clips([coded[j] for j in sorted(coded)], pcm_offsets=lambda sizes: (buf, c_offs))
            for j, r in zip(sorted(coded), res):
                if isinstance(r, Exception):
                    raise r
                off, n, width, rate, ch = r
                if n == 0:
                    raise ValueError("empty audio clip")
                if ch > 2:                        # G.711 with more than two channels: the same range check, on a copy of this clip alone
                    tomono(buf[off: off + n * ch * 2].cpu().numpy().view(np.int16).reshape(n, ch))
                clips[j] = (off, width, ch, n, rate)
        desc, out_pos = [], 0
        for j in range(len(decoded)):
            off, width, ch, n, rate = clips[j]
            g = gcd(rate, self.sample_rate)
            n_out = ratecv_len(n, rate, self.sample_rate) if rate != self.sample_rate else n
            desc.append([off, width, ch, n, rate // g, self.sample_rate // g, out_pos, n_out])
            out_pos += n_out
        return self.synth.ingest_pcm(buf, desc, out_pos), [d[7] for d in desc]

    def _ingest_polyphase(self, decoded, dev):
        import torch
        clips = []
        for frames, _w, rate in decoded:
            x = frames.astype(np.float32).mean(axis=1)
            xd = torch.from_numpy(x).to(dev)
            if rate != self.sample_rate:
                if rate not in self._taps:
                    taps, up, down, skip = resample_design(rate, self.sample_rate)
                    self._taps[rate] = (torch.from_numpy(taps).to(dev), up, down, skip)
                taps, up, down, skip = self._taps[rate]
                xd = self.synth.resample_poly(xd, taps, up, down, skip, -(-(x.size * up) // down))
            clips.append(xd)
        return (torch.cat(clips) if len(clips) > 1 else clips[0]), [int(c.numel()) for c in clips]

    def clear(self):
        self._entries.clear()
        self._by_host.clear()
        self.bytes = 0
