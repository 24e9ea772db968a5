"""The recorded trace of the PCM stage (join, output rate, G.711, loudness, limiter, pitch and tempo, FLAC out and in): one small
workload through HipSynth's public methods, and a recorder around the library's entries.  tests/golden/make_pcm_stage_golden.py runs
it on a build of the commit BEFORE the stage's host code moved into pcm_stage.py; tests/test_pcm_stage_gpu.py replays it and compares.
Only names that commit already has are used here."""
import ctypes as C
import hashlib

import numpy as np

SR = 24000
CF = 0.1
PREFIXES = ("vv_join_chunks", "vv_pcm_", "vv_flac_")

# entry -> its row tables: (index of the pointer argument, index of the row count, width, where the recorder reads it)
TABLES = {
    "vv_join_chunks": [(4, 5, 8, "host_i64"), (7, 8, 4, "host_i64")],
    "vv_pcm_resample": [(3, 4, 6, "dev_i64")],
    "vv_pcm_encode": [(3, 4, 3, "dev_i64")],
    "vv_pcm_loudness": [(4, 5, 4, "host_i64"), (8, 5, 2, "dev_f64")],
    "vv_pcm_limit": [(4, 5, 5, "host_i64"), (10, 5, 3, "dev_f64")],
    "vv_pcm_stretch": [(4, 5, 6, "host_i64")],
    "vv_pcm_flac": [(4, 5, 4, "host_i64")],
    "vv_pcm_flac_lpc": [(4, 5, 4, "host_i64")],
    "vv_flac_index": [(4, 5, 8, "host_i64")],
    "vv_flac_decode": [(4, 5, 8, "host_i64"), (7, 5, 6, "host_i64")],
}

# finish_output's option sets, in the order they run; pitch 12 with tempo 2 is a stretch ratio of 1: the conversion reads the joined signal
CASES = [
    ("default", dict()),
    ("8k_ulaw", dict(rate=8000, encoding="ulaw")),
    ("16k_alaw", dict(rate=16000, encoding="alaw")),
    ("loud_scalar", dict(loudness=-23.0)),
    ("loud_list", dict(loudness=[None, -16.0, None, -23.0])),
    ("limit", dict(limiter="true")),
    ("limit_loud", dict(limiter="true", loudness=-16.0)),
    ("limit_list", dict(limiter=[None, "sample", "true", None], loudness=[-23.0, None, -16.0, -16.0])),
    ("pitch", dict(pitch=2)),
    ("tempo", dict(tempo=1.25)),
    ("pitch_eq_tempo", dict(pitch=12, tempo=2.0)),
    ("all", dict(pitch=-3, tempo=0.8, loudness=-20.0, limiter="true", rate=8000)),
    ("flac", dict(encoding="flac")),
    ("flac_lpc", dict(encoding="flac", flac_lpc_order=8, rate=16000)),
]


def workload_pcm():
    """-> (plane int16, plans): an empty request, one of 700 samples (below one FLAC block, loudness block and limiter tile), two chunks
    joining to 9610 (the first whole 400 ms gating block), three joining to 19600 whose middle chunk of 1500 clips the first junction."""
    lens = [[0], [700], [6000, 6010], [11000, 1500, 11000]]
    rng = np.random.default_rng(20240607)
    plans, pos = [], 3
    for req in lens:
        plans.append([])
        for n in req:
            plans[-1].append((pos, n))
            pos += n + 5                                  # odd gaps: no chunk starts on an 8-sample boundary by accident
    return rng.integers(-20000, 20000, pos, dtype=np.int16), plans


def digest(a):
    a = np.ascontiguousarray(a)
    return {"dtype": str(a.dtype), "size": int(a.size), "sha256": hashlib.sha256(a.tobytes()).hexdigest()}


class _DevSpan:
    def __init__(self, ptr, n, typestr):
        self.__cuda_array_interface__ = {"shape": (n,), "typestr": typestr, "data": (ptr, False), "version": 2}


def _dev_read(ptr, n, typestr):
    import torch
    torch.cuda.synchronize()
    return torch.as_tensor(_DevSpan(ptr, n, typestr), device="cuda").cpu().numpy().copy()


class LibRecorder:
    """Wraps every vv_join_chunks / vv_pcm_* / vv_flac_* callable of ``eng.lib``.  events = per call {name, args: the non-pointer
    arguments in order, null: which pointer arguments were null, same: pairs of pointer arguments that were equal, ret (for the entries
    that return a size), tables: keys into ``arrays``}."""

    def __init__(self, eng, exports, events=None):
        self.eng, self.events, self.arrays, self._real = eng, [] if events is None else events, {}, {}
        for name, (res, argtypes) in exports.items():
            if name.startswith(PREFIXES):
                self._real[name] = getattr(eng.lib, name)
                setattr(eng.lib, name, self._wrap(name, self._real[name], res, argtypes))

    def close(self):
        for name, fn in self._real.items():
            setattr(self.eng.lib, name, fn)

    def _wrap(self, name, real, res, argtypes):
        def call(*a):
            ret = real(*a)
            vals = [(v.value if hasattr(v, "value") else v) or 0 for v in a]
            ptr = [i for i, t in enumerate(argtypes) if t is C.c_void_p]
            ev = {"name": name, "args": [vals[i] for i in range(len(vals)) if i not in ptr]}
            if res is C.c_int and ptr:                    # an entry with a context: ctx first, the stream last
                assert ret == 0, (name, ret)
                ptr = ptr[1:-1]
                ev["null"] = [i for i in ptr if not vals[i]]
                ev["same"] = [[i, j] for i in ptr for j in ptr if i < j and vals[i] and vals[i] == vals[j]]
                ev["tables"] = []
                for k, (pi, ci, width, kind) in enumerate(TABLES[name]):
                    n = int(vals[ci]) * width
                    if kind == "host_i64":
                        t = np.ctypeslib.as_array((C.c_int64 * n).from_address(vals[pi])).copy()
                    else:
                        t = _dev_read(vals[pi], n, "<i8" if kind == "dev_i64" else "<f8")
                    key = f"ev{len(self.events)}_t{k}"
                    self.arrays[key] = t.reshape(-1, width)
                    ev["tables"].append(key)
            else:
                ev["ret"] = int(ret)
            self.events.append(ev)
            return ret
        return call


def run_workload(eng, exports, events=None):
    """The whole workload on ``eng`` (a HipSynth of the tiny model) -> {"events", "marks", "arrays", "results", "prof"}; events = the
    list to append the calls to."""
    import torch
    from vietvoice_tts_amd.core.audio_processor import flac_container
    plane_h, plans = workload_pcm()
    plane = torch.from_numpy(plane_h).to(eng.device)
    rec = LibRecorder(eng, exports, events)
    results, marks = {}, {}
    eng.prof_enable(True)
    eng.prof_collect()
    try:
        files = {}
        for name, kw in CASES:
            marks[name] = len(rec.events)
            outs = eng.finish_output(plane, plans, CF, SR, **kw)
            assert len(outs) == len(plans)
            results[name] = [digest(o) for o in outs]
            if kw.get("encoding") == "flac":
                files[name] = [np.asarray(o).tobytes() for o in outs]
        marks["flac_clips"] = len(rec.events)
        bad = bytearray(files["flac"][3])
        bad[flac_container(bytes(bad)).start + 5] ^= 0xFF          # the CRC-8 that closes the first frame's header
        pcm, out = eng.flac_clips([files["flac"][1], bytes(bad), files["flac_lpc"][2], files["flac"][2]])
        host = pcm.cpu().numpy()                                   # the clips' own bytes: the padding between them is never written
        results["flac_clips"] = [list(o) + [digest(host[o[0]: o[0] + o[1] * o[2] * o[4]])] if isinstance(o, tuple) else repr(o) for o in out]
        marks["streams"] = len(rec.events)
        resample, encode = eng.output_stream_backends(SR, 8000, "ulaw")
        y = resample(plane_h[:2400], 0, 0, 800)
        _none, flac = eng.output_stream_backends(SR, None, "flac")
        limit = eng.limiter_stream_backend(SR)
        results["streams"] = {"resample": digest(y), "encode": digest(encode(y)), "flac": digest(flac(plane_h[100: 100 + 4096], 0, False)),
                              "limit": digest(limit(plane_h[:2000], 240, 1000))}
        torch.cuda.synchronize()
        prof = eng.prof_collect()["elementwise"]
    finally:
        eng.prof_enable(False)
        rec.close()
    return {"events": rec.events, "marks": marks, "arrays": rec.arrays, "results": results,
            "prof": {k: prof[k] for k in ("launches", "flops", "bytes")}}
