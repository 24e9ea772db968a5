"""Writes request_options_golden.json: what the output stage is handed for a request's options, and how a full stream chain cuts
its blocks -- recorded BEFORE the request-options refactor so that the refactor can be held against it.

The JSON in the tree was written by this script on commit 537bc8a ("Add Adams-Bashforth multistep solvers (ab2, ab3) and a step
report (N20)"), where ``TTSEngine._finish_device`` still took the ten per-option keywords.  ``finish_device`` below is the adapter: it
drives ``_finish_device`` through those keywords there (exactly as ``BatchingFrontend._finish`` spelled the call: loudness, limiter,
pitch and tempo always as lists, formants and denoise only when some request had one) and through ``options`` afterwards.
tests/test_request_options_cpu.py imports the cases and the recorder from here and compares for equality.

Nothing here needs a GPU: ``engine.finish_output`` is replaced by a recorder that notes, for the arguments it was handed, what the
stage would do with them: pcm_stage.plan_finish and plan_finish_denoise, the formants as finish_output reads them (a list, None
entries = "shift"; only looked at when a pitch is present), denoise_bias (only looked at when a strength is present; kept as a hash), and rate,
encoding, peak_dbfs and flac_lpc_order.

    python tests/golden/make_request_options_golden.py        # rewrites the JSON next to it
"""
import dataclasses
import inspect
import json
import os
import sys
import tempfile
import types

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

OUT = os.path.join(HERE, "request_options_golden.json")
FIELDS = ("cfg_strength", "cfg_interval", "apg_eta", "apg_norm", "loudness", "limiter", "pitch", "tempo", "formants", "denoise")
BIAS = [float((7 * k) % 13) for k in range(513)]

# the engine's side: no output option; every one; loudness + limiter + FLAC with LPC subframes
CONFIGS = {
    "unset": {},
    "all_set": dict(output_loudness=-20.0, output_limiter="true", output_pitch=2.0, output_tempo=1.25, output_formants="keep",
                    output_denoise=1.5, output_denoise_bias=BIAS, output_sample_rate=16000, output_encoding="ulaw", output_peak_dbfs=-2.0),
    "loud_lim_flac_lpc": dict(output_loudness=-23.0, output_limiter="sample", output_encoding="flac", flac_lpc_order=8),
}

# the requests' side: per batch the requests' (chunks, own options); None = synthesize()'s call, which names no options at all
BATCHES = {
    "engine_call": None,
    "one_plain": [(2, {})],
    "three_plain": [(1, {}), (3, {}), (2, {})],
    "own_loudness": [(2, dict(loudness=-18.0)), (1, {})],
    "own_limiter": [(1, {}), (2, dict(limiter="sample"))],
    "own_pitch": [(1, dict(pitch=-3.0)), (1, {}), (2, {})],
    "own_tempo": [(3, dict(tempo=0.8))],
    "own_formants_alone": [(1, dict(formants="keep")), (1, {})],
    "own_formants_with_pitch": [(2, dict(pitch=1.0, formants="keep")), (1, dict(pitch=2.0, formants="shift"))],
    "own_denoise": [(1, dict(denoise=2.0)), (2, {})],
    "acoustic_only": [(2, dict(cfg_strength=1.5, cfg_interval=(0.1, 0.9), apg_eta=0.5, apg_norm=2.0)), (1, {})],
    "loudness_and_limiter_groups": [(1, dict(loudness=-30.0, limiter="true")), (2, dict(limiter="sample")), (1, dict(loudness=-16.0)), (1, {})],
    "everything_mixed": [(2, dict(loudness=-14.0, pitch=-5.0, denoise=0.5, cfg_strength=2.5)),
                         (1, dict(tempo=1.5, formants="keep", limiter="true")),
                         (3, {}),
                         (1, dict(pitch=4.0, tempo=0.75, formants="shift", denoise=8.0, loudness=-27.0, limiter="sample", apg_eta=0.0))],
}

STREAM_CONFIG = dict(output_limiter="true", output_sample_rate=8000, output_encoding="flac")
STREAM_TEXT = "Hôm nay trời đẹp quá, chúng ta cùng nhau đi dạo quanh hồ nhé. " * 3


def make_engine(model_dir, **config):
    """A TTSEngine on oracle sessions (tiny spec): no GPU, no library."""
    from oracle.vv_oracle import Oracle, OracleSession
    from vietvoice_tts_amd.core import ModelConfig, TTSEngine

    def factory(spec, weights, cfg):
        orc = Oracle(spec, weights, nfe_step=cfg.nfe_step)
        return {k: OracleSession(orc, k, seed=cfg.random_seed) for k in ("preprocess", "transformer", "decode")}
    return TTSEngine(ModelConfig(model_cache_dir=str(model_dir), synthetic_model=True, model_spec="tiny", nfe_step=3, max_chunk_duration=8.0,
                                 **config), session_factory=factory)


def bias_digest(bias) -> str:
    """A bias profile as the file holds it: the number of values and a hash of them as float64."""
    import hashlib
    import struct
    vals = [float(v) for v in bias]
    return f"{len(vals)}:{hashlib.sha256(struct.pack(f'<{len(vals)}d', *vals)).hexdigest()}"


def _record(pcm, plans, cross_fade_duration, sample_rate, rate=None, encoding="pcm16", loudness=None, peak_dbfs=-1.0, limiter=None, pitch=None,
            tempo=None, flac_lpc_order=0, formants=None, denoise=None, denoise_bias=None):
    """finish_output's signature; -> what it would do, as plain JSON values."""
    from vietvoice_tts_amd.core.audio_processor import check_formants
    from vietvoice_tts_amd.pcm_stage import _per_request, plan_finish, plan_finish_denoise
    R = len(plans)
    den = plan_finish_denoise(R, denoise)
    pit, tem, groups = plan_finish(R, loudness, limiter, pitch, tempo)
    keep = None
    if pit is not None:
        keep = ["shift"] * R if formants is None else [check_formants(f) for f in _per_request("finish_output", formants, R, "formants")]
    return {"plans": [[list(s) for s in p] for p in plans], "cross_fade_duration": cross_fade_duration, "sample_rate": sample_rate,
            "rate": rate, "encoding": encoding, "peak_dbfs": peak_dbfs, "flac_lpc_order": flac_lpc_order,
            "denoise": den, "denoise_bias": None if den is None or denoise_bias is None else bias_digest(denoise_bias),
            "pitch": pit, "tempo": tem, "groups": [[mode, list(sel), list(tg)] for mode, sel, tg in groups], "formants": keep}


def finish_device(eng, dev_pcm, counts, own):
    """``eng._finish_device`` for requests with the option dicts ``own`` (None = no options named), on either side of the refactor."""
    if own is None:
        return eng._finish_device(dev_pcm, counts)
    if "options" in inspect.signature(eng._finish_device).parameters:
        from vietvoice_tts_amd.request_options import RequestOptions
        return eng._finish_device(dev_pcm, counts, options=[RequestOptions.checked(**o) for o in own])
    col = lambda k: [o.get(k) for o in own]  # noqa: E731
    return eng._finish_device(dev_pcm, counts, loudness=col("loudness"), limiter=col("limiter"), pitch=col("pitch"), tempo=col("tempo"),
                              **({} if all(v is None for v in col("formants")) else {"formants": col("formants")}),
                              **({} if all(v is None for v in col("denoise")) else {"denoise": col("denoise")}))


def record_handover(eng):
    """{config: {batch: record}} with ``eng``'s config replaced by each of CONFIGS in turn and finish_output by the recorder."""
    m, base, out = eng.model_session_manager, eng.config, {}
    seen = []
    m.engine = types.SimpleNamespace(finish_output=lambda *a, **k: seen.append(_record(*a, **k)) or [None] * len(a[1]))
    try:
        for cname, over in CONFIGS.items():
            eng.config = dataclasses.replace(base, **over)
            out[cname] = {}
            for bname, reqs in BATCHES.items():
                counts = [2] if reqs is None else [n for n, _o in reqs]
                spans = [(1000 * i, 900 + i) for i in range(sum(counts))]
                del seen[:]
                finish_device(eng, (None, spans), counts, None if reqs is None else [o for _n, o in reqs])
                assert len(seen) == 1, "one finish_output call per batch"
                out[cname][bname] = seen[0]
    finally:
        m.engine, eng.config = None, base
    return json.loads(json.dumps(out))          # tuples -> lists, as the file holds them


def stream_run(eng):
    """-> (the streamed blocks, synthesize()'s bytes) of STREAM_TEXT from equal noise streams; eng = make_engine(.., **STREAM_CONFIG)."""
    import torch

    def reseed():
        for sess in eng.model_session_manager.sessions.values():
            sess.gen = torch.Generator().manual_seed(123)
    reseed()
    whole = eng.synthesize(STREAM_TEXT)[0]
    reseed()
    return list(eng.synthesize_stream(STREAM_TEXT)), whole


def main():
    with tempfile.TemporaryDirectory() as d:
        eng = make_engine(d)
        try:
            gold = {"handover": record_handover(eng)}
        finally:
            eng.cleanup()
        eng = make_engine(d, **STREAM_CONFIG)
        try:
            blocks, _whole = stream_run(eng)
            gold["stream"] = {"chunks": len(eng._last_plan), "block_sizes": [int(b.size) for b in blocks]}
        finally:
            eng.cleanup()
    with open(OUT, "w", encoding="utf-8") as f:
        json.dump(gold, f, indent=1, sort_keys=True)
        f.write("\n")
    print("wrote", OUT, gold["stream"])


if __name__ == "__main__":
    main()
