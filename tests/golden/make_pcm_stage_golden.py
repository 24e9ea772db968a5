"""Generates tests/golden/pcm_stage_golden.{json,npz}: the recorded trace of the PCM stage (tests/pcm_stage_util.py), made on a GPU
from a build of the commit BEFORE the stage's host code moved out of HipSynth into pcm_stage.py.  Per library call: the entry, every
non-pointer argument, the row tables; per case the digests of the result bytes; the ELEMWISE profiling account of the whole run.
Next to them ``inputs``: the host values every HipSynth wrapper was called with (rows, lengths, options; a tensor becomes its length),
in call order with the index of the first library call it made, which tests/test_pcm_stage_cpu.py feeds to the pure plans.
Only methods and entry points that commit already has are used.

    python tests/golden/make_pcm_stage_golden.py [out_dir]
"""
import inspect
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)

from tests import pcm_stage_util as U  # noqa: E402

METHODS = ("join_chunks", "pcm_resample", "pcm_encode", "pcm_loudness", "pcm_limit", "pcm_stretch", "pcm_flac", "flac_index", "flac_decode",
           "_prosody", "finish_output")


def _host(v, x_ptr):
    import torch
    if isinstance(v, torch.Tensor):
        return {"tensor": int(v.numel()), "is_x": v.data_ptr() == x_ptr}
    if isinstance(v, (list, tuple)):
        return [_host(e, x_ptr) for e in v]
    if isinstance(v, (np.integer, np.floating)):
        return v.item()
    return v


def record_inputs(eng, events):
    """Wrap the HipSynth methods on the instance: -> the list the calls append {name, at, args} to."""
    import torch
    inputs = []
    for name in METHODS:
        real = getattr(eng, name)
        sig = inspect.signature(real)

        def call(*a, _name=name, _real=real, _sig=sig, **kw):
            b = _sig.bind(*a, **kw)
            b.apply_defaults()
            first = next(iter(b.arguments.values()))
            x_ptr = first.data_ptr() if isinstance(first, torch.Tensor) else 0
            args = {k: _host(v, x_ptr) for k, v in b.arguments.items()}
            if _name == "flac_decode":                     # index = (ws, rows_h, rows_d): the clips' rows are what the plan reads
                args["index"] = b.arguments["index"][1].tolist()
            inputs.append({"name": _name, "at": len(events), "args": args})
            return _real(*a, **kw)
        setattr(eng, name, call)
    return inputs


if __name__ == "__main__":
    from vietvoice_tts_amd.model_spec import ModelSpec, make_synthetic_weights
    from vietvoice_tts_amd.runtime import EXPORTS, HipSynth
    out = sys.argv[1] if len(sys.argv) > 1 else HERE
    spec = ModelSpec.tiny()
    eng = HipSynth(spec, make_synthetic_weights(spec, seed=9527), acoustic_dtype="fp32", nfe_step=8)
    events = []
    inputs = record_inputs(eng, events)
    rec = U.run_workload(eng, EXPORTS, events)
    eng.close()
    arrays = rec.pop("arrays")
    rec["inputs"] = inputs
    with open(os.path.join(out, "pcm_stage_golden.json"), "w") as f:
        json.dump(rec, f, indent=None, sort_keys=True, separators=(",", ":"))
        f.write("\n")
    np.savez_compressed(os.path.join(out, "pcm_stage_golden.npz"), **arrays)
    print("wrote", out, len(rec["events"]), "calls,", len(inputs), "wrapper calls,", len(arrays), "tables, prof", rec["prof"])
