"""-m gpu: the recorded trace of the PCM stage.  tests/golden/pcm_stage_golden.{json,npz} were recorded on a build of the commit before
the stage's host code moved into pcm_stage.py and the N10 ... N17 entries of csrc/vv_api.hip took their shared checks
(tests/golden/make_pcm_stage_golden.py).  The same workload (tests/pcm_stage_util.py) is replayed here and must give the same library
calls in the same order with the same arguments and row tables, the same result bytes and the same profiling account: equality, no
tolerance.  The results are compared through their SHA-256 (four requests times fourteen option sets of noise do not fit a fixture)."""
import json
import os

import numpy as np
import pytest

from tests import pcm_stage_util as U

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "pcm_stage_golden")


@pytest.fixture(scope="module")
def golden():
    with open(GOLDEN + ".json") as f:
        rec = json.load(f)
    with np.load(GOLDEN + ".npz") as z:
        rec["arrays"] = {k: z[k] for k in z.files}
    return rec


@pytest.fixture(scope="module")
def replay(tiny_setup):
    """On an engine of its own, as the recording was: the constant tables an engine caches (fade tables, limiter tile) are part of the trace."""
    from vietvoice_tts_amd.runtime import EXPORTS, HipSynth
    spec, w, _ = tiny_setup
    eng = HipSynth(spec, w, acoustic_dtype="fp32", nfe_step=8)
    rec = U.run_workload(eng, EXPORTS)
    eng.close()
    arrays = rec.pop("arrays")
    rec = json.loads(json.dumps(rec))                         # tuples as the file has them
    rec["arrays"] = arrays
    return rec


SECTIONS = [name for name, _kw in U.CASES] + ["flac_clips", "streams"]


@pytest.mark.parametrize("section", SECTIONS)
def test_calls_arguments_tables_and_results(golden, replay, section):
    order = sorted(golden["marks"], key=golden["marks"].get)
    assert golden["marks"] == replay["marks"] and set(order) == set(SECTIONS)
    lo = golden["marks"][section]
    hi = ([golden["marks"][s] for s in order if golden["marks"][s] > lo] + [len(golden["events"])])[0]
    assert hi > lo and len(replay["events"]) == len(golden["events"])
    for k in range(lo, hi):
        want, got = golden["events"][k], replay["events"][k]
        assert got["name"] == want["name"], k
        assert got["args"] == want["args"], (k, want["name"])
        assert got.get("ret") == want.get("ret") and got.get("null") == want.get("null") and got.get("same") == want.get("same"), (k, want["name"])
        assert got.get("tables") == want.get("tables"), (k, want["name"])
        for key in want.get("tables", []):
            a, b = golden["arrays"][key], replay["arrays"][key]
            assert a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes(), (k, want["name"], key)
    assert replay["results"][section] == golden["results"][section]


def test_the_trace_covers_every_entry_and_the_profiling_account(golden, replay):
    names = {e["name"] for e in golden["events"]}
    assert set(U.TABLES) <= names and len(golden["arrays"]) == sum(len(e.get("tables", [])) for e in golden["events"])
    assert replay["prof"] == golden["prof"] and golden["prof"]["launches"] == sum(e["name"] in U.TABLES for e in golden["events"])
