"""Generates tests/golden/steps_golden.json: what the acoustic stage driver does for a fixed set of calls, recorded on a GPU from a
build of the commit BEFORE the driver was taken apart (lane plan, per-lane launches, one schedule).  The records are
``tests.test_steps_driver_gpu.steps_records``: the three workspace byte counts per dtype x plan x lanes x batch, launches / flops /
bytes per kernel class and the SHA-256 of x for every call form (no times), and the code and text of every refusal.  Only entries and
wrappers that commit already has are used.  Two runs must write the same file.

    python tests/golden/make_steps_golden.py [out.json]
"""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)

from tests.test_steps_driver_gpu import make_engines, steps_records  # noqa: E402

if __name__ == "__main__":
    out = sys.argv[1] if len(sys.argv) > 1 else os.path.join(HERE, "steps_golden.json")
    engs = make_engines()
    rec = steps_records(engs)
    for e in engs.values():
        e.close()
    with open(out, "w") as f:
        json.dump(rec, f, indent=1, sort_keys=True)
        f.write("\n")
    print("wrote", out, {k: len(v) for k, v in rec.items()})
