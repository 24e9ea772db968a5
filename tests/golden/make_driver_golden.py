"""Generates tests/golden/driver_golden.json: the workspace byte counts and profiling accounts of the stage drivers, recorded on a
GPU from a build of the commit BEFORE the drivers were restructured (one workspace plan per stage, named GEMM arguments).  The
records are ``tests.test_workspace_gpu.driver_records``: vv_transformer_ws_bytes over dtype x plan x lanes x split_k_tail x
lengths, vv_decode_ws_bytes for the tiny HiFi-GAN and Vocos decoders, and launches / flops / bytes per kernel class of preprocess +
2 Euler steps + decode (no times).  Only entry points that commit already has are used.

    python tests/golden/make_driver_golden.py [out.json]
"""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)

from tests.test_workspace_gpu import driver_records, make_engines  # noqa: E402

if __name__ == "__main__":
    out = sys.argv[1] if len(sys.argv) > 1 else os.path.join(HERE, "driver_golden.json")
    engs = make_engines()
    rec = driver_records(engs)
    for e in engs.values():
        e.close()
    with open(out, "w") as f:
        json.dump(rec, f, indent=1, sort_keys=True)
        f.write("\n")
    print("wrote", out, {k: len(v) for k, v in rec.items()})
