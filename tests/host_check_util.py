"""The tools/*_host_check.py as modules: tests/test_host_sanitizers_cpu.py builds and runs them, and the GPU tests take from them the
edge cases they add to a kernel's list, so that the device and the sanitizer builds see the same rows."""
import importlib
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("output", "ingest", "edit", "formant", "denoise", "watermark", "elementwise", "mel", "noise")      # on tools/hip_host_shim.h
OLD = ("flac", "flac_decode", "loudness", "limiter", "prosody")            # on their own stand-ins


def tool(name):
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    try:
        return importlib.import_module(f"{name}_host_check")
    finally:
        sys.path.pop(0)
