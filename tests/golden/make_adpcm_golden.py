"""Generates tests/golden/adpcm_golden.npz: what CPython's stdlib ``audioop`` says about the inputs of tests/adpcm_util.py,
so that tests/test_adpcm_cpu.py can hold the mirror against it where audioop no longer exists (it left the stdlib in 3.13).

    python tests/golden/make_adpcm_golden.py

Stored:
  ulaw2lin, alaw2lin       audioop.ulaw2lin / alaw2lin at width 2 for the codes 0 ... 255
  enc_<spb>_<name>_{best, err, carried}   per block: the step index of the exhaustive search (89 x lin2adpcm + adpcm2lin, the first
                           smallest error over the block's real samples), that error, and the error of the carried-state encoder
  enc_<spb>_<name>_sha1    the SHA-1 of the blocks' bytes (header + nibble-swapped lin2adpcm codes of the winner)
  dec_<name>_sha1          the SHA-1 of the int16 frames audioop.adpcm2lin gives per block and channel for the decoder files
  check                    lin2adpcm of (1000, -1000, 3000, 0) from state (0, 20): 7f 7a
Digests instead of bytes keep the file at a few KB; byte equality is what they pin all the same."""
import hashlib
import os
import sys

import numpy as np

import audioop

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from tests import adpcm_util as U  # noqa: E402


def digest(b):
    return np.frombuffer(hashlib.sha1(bytes(b)).digest(), np.uint8)


def main():
    codes = bytes(range(256))
    out = {"ulaw2lin": np.frombuffer(audioop.ulaw2lin(codes, 2), np.int16), "alaw2lin": np.frombuffer(audioop.alaw2lin(codes, 2), np.int16),
           "check": np.frombuffer(audioop.lin2adpcm(np.array([1000, -1000, 3000, 0], np.int16).tobytes(), 2, (0, 20))[0], np.uint8)}
    for spb in U.SPBS:
        for name, x in U.encoder_inputs(spb):
            best, err, carried, data = U.audioop_encoder_record(audioop, x, spb)
            out[f"enc_{spb}_{name}_best"], out[f"enc_{spb}_{name}_err"], out[f"enc_{spb}_{name}_carried"] = best.astype(np.uint8), err, carried
            out[f"enc_{spb}_{name}_sha1"] = digest(data)
    for name, data, want, _rate in U.decoder_files():
        if isinstance(want, tuple):
            continue
        w = U.parse_wav(data)
        frames = U.audioop_adpcm_frames(audioop, w["payload"], w["channels"], w["block_align"], w["fact"])
        assert np.array_equal(frames, want), name                # the plain-Python reference of the tests says the same
        out[f"dec_{name}_sha1"] = digest(frames.astype("<i2").tobytes())
    np.savez_compressed(U.GOLDEN, **out)
    print(U.GOLDEN, os.path.getsize(U.GOLDEN), "bytes,", len(out), "entries")


if __name__ == "__main__":
    main()
