#!/usr/bin/env python3
"""mel_kernel of csrc/vv_mel.hip on the CPU under sanitizers (K1), against the float64 reference of tests/gpu_util.py.

Builds tools/mel_host_check.cpp (the kernel source on tools/hip_host_shim.h, exact-size heap buffers) twice, with
-fsanitize=address,undefined and with -fsanitize=thread, and runs
  a small transform (the kernel takes n_fft, hop and n_mel as arguments): n_fft 16, hop 4, n_mel 5, the window, twiddles and
    filterbank made as pack.py makes the constants; two clips per launch with audio_len of (0, 1), (n_fft / 2, n_fft / 2 + 1),
    (5 hop - 1, 5 hop), (5 hop + 1, 13), and ld_audio + 5 in the first and in the last item (the kernel clamps a device length to the
    row: the reference is that of the clip clamped to ld_audio); in every launch the longer clip has audio_len == ld_audio;
  two frames at the model's 1024 / 256 / 100 (audio_len 256 beside an empty clip).
  audio is one exact block of B x ld_audio samples, ld_audio = the longer clip; 32767 behind every audio_len.  mel is one exact block of
  B x F_max x n_mel floats filled with 0xAA, F_max two more than the longer clip's frames: the kernel owns every element (frames behind
  a clip are zeros), so none may keep the fill.  The dynamic LDS is an exact block of (3 n_fft + n_fft / 2 + 1) floats.
  grid: restated from vvk_mel (csrc/vv_mel.hip: `dim3 grid(F_max, B)`, 256 threads, `lds = (3 * n_fft + n_fft / 2 + 1) * sizeof(float)`).
  compared with gpu_util.mel_ref_counted: parity_err <= mel_c(spec) x 2^-24, the device test's count without its yardstick term, and
  exact zeros behind every clip.  logf and sqrtf are the host libm's.
The full and the reduced list are the same: every case is an edge and the whole takes seconds.  Needs no GPU.

    python tools/mel_host_check.py [--cxx clang++] [--keep DIR] [--san asan|tsan|both] [--reduced]"""
import math
import os
import sys
import types

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import host_check_common as H  # noqa: E402
import numpy as np  # noqa: E402

NAME = "mel"
SMALL = types.SimpleNamespace(n_fft=16, win_length=16, hop_length=4, n_mel=5, sample_rate=24000)
MODEL = types.SimpleNamespace(n_fft=1024, win_length=1024, hop_length=256, n_mel=100, sample_rate=24000)
F_EXTRA = 2
OVER = 5                            # a device length this much beyond ld_audio


def find_cxx():
    return H.find_cxx()


def build(cxx, work, san="asan"):
    return H.build(NAME, cxx, work, san)


def _gu():
    if H.ROOT not in sys.path:
        sys.path.insert(0, H.ROOT)
    from tests import gpu_util as gu
    return gu


def case_list():
    """-> [(spec, MelCase with the lengths the reference uses, the audio_len the kernel is given)]"""
    gu = _gu()
    h, half = SMALL.hop_length, SMALL.n_fft // 2
    cs = [(SMALL, c, c.lens) for c in gu.mel_short_cases(SMALL)]
    cs += [(SMALL, gu.MelCase("mel/host/k_hop_minus1_k_hop", (5 * h - 1, 5 * h), seed=10), (5 * h - 1, 5 * h)),
           (SMALL, gu.MelCase("mel/host/k_hop_plus1", (5 * h + 1, 13), seed=11), (5 * h + 1, 13)),
           (SMALL, gu.MelCase("mel/host/over_first", (5 * h + 1, 13), seed=12), (5 * h + 1 + OVER, 13)),
           (SMALL, gu.MelCase("mel/host/over_last", (13, 5 * h + 1), seed=13), (13, 5 * h + 1 + OVER)),
           (MODEL, gu.MelCase("mel/host/model_two_frames", (256, 0), seed=14), (256, 0))]
    return cs


def tables(spec):
    import torch
    gu = _gu()
    window, fb = gu.mel_tables(spec)
    ang = 2.0 * math.pi * torch.arange(spec.n_fft, dtype=torch.float64) / spec.n_fft          # pack.py: const.tw_cos, const.tw_sin
    return window.numpy(), ang.cos().float().numpy(), ang.sin().float().numpy(), fb.numpy()


def cases(exe, work, reduced=False):
    """Runs every case through exe; yields (label, inside the bound of the float64 reference)."""
    import torch
    gu = _gu()
    bt, meta = H.Batch(exe, work, NAME), []
    for spec, case, audio_len in case_list():
        o = case.ops()
        ld = max(case.lens)
        F_ref = ld // spec.hop_length + 1
        F_max = F_ref + F_EXTRA
        window, tc, ts, fb = tables(spec)
        lds = (3 * spec.n_fft + spec.n_fft // 2 + 1) * 4
        bt.add("mel", (F_max, 2), 256, [o.audio.numpy(), ld, np.array(audio_len, np.int32), window, tc, ts, fb,
                                       H.filled((2, F_max, spec.n_mel), np.float32), F_max, spec.n_fft, spec.hop_length, spec.n_mel], shmem=lds)
        meta.append((spec, case, o, F_ref))
    for (spec, case, o, F_ref), out in zip(meta, bt.run()):
        got = torch.from_numpy(out[7].copy())
        r = gu.mel_ref_counted(case, spec, o)
        err, where = gu.parity_err(got[:, :F_ref], r.ref, r.A, r.allow)
        yield H.check(f"{case.name} n_fft {spec.n_fft} (err / bound {err / r.bound:.3f})",
                      err <= r.bound and bool((got[:, F_ref:].view(torch.int32) == 0).all()))


if __name__ == "__main__":
    H.main(NAME, cases, __doc__)
