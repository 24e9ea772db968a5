"""N18 on the host (no GPU): the mirror of the formant-preserving pitch shift (core/audio_processor.py: formant_filters, keep_formants,
shift_prosody(.., formants="keep")) and its plumbing.  What the correction means is measured on a synthetic vowel with an envelope
estimate of the tests' own (tests/formant_util.py); the device is held to this mirror bit for bit in tests/test_formant_gpu.py."""
import ctypes
import hashlib
import json
import os
import re

import numpy as np
import pytest

from tests import formant_util as fu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _ap():
    from vietvoice_tts_amd.core import audio_processor
    return audio_processor


# ------------------------------------------------------------------ the feature means something
@pytest.fixture(scope="module")
def vowel():
    """The source vowel, where its resonances are measured, and per case (ratio, keep, shift)."""
    ap = _ap()
    src = fu.vowel()
    freqs, env = fu.envelope(src, fu.F0)
    at = {f: fu.peak_in(freqs, env, f / 1.15, f * 1.15) for f, _bw in fu.RESONANCES}
    out = {}
    for pitch, tempo in fu.MEANING_CASES:
        plan = ap.prosody_plan(src.size, pitch, tempo)
        out[(pitch, tempo)] = (plan.p_r / plan.q_r, ap.shift_prosody(src, pitch, tempo, formants="keep"), ap.shift_prosody(src, pitch, tempo))
    return src, at, out


@pytest.mark.parametrize("case", fu.MEANING_CASES)
def test_resonances_stay_and_the_fundamental_moves(vowel, case):
    src, at, out = vowel
    ratio, keep, shift = out[case]
    assert keep.dtype == np.int16 and keep.size == shift.size
    assert all(abs(at[f] / f - 1.0) < 0.02 for f in at)                               # the yardstick finds the source's own resonances
    for f in (500.0, 1500.0, 2500.0):
        got_keep, got_shift = (fu.resonance(sig, ratio * fu.F0, at[f], ratio) for sig in (keep, shift))
        print(f"case {case}: resonance {f:.0f} Hz (measured {at[f]:.0f}) -> keep {got_keep:.0f} Hz, shift {got_shift:.0f} Hz, "
              f"shifted position {at[f] * ratio:.0f} Hz")
        if f == 500.0:
            continue                                  # reported only: the harmonic spacing is as large as the shift
        assert fu.closer_in_log(got_keep, at[f], at[f] * ratio), (case, f, got_keep)             # A
        assert not fu.closer_in_log(got_shift, at[f], at[f] * ratio), (case, f, got_shift)       # C: the measurement sees the difference
    f0 = fu.fundamental(keep)
    print(f"case {case}: fundamental {f0:.2f} Hz, the shift asks for {ratio * fu.F0:.2f} Hz")
    assert fu.closer_in_log(f0, ratio * fu.F0, fu.F0), (case, f0)                                # B


@pytest.mark.parametrize("case", fu.MEANING_CASES)
def test_level_stays_within_a_factor_of_two(vowel, case):
    _src, _at, out = vowel
    _ratio, keep, shift = out[case]
    assert 0.5 < fu.rms(keep) / fu.rms(shift) < 2.0


# ------------------------------------------------------------------ flat input, the tables, the hand-worked frame
@pytest.mark.parametrize("kind,n", [("zeros", 1500), ("constant", 1500), ("zeros", 1), ("constant", 257)])
def test_flat_input_passes_through_unit_filters(kind, n):
    ap = _ap()
    x = fu.signal(kind, n)
    y = ap.shift_prosody(x, 4, 1.25)
    tn, td = ap.prosody_tempo(ap.prosody_plan(n, 4, 1.25))
    h, flat = ap.formant_filters(x, y, tn, td)
    assert h.shape == (-(-y.size // fu.H) + 1, fu.L) and h.dtype == np.float64
    if kind == "zeros":
        assert flat.all() and (h[:, 0] == 1.0).all() and not h[:, 1:].any()
    unit = np.zeros_like(h)
    unit[:, 0] = 1.0
    assert np.array_equal(h[flat], unit[flat])
    assert np.array_equal(ap.apply_formant_filters(y, unit), y)                       # through unit filters: sample for sample
    if kind == "zeros":
        assert np.array_equal(ap.keep_formants(x, y, tn, td), y)
    assert ap.keep_formants(np.zeros(0, np.int16), np.zeros(0, np.int16)).size == 0


def test_a_constant_is_flat_away_from_its_edges():
    """Inside a constant the first difference is zero: R[0] = 0, the frame is flat and z == y there; the frames that see the signal's
    start or end are live (an edge is a step)."""
    ap = _ap()
    x = fu.signal("constant", 5000)
    h, flat = ap.formant_filters(x, x)
    assert flat[3:-3].all() and not flat[0] and not flat[-1]
    z = ap.keep_formants(x, x)
    assert np.array_equal(z[3 * fu.H: -3 * fu.H], x[3 * fu.H: -3 * fu.H])


def test_tables_and_constants_match_the_header():
    ap = _ap()
    wa, g = ap.formant_tables()
    assert wa.shape == (ap.FORMANT_NA,) and g.shape == (ap.FORMANT_P + 1,) and wa.dtype == g.dtype == np.float64
    assert wa[0] == 0.0 and wa[ap.FORMANT_NA // 2] == 1.0 and g[0] == 1.0 and g[1] == ap.FORMANT_GAMMA and g[2] == g[1] * g[1]
    assert ap.FORMANT_H == ap.WSOLA_HS == fu.H and (ap.FORMANT_P, ap.FORMANT_NA, ap.FORMANT_L) == (fu.P, fu.NA, fu.L)
    hdr = open(os.path.join(ROOT, "include", "vvtts.h")).read()
    for name, v in (("P", ap.FORMANT_P), ("NA", ap.FORMANT_NA), ("H", ap.FORMANT_H), ("L", ap.FORMANT_L)):
        assert int(re.search(rf"#define VV_FORMANT_{name} (\d+)", hdr).group(1)) == v
    assert ap.FORMANT_GAMMA ** ap.FORMANT_L < 1e-4                                    # what the cut at L taps leaves out


def test_one_frame_of_a_two_pole_signal_against_lfilter():
    """h_m = gain * lfilter(A_y, A_x, impulse), from the function's own A.
    The tolerance: step t of the recursion computes r[t] = A_y[t] - sum_k A_x[k] r[t - k] in at most 2 P + 1 rounded operations, so it
    leaves a local error |d[t]| <= (2 P + 1) u S, u = 2^-53, S = max_t (|A_y[t]| + sum_k |A_x[k]| |r[t - k]|).  The local errors run
    through the same recursion, whose impulse response is g = 1 / A_x: |error of r[t]| <= ||g||_1 (2 P + 1) u S.  lfilter's own
    (transposed) form has a bound of the same size, and the product by gain adds one rounding: 2 gain ||g||_1 (2 P + 2) u S in all."""
    from scipy.signal import lfilter
    ap = _ap()
    rng = np.random.default_rng(5)

    def two_pole(fc, r, n=fu.H):
        e = rng.standard_normal(n + 2000)
        return np.rint(3000.0 * lfilter([1.0], [1.0, -2.0 * r * np.cos(2 * np.pi * fc / fu.SR), r * r], e)[2000:] / 10.0).astype(np.int16)

    x, y = two_pole(1500.0, 0.97), two_pole(1900.0, 0.97)
    h, flat, (Ay, Ax, ey, ex) = ap.formant_filters(x, y, parts=True)
    assert h.shape == (2, fu.L) and not flat.any()
    imp = np.zeros(fu.L)
    imp[0] = 1.0
    for m in range(2):
        assert Ay[m, 0] == Ax[m, 0] == 1.0 and ey[m] > 0 and ex[m] > 0
        gain = np.sqrt(ex[m] / ey[m])
        want = gain * lfilter(Ay[m], Ax[m], imp)
        g1 = np.abs(lfilter([1.0], Ax[m], imp)).sum()
        r = h[m] / gain
        S = (np.convolve(np.abs(Ax[m]), np.abs(r))[: fu.L] + np.concatenate([np.abs(Ay[m]), np.zeros(fu.L - fu.P - 1)])).max()
        tol = 2.0 * gain * g1 * (2 * fu.P + 2) * 2.0 ** -53 * S
        err = np.abs(h[m] - want).max()
        print(f"frame {m}: max |h - lfilter| = {err:.3e}, bound {tol:.3e}, gain {gain:.4f}, |h|_max {np.abs(h[m]).max():.4f}")
        assert err <= tol and tol < 1e-9
        assert np.abs(h[m][-64:]).max() < 1e-3 * np.abs(h[m]).max()                   # the response has died away at the cut


def test_keep_formants_checks_its_lengths():
    ap = _ap()
    x = fu.speechy(1000, 1)
    with pytest.raises(ValueError, match="keep_formants"):
        ap.keep_formants(x, x[:999])
    with pytest.raises(ValueError, match="keep_formants"):
        ap.keep_formants(x, x, 0, 1)
    with pytest.raises(ValueError, match="keep_formants"):
        ap.keep_formants(x, x[:800], 5, 4.5)
    assert ap.keep_formants(x, np.resize(x, 800), 5, 4).size == 800                   # tempo 1.25: 1000 -> 800 samples


def test_tempo_alone_and_no_prosody_run_nothing_new(monkeypatch):
    ap = _ap()
    monkeypatch.setattr(ap, "keep_formants", lambda *a, **k: pytest.fail("keep_formants was called"))
    x = fu.speechy(3000, 2)
    assert np.array_equal(ap.shift_prosody(x, None, 1.25, formants="keep"), ap.shift_prosody(x, None, 1.25))
    assert np.array_equal(ap.shift_prosody(x, None, None, formants="keep"), x)
    assert np.array_equal(ap.shift_prosody(x, 0.0, None, formants="keep"), x)         # a pitch ratio of 1
    assert np.array_equal(ap.shift_prosody(x, 4, None, formants="shift"), ap.shift_prosody(x, 4, None))


def test_shift_prosody_without_the_argument_is_the_parent_commits():
    ap = _ap()
    with open(os.path.join(ROOT, "tests", "golden", "formant_golden.json")) as f:
        rec = json.load(f)
    assert len(rec["cases"]) == 12
    with np.load(os.path.join(ROOT, "tests", "golden", "host_golden.npz")) as z:
        for c in rec["cases"]:
            for kw in ({}, {"formants": "shift"}, {"formants": None}):
                y = ap.shift_prosody(z[c["input"]], c["pitch"], c["tempo"], **kw)
                assert y.size == c["samples"] and hashlib.sha256(y.astype("<i2").tobytes()).hexdigest() == c["sha256"], c


# ------------------------------------------------------------------ plumbing
def test_check_formants_model_config_and_submit(tmp_path):
    from vietvoice_tts_amd.batching import BatchingFrontend
    from vietvoice_tts_amd.core import ModelConfig
    ap = _ap()
    assert ap.FORMANT_MODES == ("shift", "keep")
    assert ap.check_formants(None) == ap.check_formants("shift") == "shift" and ap.check_formants("keep") == "keep"
    for bad in ("Keep", "", 1, True, 0.5, ["keep"]):
        with pytest.raises(ValueError, match="output_formants"):
            ap.check_formants(bad)
    make = lambda **kw: ModelConfig(model_cache_dir=str(tmp_path), synthetic_model=True, **kw)  # noqa: E731
    assert make().output_formants == "shift" and make(output_formants="keep", output_pitch=3).output_formants == "keep"
    assert make(output_formants=None).output_formants == "shift"
    with pytest.raises(ValueError, match="output_formants"):
        make(output_formants="hold")
    fe = BatchingFrontend(engine=None, overlap=False)
    try:
        for bad in ("hold", 1, True):
            with pytest.raises(ValueError, match="output_formants"):
                fe.submit("x", formants=bad).result(timeout=5)
    finally:
        fe.close()


def test_plan_formant_on_hand_worked_rows():
    from vietvoice_tts_amd import pcm_stage as P
    rows = [[3, 1000, 8, 800, 8, 5, 4], [1100, 0, 900, 0, 900, 1, 1], [1200, 257, 1000, 257, 1001, 1, 1], [1500, 256, 2000, 342, 1300, 3, 4]]
    full, frame_offs, n_z = P.plan_formant(rows, 2000, 2400)
    assert full == rows and n_z == 1642
    assert frame_offs == [0, 5, 6, 9, 12]                       # ceil(800 / 256) + 1, 1, ceil(257 / 256) + 1, ceil(342 / 256) + 1
    assert P.plan_formant(rows, 2000, 2400, out_n=1642)[2] == 1642
    bad = {
        "seven entries": [[0, 10, 0, 10, 0, 1]],
        "n_f": [[0, 1000, 0, 801, 0, 5, 4]],
        "past x": [[1001, 1000, 0, 1000, 0, 1, 1]],
        "past y": [[0, 1000, 1401, 1000, 0, 1, 1]],
        "negative": [[0, 10, 0, 10, -1, 1, 1]],
        "tn": [[0, 10, 0, 10, 0, 0, 1]],
        "td": [[0, 10, 0, 10, 0, 1, 2049]],
        "overlap on z": [[0, 300, 0, 300, 0, 1, 1], [300, 300, 300, 300, 299, 1, 1]],
        "no rows": [],
    }
    for name, r in bad.items():
        with pytest.raises(ValueError, match="pcm_formant"):
            P.plan_formant(r, 2000, 2400)
            pytest.fail(name)
    with pytest.raises(ValueError, match="out holds"):
        P.plan_formant(rows, 2000, 2400, out_n=1641)
    with pytest.raises(ValueError, match="not in place"):
        P.plan_formant(rows, 2000, 2400, overlaps=True)


def test_plan_keep_picks_the_requests_with_keep_and_a_pitch():
    from vietvoice_tts_amd import pcm_stage as P
    ap = _ap()
    lens, offs = [1000, 600, 500, 0, 700], [0, 1000, 1600, 2104, 2112]
    pitch, tempo = [4, None, None, 4, -3], [1.25, 1.25, None, None, None]
    forms = ["keep", "keep", "keep", "keep", "shift"]
    new_offs, new_lens, *_rest = P.plan_prosody(offs, lens, pitch, tempo)
    plans = [ap.prosody_plan(n, p, t) for n, p, t in zip(lens, pitch, tempo)]
    rows = P.plan_keep(plans, offs, lens, new_offs, new_lens, forms)
    assert rows == [[0, 1000, new_offs[0], 800, new_offs[0], 5, 4]]                   # tempo alone, plain, empty and "shift" run nothing new
    forms[4] = "keep"
    assert P.plan_keep(plans, offs, lens, new_offs, new_lens, forms)[1] == [2112, 700, new_offs[4], 700, new_offs[4], 1, 1]
    assert P.plan_finish(3, pitch=[4, None, None]) == ([4, None, None], [None, None, None], [])      # the pinned plans are as before


def test_header_version_script_and_exports_agree_for_the_new_entries():
    from vietvoice_tts_amd import build_ext, runtime
    hdr = open(os.path.join(ROOT, "include", "vvtts.h")).read()
    declared = set(re.findall(r"VV_API\s+[\w\s\*]+?\b(vv_\w+)\s*\(", hdr))
    assert declared == set(runtime.EXPORTS), declared ^ set(runtime.EXPORTS)
    ver = open(os.path.join(ROOT, "vietvoice-tts_amd", "csrc", "vvtts.map")).read()
    globs = [g.strip() for g in re.findall(r"global:\s*([^;]+);", ver)]
    lib = runtime.load_library()
    for name, n_args in (("vv_pcm_formant", 18), ("vv_pcm_formant_ws_bytes", 2)):
        assert name in declared and len(runtime.EXPORTS[name][1]) == n_args
        assert any(re.fullmatch(g.replace("*", ".*"), name) for g in globs) and hasattr(lib, name)
    assert "vv_formant" in build_ext.SOURCES
    args = [None if t is ctypes.c_void_p else 0 for t in runtime.EXPORTS["vv_pcm_formant"][1]]
    assert lib.vv_pcm_formant(*args) == -22                                           # no context: refused before anything else
    assert len(runtime.EXPORTS["vv_pcm_stretch"][1]) == 14                            # the old entry keeps its arguments
    small, big = lib.vv_pcm_formant_ws_bytes(5, 1), lib.vv_pcm_formant_ws_bytes(50, 4)
    assert small >= 5 * fu.L * 8 and big >= 50 * fu.L * 8 + 4 * 16 and big > small
    m = re.match(rb"vvtts-hip (\d+)\.(\d+) ", lib.vv_version())
    assert m and (int(m.group(1)), int(m.group(2))) >= (0, 11)                        # bumped with the additive entries


# ------------------------------------------------------------------ engine and front end on injected sessions: the host mirror
def test_engine_and_front_end_apply_the_mirror_on_oracle_sessions(tmp_path):
    import torch
    from oracle.vv_oracle import Oracle, OracleSession
    from vietvoice_tts_amd.batching import BatchingFrontend
    from vietvoice_tts_amd.core import ModelConfig, TTSEngine
    ap = _ap()
    text = "Hôm nay trời đẹp quá, chúng ta cùng nhau đi dạo quanh hồ nhé."
    cfg = ModelConfig(model_cache_dir=str(tmp_path), synthetic_model=True, model_spec="tiny", nfe_step=3, max_chunk_duration=8.0)

    def factory(spec, weights, config):
        orc = Oracle(spec, weights, nfe_step=config.nfe_step)
        return {k: OracleSession(orc, k, seed=config.random_seed) for k in ("preprocess", "transformer", "decode")}

    eng = TTSEngine(cfg, session_factory=factory)

    def reseed():
        for sess in eng.model_session_manager.sessions.values():
            sess.gen = torch.Generator().manual_seed(123)

    try:
        reseed()
        base, _ = eng.synthesize(text)
        cfg.output_formants = "keep"
        reseed()
        assert np.array_equal(eng.synthesize(text)[0], base)                          # "keep" without a pitch: nothing happens
        cfg.output_pitch = 4
        reseed()
        got, _ = eng.synthesize(text)
        want = ap.shift_prosody(base, 4, None, formants="keep")
        assert np.array_equal(got, want) and not np.array_equal(want, ap.shift_prosody(base, 4, None))
        cfg.output_pitch, cfg.output_formants = None, "shift"
        fe = BatchingFrontend(eng, overlap=False)
        try:
            reseed()
            own = fe.submit(text, pitch=4, formants="keep").result(timeout=300)[0]
            reseed()
            moved = fe.submit(text, pitch=4).result(timeout=300)[0]
        finally:
            fe.close()
        assert np.array_equal(own, want) and np.array_equal(moved, ap.shift_prosody(base, 4, None))
    finally:
        eng.cleanup()
