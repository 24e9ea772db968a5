"""N16 without a GPU: LPC subframes in the host mirror of the FLAC encoder (core/audio_processor.py: flac_lpc_coefficients, flac_choose
and flac_encode_frames with ``lpc_order``, FlacStream) against a decoder that knows nothing of the mirror and a code-by-code count of
the subframe's bits (tests/flac_lpc_util.py), the known answers of the recipe, and the plumbing (config, ABI).  The device is held
against the mirror in tests/test_flac_lpc_gpu.py."""
import ctypes
import os
import re
from collections import Counter

import numpy as np
import pytest

from tests.flac_lpc_util import decode_frames, lpc_bits, lpc_cases, mirror_layout, no_energy
from tests.flac_util import BLOCK, best_subframe, decode_stream, device_cases, fixed_bits, signals, speechlike

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SR = 24000
ORDERS = (1, 8, 12)


def _ap():
    from vietvoice_tts_amd.core import audio_processor
    return audio_processor


# ------------------------------------------------------------------ known answers of the recipe
def test_known_answers_one_frame_signals():
    """Subframe bits of one frame of 4096 samples, fixed only and with max_order 12, and the winning order: the figures of the recipe's
    prototype.  Another reading of any step (window, lag sums, operation order in Levinson, quantisation, tie rule) moves them."""
    ap = _ap()
    want = dict(sine1k=(31113, 11740, 11), sine200=(12683, 8350, 5), alternating=(65544, 4204, 3), walk20=(23872, 23867, 1))
    for name, x in signals().items():
        fixed, lpc = ap.flac_choose(x), ap.flac_choose(x, 12)
        if name in want:
            assert (fixed[4], lpc[4], lpc[0], lpc[1]) == want[name][:2] + ("lpc", want[name][2]), (name, fixed, lpc)
        else:                                                      # noise and switching signals, zeros, ramp: unchanged
            assert lpc[:5] == fixed and lpc[5] == (0, []), name


def test_known_answers_speechlike():
    ap = _ap()
    x = speechlike(144000)
    fixed = [ap.flac_choose(x[i: i + BLOCK]) for i in range(0, x.size, BLOCK)]
    lpc = [ap.flac_choose(x[i: i + BLOCK], 12) for i in range(0, x.size, BLOCK)]
    assert len(lpc) == 36 and all(c[0] == "lpc" for c in lpc)
    ratio = [sum(c[4] for c in chosen) / 8 / x.nbytes for chosen in (fixed, lpc)]      # subframe bits over the raw size
    assert [round(r, 4) for r in ratio] == [0.5573, 0.5314], ratio
    orders = Counter(c[1] for c in lpc)
    assert orders[12] == 24 and sum(orders[p] for p in (8, 9, 10, 11)) == 12 and set(orders) <= {8, 9, 10, 11, 12}, orders


# ------------------------------------------------------------------ order 0 is the encoder as it was
def test_order_zero_is_the_fixed_only_encoder_byte_for_byte():
    ap = _ap()
    for name, x, frame0, last in device_cases():
        old = ap.flac_encode_frames(x, SR, frame0, bool(last))
        new = ap.flac_encode_frames(x, SR, frame0, bool(last), lpc_order=0)
        assert np.array_equal(old[0], new[0]) and old[1:] == new[1:], name
    x = signals()["sine1k"]
    assert ap.flac_choose(x, 0) == ap.flac_choose(x) and len(ap.flac_choose(x)) == 5
    assert np.array_equal(ap.encode_output(x, "flac", SR, lpc_order=0), ap.encode_output(x, "flac", SR))


# ------------------------------------------------------------------ round trip, frame numbers, CRCs, never larger
@pytest.fixture(scope="module")
def fixed_sizes():
    ap = _ap()
    return {c[0]: [f["bytes"] for f in decode_frames(ap.flac_encode_frames(c[1], SR, c[2], bool(c[3]))[0], SR, c[2])[1]] for c in lpc_cases()}


@pytest.mark.parametrize("order", ORDERS)
def test_round_trip_is_exact_and_no_frame_grows(order, fixed_sizes):
    ap = _ap()
    seen, highest = set(), 0
    for name, x, frame0, last in lpc_cases():
        data, lo, hi = ap.flac_encode_frames(x, SR, frame0, bool(last), order)
        samples, frames, numbers = decode_frames(data, SR, frame0)             # checks CRC-8, CRC-16 and the frame numbers
        assert np.array_equal(samples, x), name
        sizes = [f["bytes"] for f in frames]
        assert (lo, hi) == (min(sizes), max(sizes)) and len(sizes) == len(fixed_sizes[name]), name
        assert all(a <= b for a, b in zip(sizes, fixed_sizes[name])), (name, sizes, fixed_sizes[name])
        for f, frame in enumerate(frames):
            what, m = frame["what"], frame["m"]
            assert frame["bytes"] <= ap.flac_frame_bound(m) and frame["bits"] <= 8 + 16 * m
            chosen = ap.flac_choose(x[f * BLOCK: (f + 1) * BLOCK], order)
            assert what[:4] == chosen[:4] and frame["bits"] == chosen[4], (name, f)
            seen.add(what[0])
            if what[0] == "lpc":
                assert what[4:] == (12, chosen[5][0], chosen[5][1]) and 1 <= what[1] <= min(order, m - 1) and 0 <= what[5] <= 15
                assert all(-2048 <= c <= 2047 for c in what[6]) and all(0 <= k <= 14 for k in what[3])
                highest = max(highest, what[1])
    assert seen == {"constant", "verbatim", "fixed", "lpc"} and highest == order


def test_short_frames():
    """m = 2 has no window (m >= 3 is needed) and stays Fixed or verbatim; m = 3 has one sample under the window, so every lag but R[0]
    is zero, every coefficient too, and no order is a candidate; m = 13, 14 try orders up to m - 1 at the most."""
    ap = _ap()
    cases = {c[0]: c[1] for c in lpc_cases()}
    assert ap.flac_lpc_coefficients(cases["short_2"], 12) == {} and ap.flac_choose(cases["short_2"], 12)[:5] == ap.flac_choose(cases["short_2"])
    assert ap.flac_lpc_coefficients(cases["short_3"], 12) == {} and cases["short_3"][1] != 0
    for m in (13, 14):
        got = ap.flac_lpc_coefficients(cases[f"short_{m}"], 12)
        assert got and max(got) <= min(12, m - 1) and all(len(q) == p and 0 <= s <= 15 for p, (s, q) in got.items()), m
    assert ap.flac_lpc_coefficients(np.array([-5], np.int16), 12) == {}


# ------------------------------------------------------------------ the size, code by code
def test_chosen_subframe_size_by_brute_force():
    """On short frames: the size of every LPC candidate of the mirror's predictors, counted code by code over every partition order and
    k, against the mirror's choice; the winner is the smallest of Fixed (tests/flac_util.best_subframe) and LPC, Fixed first of equals."""
    ap = _ap()
    rng = np.random.default_rng(16)
    won = Counter()
    for case in range(120):
        m = int(rng.integers(16, 65))
        t = np.arange(m)
        shape = case % 4
        if shape == 0:
            x = 9000 * np.sin(2 * np.pi * t / rng.uniform(3, 20) + rng.uniform(0, 6)) + rng.normal(0, rng.choice([0.5, 30]), m)
        elif shape == 1:
            x = np.cumsum(rng.integers(-200, 201, m))
        elif shape == 2:
            x = np.where(t % 2 == 0, 1, -1) * rng.integers(5000, 30000) + rng.integers(-3, 4, m)
        else:
            x = rng.integers(-40, 41, m)
        x = np.clip(np.rint(x), -32768, 32767).astype(np.int16)
        order = int(rng.choice([1, 4, 8, 12]))
        best = best_subframe(x)                                                # constant / Fixed / verbatim by brute force
        if best[0] == "verbatim":                                              # verbatim yields to LPC of equal size; Fixed stays in front of it
            best = min((("fixed", o, po) + fixed_bits(list(x), o, po)[::-1] for o in range(5) for po in range(5) if fixed_bits(list(x), o, po)),
                       key=lambda c: (c[4], c[1], c[2]))
        for p, (shift, q) in sorted(ap.flac_lpc_coefficients(x, order).items()):
            for po in range(5):
                got = lpc_bits(list(x), shift, q, po)
                if got is not None and got[0] < best[4]:
                    best = ("lpc", p, po, got[1], got[0], (shift, q))
        if best[0] != "constant" and 8 + 16 * m < best[4]:
            best = ("verbatim", 0, 0, [], 8 + 16 * m)
        chosen = ap.flac_choose(x, order)
        assert chosen[:5] == best[:5] and (best[0] != "lpc" or chosen[5] == best[5]), (case, chosen, best)
        frame = ap.flac_encode_frame(x, SR, case, order)
        assert len(frame) == 4 + 1 + 2 + 1 + -(-best[4] // 8) + 2, case
        assert np.array_equal(decode_frames(frame, SR, case)[0], x), case
        won[best[0]] += 1
    assert won["lpc"] >= 20 and won["fixed"] >= 20, won


def test_no_energy_under_the_window_stays_fixed():
    ap = _ap()
    x = no_energy()
    assert ap.flac_lpc_coefficients(x, 12) == {}                               # the window is zero at both ends: R[0] == 0
    assert ap.flac_choose(x, 12)[:5] == ap.flac_choose(x) and ap.flac_choose(x, 12)[0] == "fixed"
    assert np.array_equal(ap.flac_encode_frames(x, SR, 0, True, 12)[0], ap.flac_encode_frames(x, SR)[0])


# frames whose smallest LPC subframe has EXACTLY the size of the smallest Fixed one.  Found once by a seeded search over short sines;
# hard-coded so that the case cannot silently go missing
LPC_TIES = (
    [81, 118, 133, 114, 72, 14, -47, -100, -126, -127, -97, -46, 12, 72, 114, 130, 118, 79, 24, -43],
    [773, 1089, 1166, 986, 599, 78, -459, -896, -1139, -1134, -886, -443, 95, 611, 994, 1166, 1084, 763, 282, -263, -751, -1077, -1165, -1007],
    [-368, -985, -1420, -1586, -1465, -1067, -475, 204, 851, 1335, 1575, 1521, 1185, 632, -39, -704, -1235, -1541, -1560, -1290, -783, -130, 548, 1124],
)


def test_a_tie_goes_to_fixed():
    ap = _ap()
    for y in LPC_TIES:
        x = np.array(y, np.int16)
        fixed = best_subframe(x)
        sizes = [lpc_bits(y, shift, q, po) for shift, q in ap.flac_lpc_coefficients(x, 12).values() for po in range(5)]
        assert fixed[0] == "fixed" and min(v[0] for v in sizes if v is not None) == fixed[4]         # equal, counted code by code
        assert ap.flac_choose(x, 12)[:5] == fixed
        assert ap.flac_encode_frame(x, SR, 0, 12) == ap.flac_encode_frame(x, SR, 0)
    x = np.array(LPC_TIES[0][:1] + [119] + LPC_TIES[0][2:], np.int16)                               # one step off the tie (118 -> 119): LPC is strictly smaller
    assert ap.flac_choose(x, 12)[0] == "lpc" and ap.flac_choose(x, 12)[4] < ap.flac_choose(x)[4]


# ------------------------------------------------------------------ FlacStream, encode_output
@pytest.mark.parametrize("order", [(1, 4095, 4096, 4097, 10000), (4096, 4096), (5000, 1, 7287)])
def test_flac_stream_with_an_order_adds_up_to_the_buffered_frames(order):
    ap = _ap()
    x = speechlike(sum(order), 11)
    fs, out, at = ap.FlacStream(SR, lpc_order=8), [], 0
    for n in order:
        out.append(fs.push(x[at: at + n]))
        at += n
    out.append(fs.flush())
    data = np.concatenate(out)
    assert data[:42].tobytes() == ap.flac_stream_header(SR, 0)
    assert np.array_equal(data[42:], ap.flac_encode_frames(x, SR, lpc_order=8)[0])
    assert np.array_equal(data[42:], ap.encode_output(x, "flac", SR, lpc_order=8)[42:])
    assert not np.array_equal(data[42:], ap.flac_encode_frames(x, SR)[0]) and np.array_equal(decode_frames(data[42:], SR, 0)[0], x)


def test_flac_stream_passes_the_order_to_its_back_end():
    ap, calls = _ap(), []

    def backend(pcm, frame0, last, lpc_order=0):
        calls.append((pcm.size, frame0, last, lpc_order))
        return ap.flac_encode_frames(pcm, 8000, frame0, last, lpc_order)[0]
    x = speechlike(BLOCK + 7, 2, 8000)
    fs = ap.FlacStream(8000, backend, 12)
    data = np.concatenate([fs.push(x), fs.flush()])
    assert calls == [(BLOCK, 0, False, 12), (7, 1, True, 12)] and np.array_equal(decode_frames(data[42:], 8000, 0)[0], x)
    calls.clear()
    fs = ap.FlacStream(8000, lambda pcm, frame0, last: backend(pcm, frame0, last))          # without an order: the call of before
    fs.push(x)
    assert calls == [(BLOCK, 0, False, 0)]
    for bad in (-1, 13, 1.0, True, "8"):
        with pytest.raises(ValueError):
            ap.FlacStream(8000, lpc_order=bad)


def test_encode_output_file_with_an_order():
    ap = _ap()
    x = signals(BLOCK + 300)["sine1k"]
    small, plain = ap.encode_output(x, "flac", SR, lpc_order=12), ap.encode_output(x, "flac", SR)
    assert small.size < 0.5 * plain.size
    info = decode_stream(plain)[2]
    assert info["total"] == x.size
    samples, frames, _n = decode_frames(small[42:], SR, 0)
    assert np.array_equal(samples, x) and [f["what"][0] for f in frames] == ["lpc", "lpc"]
    head = ap.flac_stream_header(SR, x.size, min(f["bytes"] for f in frames), max(f["bytes"] for f in frames))
    assert small[:42].tobytes() == head
    with pytest.raises(ValueError):
        ap.encode_output(x, "ulaw", SR, lpc_order=4)
    with pytest.raises(ValueError):
        ap.encode_output(x, "flac", SR, lpc_order=13)


def test_mirror_layout_rows_are_independent():
    cases = lpc_cases()
    whole, info, bound = mirror_layout(cases, SR, 12)
    assert info[-1, 0] == whole.size <= bound and len(cases) == len(device_cases()) + 5
    ap = _ap()
    for j, (name, x, frame0, last) in enumerate(cases):
        assert np.array_equal(whole[info[j, 0]: info[j + 1, 0]], ap.flac_encode_frames(x, SR, frame0, bool(last), 12)[0]), name


# ------------------------------------------------------------------ config
def test_model_config_validation():
    from vietvoice_tts_amd.core import ModelConfig
    base = dict(model_cache_dir="/tmp/x", synthetic_model=True, model_spec="tiny")
    assert ModelConfig(**base).flac_lpc_order == 0 and ModelConfig(output_encoding="flac", **base).flac_lpc_order == 0
    for order in (1, 8, 12):
        c = ModelConfig(output_encoding="flac", flac_lpc_order=order, **base)
        assert c.flac_lpc_order == order and ModelConfig.from_dict(c.to_dict()).flac_lpc_order == order
    for bad in (-1, 13, 2.5, 8.0, "8", True, None):
        with pytest.raises(ValueError, match="flac_lpc_order"):
            ModelConfig(output_encoding="flac", flac_lpc_order=bad, **base)
    for enc in ("pcm16", "ulaw", "alaw"):
        with pytest.raises(ValueError, match="flac"):
            ModelConfig(output_encoding=enc, flac_lpc_order=8, **base)
        assert ModelConfig(output_encoding=enc, flac_lpc_order=0, **base).flac_lpc_order == 0


# ------------------------------------------------------------------ engine on oracle sessions (the host path)
TEXT = "Hôm nay trời đẹp quá, chúng ta cùng nhau đi dạo quanh hồ nhé. " * 3


def test_engine_on_oracle_sessions_with_an_order(tmp_path):
    import torch
    from oracle.vv_oracle import Oracle, OracleSession
    from vietvoice_tts_amd.core import ModelConfig, TTSEngine

    def factory(spec, weights, config):
        orc = Oracle(spec, weights, nfe_step=config.nfe_step)
        return {k: OracleSession(orc, k, seed=config.random_seed) for k in ("preprocess", "transformer", "decode")}

    def run(eng, fn, enc, order):
        eng.config.output_encoding, eng.config.flac_lpc_order = enc, order
        for sess in eng.model_session_manager.sessions.values():
            sess.gen = torch.Generator().manual_seed(123)
        out = fn(TEXT)
        return list(out) if fn == eng.synthesize_stream else out[0]
    eng = TTSEngine(ModelConfig(model_cache_dir=str(tmp_path), synthetic_model=True, model_spec="tiny", nfe_step=3, max_chunk_duration=8.0,
                                output_encoding="flac", flac_lpc_order=8), session_factory=factory)
    try:
        pcm = run(eng, eng.synthesize, "pcm16", 0)
        got = run(eng, eng.synthesize, "flac", 8)
        blocks = run(eng, eng.synthesize_stream, "flac", 8)
    finally:
        eng.cleanup()
    assert pcm.dtype == np.int16 and pcm.size > 2 * BLOCK
    samples, frames, _numbers = decode_frames(got[42:], SR, 0)
    assert np.array_equal(samples, pcm) and got.size <= _ap().encode_output(pcm, "flac", SR).size
    assert np.array_equal(got, _ap().encode_output(pcm, "flac", SR, lpc_order=8))
    assert len(blocks) > 1 and np.array_equal(np.concatenate(blocks)[42:], got[42:])      # streamed == buffered frames


# ------------------------------------------------------------------ ABI
def test_header_version_script_and_exports_agree_for_the_new_entries():
    from vietvoice_tts_amd import runtime
    hdr = open(os.path.join(ROOT, "include", "vvtts.h")).read()
    declared = set(re.findall(r"VV_API\s+[\w\s\*]+?\b(vv_\w+)\s*\(", hdr))
    assert declared == set(runtime.EXPORTS), declared ^ set(runtime.EXPORTS)
    ver = open(os.path.join(ROOT, "vietvoice-tts_amd", "csrc", "vvtts.map")).read()
    globs = [g.strip() for g in re.findall(r"global:\s*([^;]+);", ver)]
    lib = runtime.load_library()
    for name, n_args in (("vv_pcm_flac_lpc", 14), ("vv_pcm_flac_lpc_ws_bytes", 3)):
        assert name in declared and len(runtime.EXPORTS[name][1]) == n_args
        assert any(re.fullmatch(g.replace("*", ".*"), name) for g in globs) and hasattr(lib, name)
    assert len(runtime.EXPORTS["vv_pcm_flac"][1]) == 13                                   # the old entry keeps its arguments
    args = [None if t is ctypes.c_void_p else 0 for t in runtime.EXPORTS["vv_pcm_flac_lpc"][1]]
    assert lib.vv_pcm_flac_lpc(*args) == -22                                              # no context: refused before anything else
    assert int(re.search(r"#define VV_FLAC_MAX_LPC_ORDER (\d+)", hdr).group(1)) == _ap().FLAC_MAX_LPC_ORDER == 12
    old = lib.vv_pcm_flac_ws_bytes(66, 33)
    assert all(lib.vv_pcm_flac_lpc_ws_bytes(66, 33, p) >= old + 66 * 13 * 4 for p in (1, 12))
    assert [lib.vv_pcm_flac_lpc_ws_bytes(66, 33, p) for p in (0, -1, 13)] == [0, 0, 0]    # no such order
    m = re.match(rb"vvtts-hip (\d+)\.(\d+) ", lib.vv_version())
    assert m and (int(m.group(1)), int(m.group(2))) >= (0, 9)                             # bumped with the additive entries
