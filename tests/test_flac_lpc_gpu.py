"""-m gpu: N16, LPC subframes of the FLAC encoder on the device (csrc/vv_flac.hip: vv_pcm_flac_lpc) and through the engine.  The yardstick
is the host mirror (core/audio_processor.py: flac_encode_frames with ``lpc_order``), which the kernels must equal BYTE FOR BYTE, frame
sizes and offsets included; what the bytes mean is checked by the stand-alone decoder of tests/flac_lpc_util.py.  The mirror itself is
held against that decoder, a code-by-code count of the bits and the known answers of the recipe in tests/test_flac_lpc_cpu.py."""
import numpy as np
import pytest
import torch

from tests.flac_lpc_util import decode_frames, lpc_cases, mirror_layout
from tests.flac_util import BLOCK, decode_stream
from tests.output_util import pack_requests

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
SR = 24000
GUARD = 256
FILL = 0xAA
LONG = "Hôm nay trời đẹp quá, chúng ta cùng nhau đi dạo quanh hồ nhé. " * 4


@pytest.fixture(scope="module")
def eng(hip_tiny):
    return hip_tiny["f32"]


@pytest.fixture(scope="module")
def cases():
    res = lpc_cases()
    assert len(res) == 35 and sum(-(-c[1].size // BLOCK) for c in res) == 43           # rows and frames of the one call
    assert any(c[3] == 0 for c in res) and {1, 2, 3, 13, 14} <= {c[1].size for c in res} and any(c[0] == "no_energy" for c in res)
    return res


def _raw(eng, items, lpc_order, gap=3, rate=SR):
    """Device buffers of one vv_pcm_flac_lpc call over ``items``, made ahead of it: sources at odd offsets with junk between, y between
    guard bands.  -> (call(**overrides), whole y buffer, info, n_y, buffers)."""
    plane, reqs = pack_requests([[c[1]] for c in items], gap=gap)
    rows = [[so, n, c[2], c[3]] for c, ((so, n),) in zip(items, reqs)]
    n_y = sum(int(eng.lib.vv_flac_frame_bound(min(BLOCK, n - f * BLOCK))) for _so, n, _f0, _l in rows for f in range(-(-n // BLOCK)))
    x = torch.from_numpy(np.ascontiguousarray(plane)).to(DEV)
    whole = torch.full((GUARD + n_y + GUARD,), FILL, dtype=torch.uint8, device=DEV)
    info = torch.full((len(items) + 1, 3), -7, dtype=torch.int64, device=DEV)
    rows_h = torch.tensor(rows, dtype=torch.int64)
    rows_d = rows_h.to(DEV)
    frames = sum(-(-r[1] // BLOCK) for r in rows)
    ws = torch.zeros((int(eng.lib.vv_pcm_flac_lpc_ws_bytes(frames, len(rows), 12)) // 8 + 1,), dtype=torch.int64, device=DEV)

    def call(**kw):
        a = dict(x=x.data_ptr(), n_x=x.numel(), rows=rows_d.data_ptr(), rows_h=rows_h.data_ptr(), R=len(rows), rate=rate, lpc_order=lpc_order,
                 y=whole.data_ptr() + GUARD, n_y=n_y, info=info.data_ptr(), ws=ws.data_ptr(), ws_bytes=ws.numel() * 8)
        a.update(kw)
        return eng.lib.vv_pcm_flac_lpc(eng.ctx, a["x"], a["n_x"], a["rows"], a["rows_h"], a["R"], a["rate"], a["lpc_order"], a["y"], a["n_y"],
                                       a["info"], a["ws"], a["ws_bytes"], torch.cuda.current_stream().cuda_stream)
    return call, whole, info, n_y, (x, rows, rows_h, rows_d, ws)


def _launch(eng, items, lpc_order, gap=3):
    """One call over ``items``, everything checked against the mirror.  -> {name: the request's frames}."""
    call, whole, info, n_y, _keep = _raw(eng, items, lpc_order, gap)
    assert call() == 0
    torch.cuda.synchronize()
    want, want_info, bound = mirror_layout([c[:4] for c in items], SR, lpc_order)
    assert bound == n_y and torch.equal(info.cpu(), torch.from_numpy(want_info))
    total = int(info[-1, 0])
    assert total == want.size and torch.equal(whole[GUARD: GUARD + total].cpu(), torch.from_numpy(want))
    assert bool((whole[:GUARD] == FILL).all()) and bool((whole[GUARD + total:] == FILL).all()), "a byte outside the frames was written"
    host, got_info = whole.cpu().numpy(), info.cpu().numpy()
    return {c[0]: host[GUARD + int(got_info[j, 0]): GUARD + int(got_info[j + 1, 0])].copy() for j, c in enumerate(items)}


@pytest.fixture(scope="module")
def batches(eng, cases):
    """{order: {name: frames}} of one shuffled call per order over every row."""
    order = [cases[i] for i in np.random.default_rng(6).permutation(len(cases))]
    return {p: _launch(eng, order, p) for p in (1, 12)}


@pytest.mark.parametrize("lpc_order", [1, 12])
def test_one_call_over_every_row_equals_the_mirror_and_decodes(cases, batches, lpc_order):
    kinds, orders = set(), set()
    for name, x, frame0, _last in cases:
        samples, frames, _numbers = decode_frames(batches[lpc_order][name], SR, frame0)
        assert np.array_equal(samples, x), name
        kinds.update(f["what"][0] for f in frames)
        orders.update(f["what"][1] for f in frames if f["what"][0] == "lpc")
    assert kinds == {"constant", "verbatim", "fixed", "lpc"} and max(orders) == lpc_order and min(orders) == 1
    what = decode_frames(batches[lpc_order]["no_energy"], SR, 9)[1][0]["what"]
    assert what[0] == "fixed"                                                  # R[0] == 0: no LPC candidate on the device either


def test_a_row_alone_equals_the_row_in_the_batch(eng, cases, batches):
    pick = [c for c in cases if c[0] in ("sine1k", "alternating", "speech_13288", "one", "short_3", "short_13", "no_energy", "stream_block", "noise_17")]
    assert len(pick) == 9
    for i, c in enumerate(pick):
        alone = _launch(eng, [c], 12, gap=1 + i % 4)
        assert np.array_equal(alone[c[0]], batches[12][c[0]]), c[0]
    moved = _launch(eng, pick[::-1], 12, gap=5)                                # another position, other neighbours
    for c in pick:
        assert np.array_equal(moved[c[0]], batches[12][c[0]]), c[0]


def test_refusals_launch_nothing_and_leave_the_context_usable(eng, cases):
    items = [c for c in cases if c[0] in ("walk_4097", "stream_block", "five")]
    call, whole, info, n_y, (x, rows, rows_h, rows_d, ws) = _raw(eng, items, 12)
    variants = {k: rows_h.clone() for k in ("past_x", "neg_src", "neg_n", "neg_frame0", "neg_last", "empty", "frames_past_2_31", "partial_block",
                                            "last_2")}
    variants["past_x"][0, 1] = x.numel()
    for col, k in ((0, "neg_src"), (1, "neg_n"), (2, "neg_frame0"), (3, "neg_last")):
        variants[k][0, col] = -1
    variants["empty"][2, 1] = 0
    variants["frames_past_2_31"][0, 2] = (1 << 31) - 1
    variants["partial_block"][1, 1] = 2 * BLOCK - 1
    variants["last_2"][0, 3] = 2
    assert sum(-(-r[1] // BLOCK) for r in rows) == 5                           # vv_pcm_flac's workspace for them is too small here
    bads = [dict(lpc_order=0), dict(lpc_order=-1), dict(lpc_order=13), dict(lpc_order=1 << 20),
            dict(R=0), dict(R=-1), dict(R=65536), dict(x=None), dict(rows=None), dict(rows_h=None), dict(y=None), dict(info=None), dict(ws=None),
            dict(x=x.data_ptr() + 1), dict(rows=rows_d.data_ptr() + 4), dict(info=info.data_ptr() + 4), dict(ws=ws.data_ptr() + 4),
            dict(ws_bytes=int(eng.lib.vv_pcm_flac_ws_bytes(5, 3))), dict(ws_bytes=0), dict(n_y=n_y - 1), dict(n_y=0), dict(rate=0), dict(rate=-5),
            dict(rate=655351), dict(n_x=100)]
    bads += [dict(rows_h=v.data_ptr()) for v in variants.values()]
    for bad in bads:
        assert call(**bad) == -22, bad
        assert b"vv_pcm_flac_lpc" in eng.lib.vv_last_error(eng.ctx)
    torch.cuda.synchronize()
    assert bool((whole == FILL).all()) and bool((info == -7).all())            # nothing was launched
    for bad_order in (-1, 13, 2.0, True):
        with pytest.raises(ValueError):
            eng.pcm_flac(x, rows, SR, bad_order)
    assert call() == 0                                                         # the context still works
    torch.cuda.synchronize()
    want = mirror_layout([c[:4] for c in items], SR, 12)[0]
    assert torch.equal(whole[GUARD: GUARD + int(info[-1, 0])].cpu(), torch.from_numpy(want))
    y, inf = eng.pcm_flac(x, rows, SR, 12)                                     # the wrapper: the same bytes
    assert torch.equal(y[: int(inf[-1, 0])].cpu(), torch.from_numpy(want))


def test_the_old_entry_gives_its_old_bytes_after_the_new_one(eng, cases, batches):
    items = [c for c in cases if c[0] in ("sine1k", "alternating", "speech_13288", "two", "stream_block", "verbatim_tie_16")]
    plane, reqs = pack_requests([[c[1]] for c in items], gap=3)
    rows = [[so, n, c[2], c[3]] for c, ((so, n),) in zip(items, reqs)]
    x = torch.from_numpy(np.ascontiguousarray(plane)).to(DEV)
    eng.pcm_flac(x, rows, SR, 12)
    y, info = eng.pcm_flac(x, rows, SR)
    want, want_info, _bound = mirror_layout([c[:4] for c in items], SR, 0)
    assert torch.equal(info.cpu(), torch.from_numpy(want_info)) and torch.equal(y[: want.size].cpu(), torch.from_numpy(want))
    assert want.size > sum(batches[12][c[0]].size for c in items)              # and the new one is smaller on these rows


# ------------------------------------------------------------------ engine, tiny preset
@pytest.fixture(scope="module")
def tiny(tmp_path_factory):
    from vietvoice_tts_amd.core import ModelConfig, TTSEngine
    e = TTSEngine(ModelConfig(model_cache_dir=str(tmp_path_factory.mktemp("flac_lpc_models")), synthetic_model=True, nfe_step=5, acoustic_dtype="fp32",
                              max_chunk_duration=8.0, model_spec="tiny", noise_source="device", output_stage="device", output_encoding="flac",
                              flac_lpc_order=8))
    yield e
    e.cleanup()


def _call(e, fn, *a, enc="flac", order=8, **k):
    """One engine call under the given encoding and LPC order, from call serial 0 (the same start noise every time)."""
    e.config.output_encoding, e.config.flac_lpc_order = enc, order
    e.model_session_manager.noise_serial = 0
    try:
        out = fn(*a, **k)
        return list(out) if fn == e.synthesize_stream else out
    finally:
        e.config.output_encoding, e.config.flac_lpc_order = "flac", 8


def test_engine_file_stream_and_size(tiny, tmp_path, monkeypatch):
    from vietvoice_tts_amd.core.audio_processor import encode_output
    e = tiny
    lib, calls = e.model_session_manager.engine.lib, []
    for name in ("vv_pcm_flac", "vv_pcm_flac_lpc"):
        monkeypatch.setattr(lib, name, (lambda real, name: lambda *a: calls.append(name) or real(*a))(getattr(lib, name), name))
    pcm, _ = _call(e, e.synthesize, LONG, enc="pcm16", order=0)
    assert len(e._last_plan) >= 3 and pcm.dtype == np.int16 and pcm.size > 2 * BLOCK and not calls
    path = tmp_path / "x.flac"
    got, _ = _call(e, e.synthesize, LONG, output_path=str(path))
    assert calls == ["vv_pcm_flac_lpc"] and got.dtype == np.uint8 and path.read_bytes() == got.tobytes()
    samples, frames, _numbers = decode_frames(got[42:], SR, 0)
    assert np.array_equal(samples, pcm) and any(f["what"][0] == "lpc" for f in frames)
    assert np.array_equal(got, encode_output(pcm, "flac", SR, lpc_order=8))    # host and device files are equal
    blocks = _call(e, e.synthesize_stream, LONG)
    streamed = np.concatenate(blocks)
    assert len(blocks) > 1 and np.array_equal(streamed[42:], got[42:]) and set(calls) == {"vv_pcm_flac_lpc"}
    calls.clear()
    plain, _ = _call(e, e.synthesize, LONG, order=0)
    assert calls == ["vv_pcm_flac"] and np.array_equal(decode_stream(plain)[0], pcm) and got.size <= plain.size
