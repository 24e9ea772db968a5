"""Speech editing, host side: the edit plan on the hop grid against plans worked out by hand, every validation
error of the planner, and the refusal of an engine without the HIP path.  No GPU."""
import numpy as np
import pytest

from vietvoice_tts_amd.speech_edit import plan_edit

SR, HOP, NFFT, MAXF = 24000, 256, 1024, 4096


def fr(f):
    """f frames in seconds (on the hop grid)."""
    return f * HOP / SR


def keep_of(n, gaps):
    k = np.ones(n, dtype=np.uint8)
    for f0, f1 in gaps:
        k[f0:f1] = 0
    return k


CASES = {
    # name: (S, parts, fix_duration, segments (src_off, dst_off, n), gaps, L)
    "same_length_middle": (100 * HOP, [(fr(30), fr(40))], None,
                           [(0, 0, 30 * HOP), (40 * HOP, 40 * HOP, 60 * HOP)], [(30, 40)], 100 * HOP),
    "longer": (100 * HOP, [(fr(30), fr(40))], [fr(15)],
               [(0, 0, 30 * HOP), (40 * HOP, 45 * HOP, 60 * HOP)], [(30, 45)], 105 * HOP),
    "deletion": (100 * HOP, [(fr(30), fr(40))], [0.0],
                 [(0, 0, 30 * HOP), (40 * HOP, 30 * HOP, 60 * HOP)], [(30, 30)], 90 * HOP),
    "insertion": (100 * HOP, [(fr(50), fr(50))], [fr(8)],
                  [(0, 0, 50 * HOP), (50 * HOP, 58 * HOP, 50 * HOP)], [(50, 58)], 108 * HOP),
    "span_at_zero": (100 * HOP, [(0.0, fr(5))], None,
                     [(5 * HOP, 5 * HOP, 95 * HOP)], [(0, 5)], 100 * HOP),
    # S = 100 hops + 100 samples: the span's end (S / sr) snaps to H = 100 hops, the final partial hop is kept after the gap
    "end_partial_hop": (100 * HOP + 100, [(fr(90), (100 * HOP + 100) / SR)], [fr(12)],
                        [(0, 0, 90 * HOP), (100 * HOP, 102 * HOP, 100)], [(90, 102)], 102 * HOP + 100),
    "two_spans": (100 * HOP, [(fr(10), fr(20)), (fr(50), fr(55))], [fr(5), fr(9)],
                  [(0, 0, 10 * HOP), (20 * HOP, 15 * HOP, 30 * HOP), (55 * HOP, 54 * HOP, 45 * HOP)], [(10, 15), (45, 54)], 99 * HOP),
}


@pytest.mark.parametrize("name", sorted(CASES))
def test_plan_edit_matches_hand_plan(name):
    S, parts, fix, segs, gaps, L = CASES[name]
    p = plan_edit(S, parts, fix, SR, HOP, NFFT, MAXF)
    assert [tuple(s) for s in p.segments] == segs
    assert [tuple(g) for g in p.gaps] == gaps
    assert p.spliced_len == L
    assert p.n_frames == L // HOP + 1
    assert p.keep.dtype == np.uint8 and np.array_equal(p.keep, keep_of(L // HOP + 1, gaps))
    # the segments and the gaps tile [0, L) in order, every gap starts on the hop grid
    pos = 0
    spans = sorted([(d, n, "seg") for _s, d, n in segs] + [(f0 * HOP, (f1 - f0) * HOP, "gap") for f0, f1 in gaps])
    for d, n, _k in spans:
        assert d == pos
        pos += n
    assert pos == L
    assert p.rows(item=2, src_base=1000) == [[2, 1000 + s, d, n] for s, d, n in segs]


def test_plan_without_parts_keeps_every_frame():
    p = plan_edit(100 * HOP + 7, [], None, SR, HOP, NFFT, MAXF)
    assert p.segments == ((0, 0, 100 * HOP + 7),) and p.gaps == () and p.spliced_len == 100 * HOP + 7
    assert p.n_frames == 101 and bool(p.keep.all())


@pytest.mark.parametrize("parts, fix, S, maxf, match", [
    ([(-0.01, fr(10))], None, 100 * HOP, MAXF, "start <= end"),                        # start < 0
    ([(fr(10), fr(101))], None, 100 * HOP, MAXF, "start <= end"),                      # end past the clip
    ([(fr(20), fr(10))], None, 100 * HOP, MAXF, "start <= end"),                       # start > end
    ([(fr(10), fr(20))], [-0.5], 100 * HOP, MAXF, ">= 0"),                             # negative new length
    ([(fr(10), fr(20))], [float("nan")], 100 * HOP, MAXF, ">= 0"),
    ([(fr(10), fr(20))], [0.1, 0.2], 100 * HOP, MAXF, "entries"),                      # len(fix_duration) != P
    ([(fr(10), fr(20))], [], 100 * HOP, MAXF, "entries"),
    ([(fr(10), fr(30)), (fr(20), fr(40))], None, 100 * HOP, MAXF, "overlap"),           # overlapping spans
    ([(fr(50), fr(60)), (fr(10), fr(20))], None, 100 * HOP, MAXF, "overlap"),           # out of order
    ([(0.0, fr(100))], [0.0], 100 * HOP, MAXF, "n_fft / 2"),                           # everything deleted: L = 0
    ([(fr(1), (2 * HOP + 100) / SR)], [0.0], 2 * HOP + 100, MAXF, "n_fft / 2"),         # L = 256 + 100 <= n_fft / 2
    ([(fr(10), fr(20))], None, 100 * HOP, 50, "position tables"),                      # N = 101 > max frames
])
def test_plan_edit_validation(parts, fix, S, maxf, match):
    with pytest.raises(ValueError, match=match):
        plan_edit(S, parts, fix, SR, HOP, NFFT, maxf)


def test_spans_that_touch_are_accepted():
    p = plan_edit(100 * HOP, [(fr(10), fr(20)), (fr(20), fr(30))], [fr(1), fr(2)], SR, HOP, NFFT, MAXF)
    assert p.gaps == ((10, 11), (11, 13)) and p.spliced_len == 83 * HOP


@pytest.fixture(scope="module")
def cpu_engine(tmp_path_factory):
    from vietvoice_tts_amd.core import ModelConfig, TTSEngine
    from oracle.vv_oracle import Oracle, OracleSession
    d = tmp_path_factory.mktemp("models")
    cfg = ModelConfig(model_cache_dir=str(d), synthetic_model=True, model_spec="tiny", nfe_step=4, max_chunk_duration=8.0)

    def factory(spec, weights, config):
        orc = Oracle(spec, weights, nfe_step=config.nfe_step)
        return {k: OracleSession(orc, k, seed=config.random_seed) for k in ("preprocess", "transformer", "decode")}
    eng = TTSEngine(cfg, session_factory=factory)
    yield eng
    eng.cleanup()


def test_edit_speech_needs_the_hip_engine(cpu_engine):
    clip = (np.sin(np.arange(24000) / 9.0) * 8000).astype(np.int16)
    with pytest.raises(RuntimeError, match="HIP engine"):
        cpu_engine.edit_speech(clip, "Xin chào các bạn.", [(0.2, 0.4)])
