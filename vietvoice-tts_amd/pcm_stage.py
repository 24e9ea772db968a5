"""The PCM stage of HipSynth (DESIGN §8 N10 ... N22, layering described there): per call a pure plan_* function of host values (every
ValueError, the row table, the derived sizes; no GPU needed) and a launch method of PcmStage, which HipSynth inherits."""
from typing import Optional

import torch

JOIN_MAX_N = 24576            # VV_JOIN_MAX_N of include/vvtts.h: the largest junction vv_join_chunks walks
LOUD_RUN = 128                # VV_LOUD_RUN of include/vvtts.h: samples per independent run of the K-weighting recurrence
_I64_MAX = (1 << 63) - 1
_FLAC_WIDTH = {8: 1, 16: 2, 24: 4}      # bytes per sample of the PCM a FLAC clip decodes to


def _ptr(t: Optional[torch.Tensor]) -> Optional[int]:
    return None if t is None else t.data_ptr()


# --------------------------------------------------------------------------- what every plan shares
def _int_rows(name: str, rows, widths, what: str, limit: Optional[int] = 65535):
    rows = [[int(v) for v in r] for r in rows]
    if not rows or any(len(r) not in widths for r in rows) or (limit is not None and len(rows) > limit):
        raise ValueError(f"{name}: {'rows' if limit is None else f'1 to {limit} rows'} of {what}")
    return rows


def _spans(name: str, spans, out_n: Optional[int] = None) -> int:
    """What the rows write: disjoint, and inside an ``out`` of out_n samples when one is given -> n_y, the samples the output needs."""
    spans.sort()
    if any(spans[i][0] < spans[i - 1][1] for i in range(1, len(spans))):
        raise ValueError(f"{name}: rows overlap on the output")
    n_y = max((e for _b, e in spans), default=0)
    if out_n is not None and out_n < n_y:
        raise ValueError(f"{name}: out holds {out_n} samples, {n_y} are needed")
    return n_y


def _per_request(name: str, v, R: int, what: str):
    v = list(v) if isinstance(v, (list, tuple)) else [v] * R
    if len(v) != R:
        raise ValueError(f"{name}: one {what}")
    return v


def _place(lens, align: int = 1):
    """The lengths one after another, each start on a multiple of ``align`` -> (offsets, the end of the last)."""
    offs, end = [], 0
    for n in lens:
        end = -(-end // align) * align
        offs.append(end)
        end += n
    return offs, end


def _out_arg(out, x: Optional[torch.Tensor] = None):
    """``out`` of a wrapper as its plan takes it -> (None = a new buffer, the sentinel string or the tensor's length; it is x itself)."""
    if out is None or isinstance(out, str):
        return out, False
    return out.numel(), x is not None and out.data_ptr() == x.data_ptr()


# --------------------------------------------------------------------------- the plans
def plan_join(requests, cross_fade_duration: float, sample_rate: int, align: int = 8, n_pcm: Optional[int] = None, out_n: Optional[int] = None,
              out_base: int = 0):
    """The host side of vv_join_chunks: every length is known here, so every junction size, position and final owner is too.
    requests = per request a list of chunks (src_off, len) in joining order.  Returns (chunk rows WITHOUT tab_off resolved: column 5 holds
    n, request rows, joined lengths, sorted distinct n, total output samples); request r's result starts at an ``align``-sample boundary
    behind ``out_base``; n_pcm / out_n (when given) are the lengths of the buffers the rows must fit.
    Mirrors AudioProcessor.concatenate_with_crossfade_improved: n = min(int(cross_fade_duration * sample_rate), joined so far, len(next));
    a request of one chunk is copied untouched; an empty chunk inside a longer request is refused (the reference raises on it in
    fix_clipped_audio), and so is an empty request."""
    cf = int(cross_fade_duration * sample_rate) if cross_fade_duration > 0 else 0
    rows, spans, lens = [], [], []
    for r, chunks in enumerate(requests):
        chunks = [(int(a), int(b)) for a, b in chunks]
        if not chunks:
            raise ValueError("join_chunks: a request without chunks")
        spans.append((len(rows), len(chunks)))
        if len(chunks) == 1:
            so, ln = chunks[0]
            if ln < 0:
                raise ValueError("join_chunks: negative chunk length")
            rows.append([so, ln, 0, 0, _I64_MAX, 0, 0, r])
            total = ln
        else:
            total, pos_n = 0, []
            for k, (so, ln) in enumerate(chunks):
                if ln <= 0:
                    raise ValueError("join_chunks: an empty chunk inside a request of two or more chunks")
                n = min(cf, total, ln) if k else 0
                if n > JOIN_MAX_N:
                    raise ValueError(f"join_chunks: a junction of {n} samples, more than {JOIN_MAX_N}")
                pos_n.append((total - n, n))
                total = total - n + ln
            fin, fins = _I64_MAX, []
            for P, _n in reversed(pos_n):          # fin_k = the smallest position of a later chunk
                fins.append(fin)
                fin = min(fin, P)
            fins.reverse()
            for (so, ln), (P, n), f in zip(chunks, pos_n, fins):
                rows.append([so, ln, P, n, f, n, 1, r])
        lens.append(total)
    if out_base < 0 or out_base % 8:
        raise ValueError("join_chunks: out_base must be a non-negative multiple of 8 samples")
    offs, total = _place(lens, align)
    if n_pcm is not None:
        for row in rows:
            if row[0] < 0 or row[0] + row[1] > n_pcm:
                raise ValueError(f"join_chunks: chunk ({row[0]}, {row[1]}) does not fit the {n_pcm} samples of pcm")
    if total + out_base >= 1 << 40 or len(rows) > 65535:
        raise ValueError("join_chunks: too many chunks or samples for one call")
    _spans("join_chunks", [(0, total + out_base)], out_n)
    reqs = [[c0, k, o + out_base, n] for (c0, k), o, n in zip(spans, offs, lens)]
    return rows, reqs, lens, sorted({row[3] for row in rows if row[3] > 0}), total


def _plan_copy(name: str, rows, what: str, col: int, n_x: int, n_y: Optional[int], skip: int = 0, down: int = 0):
    """Rows {src_off, n_in, dst_off, ...} that write r[col] outputs: inside both buffers, disjoint on the output -> (rows, n_y: None = what
    the rows need, the largest r[col])."""
    rows = _int_rows(name, rows, (what.count(",") + 1,), what, None)
    n_y = max(r[2] + r[col] for r in rows) if n_y is None else int(n_y)
    spans = [(r[2], r[2] + r[col]) for r in rows]
    for r, (do, end) in zip(rows, spans):
        if min(r) < 0 or r[0] + r[1] > n_x or end > n_y or (down and (r[4] + r[3] + skip) * down >= 1 << 62):
            raise ValueError(f"{name}: row {r} does not fit the buffers ({n_x} in, {n_y} out)")
    _spans(name, spans)
    return rows, n_y, max(r[col] for r in rows)


def plan_resample(rows, n_x: int, n_y: Optional[int], down: int, skip: int):
    return _plan_copy("pcm_resample", rows, "6 entries {src_off, n_in, dst_off, n_out, m0, i0}", 3, n_x, n_y, skip, down)


def plan_encode(rows, encoding: str, n_x: int, n_y: Optional[int]):
    kind = {"ulaw": 1, "alaw": 2}.get(encoding)
    if kind is None:
        raise ValueError("pcm_encode: encoding is 'ulaw' or 'alaw'")
    return (kind,) + _plan_copy("pcm_encode", rows, "3 entries {src_off, n, dst_off}", 1, n_x, n_y)


def plan_loudness(rows, sr: int, targets, peak_dbfs: float, n_x: int, out_n=None, in_place: bool = False):
    """-> (sub, rows with run_off, params {target, ceiling}, total runs, n_y); out_n, in_place: _out_arg."""
    from .core.audio_processor import check_loudness, loudness_ceiling, loudness_target
    sr = int(sr)
    if sr % 10 or sr // 10 < LOUD_RUN:
        raise ValueError(f"pcm_loudness: the sample rate must be a multiple of 10 Hz and at least {10 * LOUD_RUN} Hz, got {sr}")
    sub = sr // 10
    rows = _int_rows("pcm_loudness", rows, (3,), "3 entries {src_off, n, dst_off}")
    par = [check_loudness(t, peak_dbfs) for t in _per_request("pcm_loudness", targets, len(rows), "target per row")]
    par = [[loudness_target(t), loudness_ceiling(pk)] for t, pk in par]
    rps = -(-sub // LOUD_RUN)
    full, runs, spans = [], 0, []
    for so, n, do in rows:
        if min(so, n, do) < 0 or so + n > n_x:
            raise ValueError(f"pcm_loudness: row {[so, n, do]} does not fit the {n_x} samples of x")
        full.append([so, n, do, runs])
        runs += (n // sub) * rps + -(-(n % sub) // LOUD_RUN)
        spans.append((do, do + n))
    n_y = 0 if out_n == "measure" else _spans("pcm_loudness", spans, out_n)
    if in_place and any(r[0] != r[2] for r in rows):
        raise ValueError("pcm_loudness: in place needs dst_off == src_off")
    return sub, full, par, runs, n_y


def plan_limit(rows, sr: int, peak_dbfs: float, mode: str, gain, targets, has_meas: bool, L: Optional[int], tile, n_x: int, out_n=None,
               in_place: bool = False):
    """-> (L, mode index, 5-entry rows, params {target, ceiling, gain}, total samples, total tiles, n_y).  tile = L -> the limiter's tile for
    that look-ahead (vv_pcm_limit_tile); out_n, in_place: _out_arg."""
    from .core.audio_processor import LIMITER_MODES, _check_lookahead, check_limiter, check_loudness, limiter_lookahead, loudness_ceiling, loudness_target
    if check_limiter(mode) is None:
        raise ValueError("pcm_limit: a mode is needed")
    L = limiter_lookahead(sr) if L is None else _check_lookahead(L)
    rows = _int_rows("pcm_limit", rows, (3, 5), "3 entries {src_off, n, dst_off} or 5 {src_off, n, dst_off, out_lo, out_n}")
    rows = [r if len(r) == 5 else [r[0], r[1], r[2], 0, r[1]] for r in rows]
    targets, gains = (_per_request("pcm_limit", v, len(rows), "target and one gain per row") for v in (targets, gain))
    if not has_meas and any(t is not None for t in targets):
        raise ValueError("pcm_limit: a loudness target needs meas, the stats of a pcm_loudness measure call")
    c = loudness_ceiling(check_loudness(None, peak_dbfs)[1])
    par = []
    for t, g0 in zip(targets, gains):
        if isinstance(g0, bool) or not isinstance(g0, (int, float)) or not 0.0 < float(g0) < float("inf"):
            raise ValueError("pcm_limit: the gain must be a positive finite number")
        par.append([loudness_target(check_loudness(t, peak_dbfs)[0]), c, float(g0)])
    tile, samples, tiles, spans = tile(L), 0, 0, []
    for so, n, do, lo, on in rows:
        if min(so, n, do, lo, on) < 0 or so + n > n_x or lo + on > n:
            raise ValueError(f"pcm_limit: row {[so, n, do, lo, on]} does not fit the {n_x} samples of x or its own n")
        samples += n
        tiles += -(-n // tile)
        if on:
            spans.append((do, do + on))
    n_y = 0 if out_n == "measure" else _spans("pcm_limit", spans, out_n)
    if in_place and any(r[4] and r[2] != r[0] + r[3] for r in rows):
        raise ValueError("pcm_limit: in place needs dst_off == src_off + out_lo")
    return L, LIMITER_MODES.index(mode), rows, par, samples, tiles, n_y


def plan_stretch(rows, n_x: int, out_n=None, overlaps_x: bool = False):
    """-> (rows with pos_off, pos_offs, n_y); out_n: _out_arg; overlaps_x: out shares memory with x."""
    from .core.audio_processor import WSOLA_HS, check_stretch_ratio
    rows = _int_rows("pcm_stretch", rows, (5,), "5 entries {src_off, n, dst_off, p, q}")
    spans, full, pos_offs = [], [], [0]
    for so, n, do, p, q in rows:
        check_stretch_ratio(p, q)
        if min(so, n, do) < 0 or so + n > n_x or n > 1 << 30:
            raise ValueError(f"pcm_stretch: row {[so, n, do, p, q]} does not fit the {n_x} samples of x")
        n_s = -(-n * p // q)
        if n_s:
            spans.append((do, do + n_s))
        full.append([so, n, do, p, q, pos_offs[-1]])
        pos_offs.append(pos_offs[-1] + -(-n_s // WSOLA_HS) + 1)
    if overlaps_x and out_n != "positions":
        raise ValueError("pcm_stretch: out overlaps x (the stretch is not in place)")
    return full, pos_offs, 0 if out_n == "positions" else _spans("pcm_stretch", spans, out_n)


def plan_prosody(offs, lens, pitch, tempo):
    """The layout of finish_output's prosody step.  Every request gets its place in a new buffer, on 8-sample boundaries as in plan_join:
    a request with a stretch alone is stretched into it, one with a pitch is stretched into an intermediate region behind the results
    (from ``base`` on) and converted from there, one without prosody is copied sample for sample.  -> (new offsets, new lengths, base,
    buffer size, copies [(src, dst, n)], stretch rows, converts [(from the new buffer (src_off then counts from base), p_r, q_r, rows)])."""
    from .core.audio_processor import prosody_plan
    plans = [prosody_plan(n, p, t) for n, p, t in zip(lens, pitch, tempo)]
    new_lens = [n if pl is None else pl.n_f for n, pl in zip(lens, plans)]
    new_offs, end = _place(new_lens, 8)
    base = -(-end // 8) * 8
    two = [i for i, pl in enumerate(plans) if pl is not None and pl.p != pl.q and pl.p_r != pl.q_r]     # stretched, then converted
    mid_offs, size = _place([base] + [plans[i].n_s for i in two], 8)
    mid = dict(zip(two, mid_offs[1:]))
    copies, stretch, convert = [], [], {}
    for i, pl in enumerate(plans):
        if pl is None:
            copies.append((offs[i], new_offs[i], lens[i]))
            continue
        if pl.p != pl.q:
            stretch.append([offs[i], lens[i], mid.get(i, new_offs[i]), pl.p, pl.q])
        if pl.p_r != pl.q_r and pl.n_f > 0:       # from the stretched signal, or straight from the joined one when tempo == pitch ratio
            src = [mid[i] - base, pl.n_s] if i in mid else [offs[i], lens[i]]
            convert.setdefault((pl.p_r, pl.q_r, i not in mid), []).append(src + [new_offs[i], pl.n_f, 0, 0])
    converts = [(not joined, p_r, q_r, rows) for (p_r, q_r, joined), rows in sorted(convert.items())]
    return new_offs, new_lens, base, max(-(-size // 8) * 8, 8), copies, stretch, converts


def plan_formant(rows, n_x: int, n_y: int, out_n: Optional[int] = None, overlaps: bool = False):
    """vv_pcm_formant's rows {x_off, n, y_off, n_f, z_off, tn, td}, validated -> (rows, frame offsets [R + 1]: request r's frames 0 ... M
    are frame_offs[r] ... frame_offs[r + 1] - 1, n_z); out_n: _out_arg; overlaps: out shares memory with x or y."""
    from .core.audio_processor import FORMANT_H, WSOLA_MAX_PQ
    rows = _int_rows("pcm_formant", rows, (7,), "7 entries {x_off, n, y_off, n_f, z_off, tn, td}")
    spans, frame_offs = [], [0]
    for r in rows:
        xo, n, yo, n_f, zo, tn, td = r
        if not (1 <= tn <= WSOLA_MAX_PQ and 1 <= td <= WSOLA_MAX_PQ):
            raise ValueError(f"pcm_formant: row {r}: tn and td in 1 ... {WSOLA_MAX_PQ}")
        if min(xo, n, yo, n_f, zo) < 0 or xo + n > n_x or yo + n_f > n_y or n > 1 << 30:
            raise ValueError(f"pcm_formant: row {r} does not fit the buffers ({n_x} samples of x, {n_y} of y)")
        if n_f != -(-n * td // tn):
            raise ValueError(f"pcm_formant: row {r}: n_f is not ceil(n td / tn) = {-(-n * td // tn)}")
        if n_f:
            spans.append((zo, zo + n_f))
        frame_offs.append(frame_offs[-1] + -(-n_f // FORMANT_H) + 1)
    if overlaps:
        raise ValueError("pcm_formant: out overlaps x or y (the filter is not in place)")
    return rows, frame_offs, _spans("pcm_formant", spans, out_n)


def plan_keep(plans, offs, lens, new_offs, new_lens, formants):
    """The requests of a prosody step that ask for formants = "keep" and have a pitch: -> their vv_pcm_formant rows, z_off = y_off (the
    result takes the place of the converted signal in a buffer of the same layout).  plans = prosody_plan per request."""
    from .core.audio_processor import prosody_tempo
    rows = []
    for i, pl in enumerate(plans):
        if formants[i] == "keep" and pl is not None and pl.p_r != pl.q_r and pl.n_f > 0:
            rows.append([offs[i], lens[i], new_offs[i], new_lens[i], new_offs[i], *prosody_tempo(pl)])
    return rows


def plan_denoise(rows, strengths, n_x: int, n_bias: int, out_n: Optional[int] = None, overlaps: bool = False):
    """vv_pcm_denoise's rows {x_off, n, y_off, bias_row} and one strength per row (or one for all), validated -> (rows, strengths as floats,
    frame offsets [R + 1]: request r's frames 0 ... M + 2 are frame_offs[r] ... frame_offs[r + 1] - 1, n_y); out_n: _out_arg; overlaps: out
    shares memory with x."""
    import math
    from .core.audio_processor import DENOISE_H, DENOISE_MAX_STRENGTH
    rows = _int_rows("pcm_denoise", rows, (4,), "4 entries {x_off, n, y_off, bias_row}")
    strengths = _per_request("pcm_denoise", strengths, len(rows), "strength per row")
    spans, frame_offs, out_s = [], [0], []
    for r, s in zip(rows, strengths):
        xo, n, yo, b = r
        if isinstance(s, bool) or not isinstance(s, (int, float)) or not math.isfinite(s) or not 0.0 <= s <= DENOISE_MAX_STRENGTH:
            raise ValueError(f"pcm_denoise: row {r}: the strength is a finite number in 0 ... {DENOISE_MAX_STRENGTH:g}")
        if min(xo, n, yo, b) < 0 or xo + n > n_x or n > 1 << 30:
            raise ValueError(f"pcm_denoise: row {r} does not fit the buffers ({n_x} samples of x)")
        if b >= n_bias:
            raise ValueError(f"pcm_denoise: row {r}: bias_row outside the {n_bias} rows of bias")
        if n:
            spans.append((yo, yo + n))
        out_s.append(float(s))
        frame_offs.append(frame_offs[-1] + -(-n // DENOISE_H) + 3)
    if overlaps:
        raise ValueError("pcm_denoise: out overlaps x (a hop reads the input under its neighbours: not in place)")
    return rows, out_s, frame_offs, _spans("pcm_denoise", spans, out_n)


def plan_denoise_bias(rows, n_x: int):
    """vv_pcm_denoise_bias's rows {x_off, n, 0, 0}, or {x_off, n}, validated -> (4-entry rows, the sum of the full frames)."""
    from .core.audio_processor import DENOISE_BIAS_MAX_N, DENOISE_H, DENOISE_N
    rows = [r + [0] * (4 - len(r)) for r in _int_rows("pcm_denoise_bias", rows, (2, 4), "2 entries {x_off, n} or 4 {x_off, n, 0, 0}")]
    frames = 0
    for r in rows:
        if min(r) < 0 or not DENOISE_N <= r[1] <= DENOISE_BIAS_MAX_N or r[0] + r[1] > n_x:
            raise ValueError(f"pcm_denoise_bias: row {r}: a signal of {DENOISE_N} ... {DENOISE_BIAS_MAX_N} samples inside the {n_x} samples of x is "
                             f"needed (one full frame)")
        frames += (r[1] - DENOISE_N) // DENOISE_H + 1
    return rows, frames


def plan_finish_denoise(R: int, denoise=None):
    """finish_output's ``denoise``: one strength for every request or a per-request list with None entries -> the list, or None when no
    request has one (nothing new is then called)."""
    from .core.audio_processor import check_denoise
    if denoise is None:
        return None
    vals = [check_denoise(v) for v in _per_request("finish_output", denoise, R, "denoise entry per request")]
    return None if all(v is None for v in vals) else vals


def plan_watermark(rows, payloads, strength, n_x: int, out_n: Optional[int] = None, overlaps: bool = False):
    """vv_pcm_watermark's rows {x_off, n, y_off} and one payload per row (or one for all), validated -> (4-entry rows {x_off, n, y_off,
    message}, gp = 1.0 + a, gm = 1.0 - a, n_y); strength a in 0 ... 0.5 (0 gives the input back); out_n: _out_arg; overlaps: out shares
    memory with x."""
    from .core.audio_processor import check_watermark_strength, watermark_message
    rows = _int_rows("pcm_watermark", rows, (3,), "3 entries {x_off, n, y_off}")
    payloads = _per_request("pcm_watermark", payloads, len(rows), "payload per row")
    a = check_watermark_strength(strength, zero=True)
    spans, full = [], []
    for r, p in zip(rows, payloads):
        xo, n, yo = r
        if min(xo, n, yo) < 0 or xo + n > n_x or n > 1 << 30:
            raise ValueError(f"pcm_watermark: row {r} does not fit the buffers ({n_x} samples of x)")
        if n:
            spans.append((yo, yo + n))
        full.append([xo, n, yo, watermark_message(p)])
    if overlaps:
        raise ValueError("pcm_watermark: out overlaps x (a hop reads the input under its neighbours: not in place)")
    return full, 1.0 + a, 1.0 - a, _spans("pcm_watermark", spans, out_n)


def plan_watermark_detect(rows, n_x: int):
    """vv_pcm_watermark_detect's rows {x_off, n}, or {x_off, n, 0, 0}, validated -> (4-entry rows, frame offsets [R + 1]: request r's frames
    0 ... M + 2 are frame_offs[r] ... frame_offs[r + 1] - 1)."""
    from .core.audio_processor import DENOISE_H, WATERMARK_DETECT_MAX_N
    rows = [r + [0] * (4 - len(r)) for r in _int_rows("pcm_watermark_detect", rows, (2, 4), "2 entries {x_off, n} or 4 {x_off, n, 0, 0}")]
    frame_offs = [0]
    for r in rows:
        if min(r) < 0 or r[1] > WATERMARK_DETECT_MAX_N or r[0] + r[1] > n_x:
            raise ValueError(f"pcm_watermark_detect: row {r}: a signal of at most {WATERMARK_DETECT_MAX_N} samples inside the {n_x} samples of x "
                             f"is needed")
        frame_offs.append(frame_offs[-1] + -(-r[1] // DENOISE_H) + 3)
    return rows, frame_offs


def plan_finish_watermark(R: int, watermark=None, key=None, strength=0.2):
    """finish_output's ``watermark``: one payload for every request or a per-request list with None entries -> (key, the list, strength), or
    None when no request has one (nothing new is then called).  A payload without a key is refused."""
    from .core.audio_processor import check_watermark_key, check_watermark_payload, check_watermark_strength
    if watermark is None:
        return None
    vals = [check_watermark_payload(v) for v in _per_request("finish_output", watermark, R, "watermark entry per request")]
    if all(v is None for v in vals):
        return None
    key = check_watermark_key(key)
    if key is None:
        raise ValueError("finish_output: a watermark payload needs watermark_key")
    return key, vals, check_watermark_strength(strength)


def plan_flac(rows, n_x: int, sample_rate, lpc_order: int = 0):
    """vv_pcm_flac's rows (src_off, n, frame0, last) -> (lpc_order, rows, the sum of the frame bounds = n_y, frames)."""
    from .core.audio_processor import FLAC_BLOCK, FLAC_MAX_RATE, check_flac_lpc_order, flac_frame_bound
    lpc_order = check_flac_lpc_order(lpc_order)
    rows = _int_rows("pcm_flac", rows, (4,), "4 entries {src_off, n, frame0, last}")
    if isinstance(sample_rate, bool) or int(sample_rate) != sample_rate or not 1 <= int(sample_rate) <= FLAC_MAX_RATE:
        raise ValueError(f"pcm_flac: a sample rate in 1 ... {FLAC_MAX_RATE} Hz is needed")
    n_y, frames = 0, 0
    for so, n, f0, last in rows:
        nf = -(-n // FLAC_BLOCK)
        if so < 0 or n < 1 or so + n > n_x or f0 < 0 or f0 + nf > 1 << 31 or last not in (0, 1) or (not last and n % FLAC_BLOCK):
            raise ValueError(f"pcm_flac: row {[so, n, f0, last]} does not fit the {n_x} samples of x, the frame numbers below 2^31 or "
                             f"whole frames of {FLAC_BLOCK} samples where last = 0")
        n_y += (nf - 1) * flac_frame_bound(FLAC_BLOCK) + flac_frame_bound(n - (nf - 1) * FLAC_BLOCK)
        frames += nf
    return lpc_order, rows, n_y, frames


def plan_flac_index(rows, n_bytes: int, aligned: bool = True):
    """vv_flac_index's rows {byte offset, n_bytes, channels, bits, min block, max block, rate, total}, validated; aligned: data is, to 8 bytes."""
    from .core.audio_processor import FLAC_MAX_CLIP
    if not 8 <= n_bytes <= (1 << 31) - 64 or not aligned:
        raise ValueError("flac_index: 8 ... 2^31 - 64 bytes of data, 8-byte aligned")
    rows = _int_rows("flac_index", rows, (8,), "8 entries {byte offset, n_bytes, channels, bits, min block, max block, rate, total}")
    at = 0
    for r in rows:
        off, n, ch, bits, lo, hi, rate, total = r
        if (off < at or off % 4 or n < 0 or off + n + 8 > n_bytes or not 1 <= ch <= 8 or bits not in (8, 16, 24) or not 16 <= hi <= 65535
                or not 0 <= lo <= hi or not 1 <= rate <= 1048575 or not 0 <= total <= FLAC_MAX_CLIP):
            raise ValueError(f"flac_index: row {r} does not fit the {n_bytes} bytes of data (ascending, 4-byte aligned, 8 bytes of padding behind "
                             f"the last clip) or the decoder's limits")
        at = off + n
    return rows


def plan_flac_decode(lay, clips, n_pcm: int):
    """vv_flac_decode's rows {pcm byte offset, frames, samples} per clip of flac_index's rows -> (rows with the prefix sums, frames, plane samples)."""
    lay = [[int(v) for v in r] for r in lay]
    if len(lay) != len(clips) or any(len(r) != 3 for r in lay):
        raise ValueError("flac_decode: one row {pcm byte offset, frames, samples} per clip")
    full, F, S, P, at = [], 0, 0, 0, 0
    for (off, frames, samples), row in zip(lay, clips):
        nbytes = samples * row[2] * _FLAC_WIDTH[row[3]]
        if off < at or frames < 0 or samples < frames or off + nbytes > n_pcm:
            raise ValueError(f"flac_decode: row {[off, frames, samples]} does not fit the {n_pcm} bytes of pcm, in ascending order")
        full.append([off, frames, samples, F, P, S])
        at, F, S, P = off + nbytes, F + frames, S + samples, P + samples * row[2]
    return full, F, P


def plan_adpcm(rows, n_x: int, samples_per_block, n_y: Optional[int] = None):
    """vv_pcm_adpcm's rows (src_off, n, dst_off in bytes), ascending and disjoint on y -> (samples_per_block, rows, n_y: None = what the
    rows need, the largest number of blocks of a row)."""
    from .core.audio_processor import check_adpcm_block
    spb = check_adpcm_block(samples_per_block)
    ba = (spb - 1) // 2 + 4
    rows = _int_rows("pcm_adpcm", rows, (3,), "3 entries {src_off, n, dst_off}")
    at, most = 0, 0
    for so, n, do in rows:
        blocks = -(-n // spb)
        if so < 0 or n < 1 or so + n > n_x or do < at or do % 4:
            raise ValueError(f"pcm_adpcm: row {[so, n, do]} does not fit the {n_x} samples of x (n >= 1), or its blocks do not lie in ascending "
                             f"order on y at a multiple of 4 bytes")
        at, most = do + blocks * ba, max(most, blocks)
    if n_y is not None and at > n_y:
        raise ValueError(f"pcm_adpcm: y holds {n_y} bytes, {at} are needed")
    return spb, rows, at if n_y is None else int(n_y), most


def plan_wav_decode(rows, n_bytes: int, n_pcm: int):
    """vv_wav_decode's rows {data byte offset, n_bytes, tag, channels, block align, frames, pcm byte offset}, validated -> 8-entry rows."""
    from .core.audio_processor import ADPCM_WAVE_TAG, adpcm_frame_count
    rows = _int_rows("wav_decode", rows, (7,), "7 entries {data byte offset, n_bytes, tag, channels, block align, frames, pcm byte offset}")
    at = 0
    for r in rows:
        off, n, tag, ch, ba, frames, po = r
        if off < 0 or off % 16 or n < 0 or off + n > n_bytes or not 1 <= ch <= 65535 or frames < 0:
            raise ValueError(f"wav_decode: row {r} does not fit the {n_bytes} bytes of data (16-byte aligned clips)")
        if tag == ADPCM_WAVE_TAG:
            if ch > 2 or ba < 8 * ch or ba % (4 * ch) or ba > 65535:
                raise ValueError(f"wav_decode: row {r}: IMA ADPCM has 1 or 2 channels and a block alignment that is a multiple of 4 x channels")
            holds = adpcm_frame_count(n, ch, ba)
        elif tag in (6, 7):
            holds = n // ch
        else:
            raise ValueError(f"wav_decode: row {r}: format tag 6, 7 or 17")
        if frames > holds or po < at or po % 16 or po + frames * ch * 2 > n_pcm:
            raise ValueError(f"wav_decode: row {r}: {frames} frames do not fit its bytes ({holds}) or the {n_pcm} bytes of pcm (16-byte aligned, ascending)")
        at = po + frames * ch * 2
    return [r + [0] for r in rows]


def plan_finish(R: int, loudness=None, limiter=None, pitch=None, tempo=None):
    """finish_output's options, each one value or one per request, normalised once -> (pitch list, tempo list: both None when no request
    has either; groups [(limiter mode or None, requests, their loudness targets)] in calling order: None = one pcm_loudness call)."""
    from .core.audio_processor import LIMITER_MODES, check_limiter
    if loudness is None and limiter is None and pitch is None and tempo is None:       # the plain output: nothing beyond the join is called
        return None, None, []
    pitch, tempo = (_per_request("finish_output", v, R, "pitch and one tempo entry per request") for v in (pitch, tempo))
    if all(v is None for v in pitch + tempo):
        pitch = tempo = None
    louds = _per_request("finish_output", loudness, R, "loudness entry per request")
    lims = _per_request("finish_output", limiter, R, "limiter entry per request")
    by_mode = {}
    for i, (mode, target) in enumerate(zip(lims, louds)):
        if mode is not None or target is not None:
            by_mode.setdefault(check_limiter(mode), []).append(i)
    groups = [(mode, by_mode[mode], [louds[i] for i in by_mode[mode]]) for mode in (None,) + tuple(LIMITER_MODES) if mode in by_mode]
    return pitch, tempo, groups


# --------------------------------------------------------------------------- the launches
class PcmStage:
    """HipSynth's PCM stage: what the methods below need of it is lib, ctx, device, _lock, _check and _stream (and vocoder_bias, where
    finish_output is asked to denoise against the model's own profile)."""

    def __init__(self):
        self._tables = {"fade": {"off": {}, "host": [], "dev": None, "size": 0}}      # the constant device tables; "fade" grows (_fade_tables)

    def _table(self, key, make, *args):
        """make(*args) (a callable, or the name of one in core.audio_processor) as this device keeps it under ``key``: numpy tables go up."""
        if key not in self._tables:
            import numpy as np
            from .core import audio_processor
            up = lambda v: torch.from_numpy(v.copy()).to(self.device) if isinstance(v, np.ndarray) else v  # noqa: E731
            made = (getattr(audio_processor, make) if isinstance(make, str) else make)(*args)
            self._tables[key] = tuple(up(v) for v in made) if isinstance(made, tuple) else up(made)
        return self._tables[key]

    def _upload(self, rows, dtype=torch.int64):
        """A table of equally long rows -> (its device copy, its host copy), the order in which the entries take the two."""
        h = torch.tensor(rows, dtype=dtype)
        return h.to(self.device), h

    def _ws(self, nbytes: int) -> torch.Tensor:
        return torch.empty((int(nbytes) // 8 + 1,), dtype=torch.int64, device=self.device)

    def _out(self, out, n_y: int, dtype=torch.int16, floor: int = 4):
        """``out`` of a wrapper -> the tensor to write, or None for a sentinel string; its length was the plan's to check."""
        if isinstance(out, str):
            return None
        if out is None:
            return torch.empty((max(n_y, floor),), dtype=dtype, device=self.device)
        assert out.is_cuda and out.dtype == dtype and out.is_contiguous() and out.dim() == 1
        return out

    def _call(self, fn, *args):
        """One library call on the caller's stream, under the engine lock; a non-zero status raises."""
        with self._lock, torch.cuda.device(self.device):
            self._check(fn(self.ctx, *args, self._stream()))

    # ------------------------------------------------------------------ the output stage (N10): join, output rate, G.711
    def _fade_tables(self, ns):
        """c = cos(linspace(0, pi / 2, n)) ** 2 | s = sin(..) ** 2 per distinct n, computed by numpy on the HOST (the expression of the
        reference's mix) and kept in one float64 device buffer: -> (buffer, {n: offset in doubles})."""
        import numpy as np
        cache = self._tables["fade"]
        new = [n for n in ns if n not in cache["off"]]
        if new:
            if cache["size"] + 2 * sum(new) > (1 << 22):       # 32 MB of tables: start over
                cache.update(off={}, host=[], dev=None, size=0)
                new = list(ns)
            for n in new:
                theta = np.linspace(0, np.pi / 2, n)
                cache["off"][n] = cache["size"]
                cache["host"] += [np.cos(theta) ** 2, np.sin(theta) ** 2]
                cache["size"] += 2 * n
            cache["dev"] = torch.from_numpy(np.concatenate(cache["host"])).to(self.device)
        if cache["dev"] is None:
            cache["dev"] = torch.zeros(2, dtype=torch.float64, device=self.device)
        return cache["dev"], cache["off"]

    def join_chunks(self, pcm: torch.Tensor, requests, cross_fade_duration: float, sample_rate: int, out: Optional[torch.Tensor] = None,
                    out_base: int = 0):
        """AudioProcessor.concatenate_with_crossfade_improved for R requests in one call (vv_join_chunks), bit for bit.
        pcm int16 on the device (vv_decode's plane, taken flat); requests = per request the (src_off, len) spans of its chunks in joining
        order.  -> (out int16 flat, offsets, lengths): request r is out[offsets[r] : offsets[r] + lengths[r]].  out (optional) = an
        existing flat int16 buffer, the results then start out_base samples into it (out_base % 8 == 0).  The rows are planned and
        validated here, on the host, before anything is launched; the call never synchronises."""
        assert pcm.is_cuda and pcm.dtype == torch.int16 and pcm.is_contiguous()
        n_pcm = pcm.numel()
        rows, reqs, lens, ns, total = plan_join(requests, cross_fade_duration, sample_rate, n_pcm=n_pcm, out_n=_out_arg(out)[0], out_base=out_base)
        out = self._out(out, total + out_base, floor=8)
        fade, off = self._fade_tables(ns)
        for row in rows:
            row[5] = off[row[3]] if row[3] > 0 else 0
        (rows_d, rows_h), (reqs_d, reqs_h) = self._upload(rows), self._upload(reqs)
        ws = torch.empty((2 * len(rows),), dtype=torch.int32, device=self.device)
        self._call(self.lib.vv_join_chunks, pcm.data_ptr(), n_pcm, rows_d.data_ptr(), rows_h.data_ptr(), len(rows), reqs_d.data_ptr(), reqs_h.data_ptr(),
                   len(reqs), fade.data_ptr(), fade.numel(), max(ns, default=0), max(r[1] for r in rows), out.data_ptr(), out.numel(), ws.data_ptr())
        return out, [rq[2] for rq in reqs], lens

    def _output_taps(self, src: int, dst: int):
        return self._table(("taps", src, dst), "output_design", src, dst)

    def pcm_resample(self, x: torch.Tensor, rows, src: int, dst: int, n_y: Optional[int] = None, out: Optional[torch.Tensor] = None) -> torch.Tensor:
        """Output rate (vv_pcm_resample): x int16 flat on the device at ``src`` Hz, rows = HOST rows {src_off, n_in, dst_off, n_out, m0, i0}
        (include/vvtts.h) -> int16 [n_y] at ``dst`` Hz through voice_bank.resample_design(src, dst).  A whole clip is m0 = i0 = 0 and
        n_out = ceil(n_in * up / down).  The rows are validated here (in range of both buffers, disjoint on the output).
        out (optional) = an existing flat int16 device buffer to write into (n_y = its length); what the rows read must not be written."""
        assert x.is_cuda and x.dtype == torch.int16 and x.is_contiguous()
        if int(src) == int(dst):
            raise ValueError("pcm_resample: equal rates need no launch")
        taps, up, down, skip = self._output_taps(int(src), int(dst))
        rows, n_y, max_out = plan_resample(rows, x.numel(), n_y if out is None else out.numel(), down, skip)
        y = self._out(out, n_y, floor=1)
        d = self._upload(rows)[0]
        self._call(self.lib.vv_pcm_resample, x.data_ptr(), x.numel(), d.data_ptr(), len(rows), max_out, taps.data_ptr(), taps.numel(), up, down, skip,
                   y.data_ptr(), n_y)
        return y[:n_y]

    def pcm_encode(self, x: torch.Tensor, rows, encoding: str, n_y: Optional[int] = None) -> torch.Tensor:
        """G.711 (vv_pcm_encode): x int16 flat on the device, rows = HOST rows {src_off, n, dst_off} -> uint8 [n_y]; encoding "ulaw" | "alaw",
        bit-exact to audioop.lin2ulaw / lin2alaw at width 2.  The rows are validated here."""
        assert x.is_cuda and x.dtype == torch.int16 and x.is_contiguous()
        kind, rows, n_y, max_n = plan_encode(rows, encoding, x.numel(), n_y)
        y = self._out(None, n_y, torch.uint8, floor=8)
        d = self._upload(rows)[0]
        self._call(self.lib.vv_pcm_encode, x.data_ptr(), x.numel(), d.data_ptr(), len(rows), max_n, kind, y.data_ptr(), n_y)
        return y[:n_y]

    # ------------------------------------------------------------------ loudness normalisation (N12)
    def _loudness_tables(self, sr: int) -> torch.Tensor:
        return self._table(("loudness", int(sr)), "loudness_tables", int(sr))

    def pcm_loudness(self, x: torch.Tensor, rows, sr: int, targets, peak_dbfs: float = -1.0, out: Optional[torch.Tensor] = None,
                     stats: bool = False):
        """Loudness normalisation of R joined signals in one call (vv_pcm_loudness), bit for bit
        core.audio_processor.normalize_loudness.  x int16 flat on the device at ``sr`` Hz; rows = HOST rows (src_off, n, dst_off);
        targets = one LUFS value, or per request a value or None (None = measured, copied through unchanged); peak_dbfs = the sample-peak
        ceiling.  out = None: a new buffer; out = "measure": nothing is written; out = a flat int16 device tensor (x itself with
        dst_off == src_off = in place).  -> the output (None when measuring), and with ``stats`` also the R x 4 float64 DEVICE tensor
        {zbar, kept, P, g}.  The rows are validated here; the call never synchronises."""
        assert x.is_cuda and x.dtype == torch.int16 and x.is_contiguous() and x.dim() == 1
        sub, rows, par, runs, n_y = plan_loudness(rows, sr, targets, peak_dbfs, x.numel(), *_out_arg(out, x))
        y, R = self._out(out, n_y), len(rows)
        (rows_d, rows_h), par_d = self._upload(rows), self._upload(par, torch.float64)[0]
        st = torch.empty((R, 4), dtype=torch.float64, device=self.device)
        ws = self._ws(self.lib.vv_pcm_loudness_ws_bytes(runs, R))
        self._call(self.lib.vv_pcm_loudness, x.data_ptr(), x.numel(), rows_d.data_ptr(), rows_h.data_ptr(), R, sub, self._loudness_tables(sr).data_ptr(),
                   par_d.data_ptr(), _ptr(y), 0 if y is None else y.numel(), st.data_ptr(), ws.data_ptr(), ws.numel() * 8)
        return (y, st) if stats else y

    # ------------------------------------------------------------------ look-ahead peak limiter (N13)
    def _limiter_tables(self, L: int):
        """(window, taps, tile) for a look-ahead: the host's float64 tables on the device, cached per L."""
        make = lambda L: (self._table(("window", L), "limiter_window", L), self._table("taps", "limiter_taps"), int(self.lib.vv_pcm_limit_tile(L)))  # noqa: E731
        return self._table(("limiter", int(L)), make, int(L))

    def pcm_limit(self, x: torch.Tensor, rows, sr: int, peak_dbfs: float = -1.0, mode: str = "true", gain=1.0, meas: Optional[torch.Tensor] = None,
                  targets=None, L: Optional[int] = None, out=None, stats: bool = False):
        """The look-ahead limiter on R joined signals in one call (vv_pcm_limit), bit for bit
        core.audio_processor.limit_peaks.  x int16 flat on the device at ``sr`` Hz; rows = HOST rows (src_off, n, dst_off) or
        (src_off, n, dst_off, out_lo, out_n): the limiter runs over the row's n samples as a whole signal and y[out_lo, +out_n) of it is
        written at dst_off.  mode "sample" | "true"; peak_dbfs = the ceiling; gain = the pre-gain (one value or one per row).
        meas = the R x 4 device tensor of a pcm_loudness(out="measure", stats=True) call on the same rows, with targets = one LUFS value
        or per row a value or None: rows with a target take the uncapped loudness gain from meas on the device, the others ``gain``.
        L = the look-ahead in samples (None = 5 ms).  out = None: a new buffer; "measure": nothing is written; a flat int16 device tensor
        (x itself with dst_off == src_off + out_lo = in place).  -> the output (None when measuring), and with ``stats`` also the R x 4
        float64 DEVICE tensor {g, e_max, s_min, n_limited}.  The rows are validated here; the call never synchronises."""
        assert x.is_cuda and x.dtype == torch.int16 and x.is_contiguous() and x.dim() == 1
        L, mode, rows, par, samples, tiles, n_y = plan_limit(rows, sr, peak_dbfs, mode, gain, targets, meas is not None, L,
                                                             lambda L: self._limiter_tables(L)[2], x.numel(), *_out_arg(out, x))
        y, R = self._out(out, n_y), len(rows)
        assert meas is None or (meas.is_cuda and meas.dtype == torch.float64 and meas.is_contiguous() and tuple(meas.shape) == (R, 4))
        window, taps, _tile = self._limiter_tables(L)
        (rows_d, rows_h), par_d = self._upload(rows), self._upload(par, torch.float64)[0]
        st = torch.empty((R, 4), dtype=torch.float64, device=self.device)
        ws = self._ws(self.lib.vv_pcm_limit_ws_bytes(samples, tiles, R))
        self._call(self.lib.vv_pcm_limit, x.data_ptr(), x.numel(), rows_d.data_ptr(), rows_h.data_ptr(), R, L, mode, window.data_ptr(), taps.data_ptr(),
                   par_d.data_ptr(), _ptr(meas), _ptr(y), 0 if y is None else y.numel(), st.data_ptr(), ws.data_ptr(), ws.numel() * 8)
        return (y, st) if stats else y

    def limiter_stream_backend(self, sr: int, peak_dbfs: float = -1.0, mode: str = "true", L: Optional[int] = None):
        """The ``backend(hist, out_lo, out_n)`` callable of core.audio_processor.LimiterStream on this device: the block and its context go
        up, vv_pcm_limit runs over them as one signal and writes the window alone, which comes back."""
        import numpy as np

        def backend(hist, out_lo, out_n):
            hist = np.ascontiguousarray(hist, dtype=np.int16).reshape(-1)
            if out_n <= 0:
                return np.zeros(0, np.int16)
            y = self.pcm_limit(torch.from_numpy(hist).to(self.device), [[0, hist.size, 0, int(out_lo), int(out_n)]], sr, peak_dbfs, mode, L=L)
            return y[: int(out_n)].cpu().numpy()

        return backend

    # ------------------------------------------------------------------ pitch and tempo (N14)
    @property
    def _wsola_window(self) -> torch.Tensor:
        return self._table("wsola", "wsola_window")

    def pcm_stretch(self, x: torch.Tensor, rows, out: Optional[torch.Tensor] = None):
        """The WSOLA time stretch on R joined signals in one call (vv_pcm_stretch), bit for bit
        core.audio_processor.time_stretch.  x int16 flat on the device; rows = HOST rows (src_off, n, dst_off, p, q): x[src_off, +n) is
        stretched by p / q to ceil(n p / q) samples at dst_off.  out = None: a new buffer; "positions": the search alone, no sample is
        written and y is None; or a flat int16 device tensor that does not overlap x.  -> (y, pos, pos_offs): pos is the int32 device tensor of every frame position, request r's pos_0 ... pos_M are
        pos[pos_offs[r] : pos_offs[r + 1]].  The rows are validated here; the call never synchronises."""
        assert x.is_cuda and x.dtype == torch.int16 and x.is_contiguous() and x.dim() == 1
        n_x = x.numel()
        shared = isinstance(out, torch.Tensor) and out.data_ptr() < x.data_ptr() + 2 * n_x and x.data_ptr() < out.data_ptr() + 2 * out.numel()
        rows, pos_offs, n_y = plan_stretch(rows, n_x, _out_arg(out)[0], shared)
        y, R = self._out(out, n_y), len(rows)
        rows_d, rows_h = self._upload(rows)
        pos = torch.empty((pos_offs[-1],), dtype=torch.int32, device=self.device)
        ws = self._ws(self.lib.vv_pcm_stretch_ws_bytes(R))
        self._call(self.lib.vv_pcm_stretch, x.data_ptr(), n_x, rows_d.data_ptr(), rows_h.data_ptr(), R, self._wsola_window.data_ptr(), _ptr(y),
                   0 if y is None else y.numel(), pos.data_ptr(), pos.numel(), ws.data_ptr(), ws.numel() * 8)
        return y, pos, pos_offs

    def _prosody(self, buf: torch.Tensor, offs, lens, pitch, tempo, formants=None):
        """The prosody step of finish_output after plan_prosody: -> (new buffer, offsets, lengths).  formants = per request "shift" |
        "keep" (N18; None = "shift" everywhere, nothing new is called): the converted signal of a request with "keep" and a pitch goes
        through pcm_formant, against its joined signal in ``buf``, into a second buffer of the same layout."""
        new_offs, new_lens, base, size, copies, stretch, converts = plan_prosody(offs, lens, pitch, tempo)
        new = torch.empty((size,), dtype=torch.int16, device=self.device)
        for src, dst, n in copies:
            new[dst: dst + n].copy_(buf[src: src + n])
        if stretch:
            self.pcm_stretch(buf, stretch, out=new)
        for from_new, p_r, q_r, rows in converts:          # source and destination are separate parts of ``new``
            self.pcm_resample(new[base:] if from_new else buf, rows, p_r, q_r, out=new[:base])
        out = new[:max(base, 8)]
        if formants is not None and "keep" in formants:
            from .core.audio_processor import prosody_plan
            keep = plan_keep([prosody_plan(n, p, t) for n, p, t in zip(lens, pitch, tempo)], offs, lens, new_offs, new_lens, formants)
            if keep:
                kept = out.clone()                          # the others stay as they are; z overlaps neither x nor y
                self.pcm_formant(buf, out, keep, out=kept)
                out = kept
        return out, new_offs, new_lens

    # ------------------------------------------------------------------ formant-preserving pitch shift (N18)
    @property
    def _formant_tables(self):
        return self._table("formant", "formant_tables")

    def pcm_formant(self, x: torch.Tensor, y: torch.Tensor, rows, out: Optional[torch.Tensor] = None, taps: bool = False):
        """The envelope correction of a pitch shift on R requests in one call (vv_pcm_formant), bit for bit
        core.audio_processor.keep_formants.  x int16 flat on the device: the joined signals; y int16 flat: what the prosody step made of
        them; rows = HOST rows (x_off, n, y_off, n_f, z_off, tn, td): tn / td the tempo fraction, n_f = ceil(n td / tn).  out = None: a new
        buffer, or a flat int16 device tensor that overlaps neither x nor y.  -> z, or with ``taps`` (z, h, frame_offs): h the float64
        device tensor [frames][L] of every frame's filter, request r's frames h[frame_offs[r] : frame_offs[r + 1]].  The rows are
        validated here; the call never synchronises."""
        for t in (x, y):
            assert t.is_cuda and t.dtype == torch.int16 and t.is_contiguous() and t.dim() == 1
        n_x, n_y = x.numel(), y.numel()
        shared = isinstance(out, torch.Tensor) and any(out.data_ptr() < t.data_ptr() + 2 * t.numel() and t.data_ptr() < out.data_ptr() + 2 * out.numel()
                                                       for t in (x, y))
        rows, frame_offs, n_z = plan_formant(rows, n_x, n_y, _out_arg(out)[0], shared)
        from .core.audio_processor import FORMANT_L
        z, R = self._out(out, n_z), len(rows)
        rows_d, rows_h = self._upload(rows)
        wa, g = self._formant_tables
        h = torch.empty((frame_offs[-1], FORMANT_L), dtype=torch.float64, device=self.device) if taps else None
        ws = self._ws(self.lib.vv_pcm_formant_ws_bytes(frame_offs[-1], R))
        self._call(self.lib.vv_pcm_formant, x.data_ptr(), n_x, y.data_ptr(), n_y, rows_d.data_ptr(), rows_h.data_ptr(), R, wa.data_ptr(), g.data_ptr(),
                   self._wsola_window.data_ptr(), z.data_ptr(), z.numel(), _ptr(h), 0 if h is None else h.numel(), ws.data_ptr(), ws.numel() * 8)
        return (z, h, frame_offs) if taps else z

    # ------------------------------------------------------------------ vocoder-bias denoiser (N19)
    @property
    def _denoise_tables(self):
        """(window [1024], twiddles [2][512]: cos | -sin, contiguous) on the device."""
        return self._table("denoise", "denoise_tables")

    def pcm_denoise(self, x: torch.Tensor, rows, strengths, bias: torch.Tensor, out: Optional[torch.Tensor] = None, mags: bool = False):
        """Spectral subtraction of a stationary profile on R requests in one call (vv_pcm_denoise), bit for bit
        core.audio_processor.denoise_pcm.  x int16 flat on the device; rows = HOST rows (x_off, n, y_off, bias_row); strengths = one value
        in 0 ... 16 or one per row; bias = float64 [n_bias][513] (or [513]) on the device.  out = None: a new buffer, or a flat int16 device
        tensor that does not overlap x.  -> y, or with ``mags`` (y, mag, frame_offs): mag the float64 device tensor [frames][1024] of every
        frame's magnitudes, request r's frames mag[frame_offs[r] : frame_offs[r + 1]].  The rows are validated here; the call never
        synchronises."""
        assert x.is_cuda and x.dtype == torch.int16 and x.is_contiguous() and x.dim() == 1
        assert bias.is_cuda and bias.dtype == torch.float64 and bias.is_contiguous() and bias.numel() % 513 == 0 and bias.numel() > 0
        n_x, n_bias = x.numel(), bias.numel() // 513
        shared = isinstance(out, torch.Tensor) and out.data_ptr() < x.data_ptr() + 2 * n_x and x.data_ptr() < out.data_ptr() + 2 * out.numel()
        rows, strengths, frame_offs, n_y = plan_denoise(rows, strengths, n_x, n_bias, _out_arg(out)[0], shared)
        from .core.audio_processor import DENOISE_N
        y, R = self._out(out, n_y), len(rows)
        (rows_d, rows_h), (s_d, s_h) = self._upload(rows), self._upload(strengths, torch.float64)
        window, tw = self._denoise_tables
        mag = torch.empty((frame_offs[-1], DENOISE_N), dtype=torch.float64, device=self.device) if mags else None
        ws = self._ws(self.lib.vv_pcm_denoise_ws_bytes(R))
        self._call(self.lib.vv_pcm_denoise, x.data_ptr(), n_x, rows_d.data_ptr(), rows_h.data_ptr(), R, s_d.data_ptr(), s_h.data_ptr(), bias.data_ptr(),
                   n_bias, window.data_ptr(), tw.data_ptr(), y.data_ptr(), y.numel(), _ptr(mag), 0 if mag is None else mag.numel(), ws.data_ptr(),
                   ws.numel() * 8)
        return (y, mag, frame_offs) if mags else y

    def pcm_denoise_bias(self, x: torch.Tensor, rows) -> torch.Tensor:
        """The bias profiles of R signals in one call (vv_pcm_denoise_bias), bit for bit core.audio_processor.denoise_bias: x int16 flat on
        the device, rows = HOST rows (x_off, n) -> float64 [R][513] on the device.  The rows are validated here; the call never synchronises."""
        assert x.is_cuda and x.dtype == torch.int16 and x.is_contiguous() and x.dim() == 1
        rows, frames = plan_denoise_bias(rows, x.numel())
        (rows_d, rows_h), R = self._upload(rows), len(rows)
        window, tw = self._denoise_tables
        out = torch.empty((R, 513), dtype=torch.float64, device=self.device)
        ws = self._ws(self.lib.vv_pcm_denoise_bias_ws_bytes(frames, R))
        self._call(self.lib.vv_pcm_denoise_bias, x.data_ptr(), x.numel(), rows_d.data_ptr(), rows_h.data_ptr(), R, window.data_ptr(), tw.data_ptr(),
                   out.data_ptr(), out.numel(), ws.data_ptr(), ws.numel() * 8)
        return out

    def _denoise(self, buf: torch.Tensor, offs, lens, denoise, bias):
        """The denoise step of finish_output: the requests with a strength go through pcm_denoise into a copy of the joined buffer, the
        others stay as they are.  bias = None: the model's (vocoder_bias), else 513 values or a float64 device tensor."""
        import numpy as np
        rows = [[offs[i], lens[i], offs[i], 0] for i, s in enumerate(denoise) if s is not None and lens[i] > 0]
        if not rows:
            return buf
        if bias is None:
            bias = self.vocoder_bias()
        elif not isinstance(bias, torch.Tensor):
            from .core.audio_processor import check_denoise_bias
            bias = torch.from_numpy(np.ascontiguousarray(check_denoise_bias(bias))).to(self.device)
        new = buf.clone()
        self.pcm_denoise(buf, rows, [s for i, s in enumerate(denoise) if s is not None and lens[i] > 0], bias, out=new)
        return new

    # ------------------------------------------------------------------ keyed audio watermark (N22)
    def _watermark_chips(self, key: int) -> torch.Tensor:
        """The chip table of ``key`` (int8 [64][320], made on the host) on the device; the last key's table is kept."""
        from .core.audio_processor import watermark_chips
        have = self._tables.get("watermark")
        if have is None or have[0] != key:
            have = self._tables["watermark"] = (key, torch.from_numpy(watermark_chips(key).copy()).to(self.device))
        return have[1]

    def pcm_watermark(self, x: torch.Tensor, rows, key: int, payloads, strength: float = 0.2, out: Optional[torch.Tensor] = None) -> torch.Tensor:
        """The keyed watermark on R requests in one call (vv_pcm_watermark), bit for bit core.audio_processor.watermark_embed.
        x int16 flat on the device; rows = HOST rows (x_off, n, y_off); key = 0 ... 2^64 - 1; payloads = one value in 0 ... 65535 or one per
        row; strength 0 ... 0.5 (0 gives the input back).  out = None: a new buffer, or a flat int16 device tensor that does not overlap x.
        -> y.  The rows are validated here; the call never synchronises."""
        assert x.is_cuda and x.dtype == torch.int16 and x.is_contiguous() and x.dim() == 1
        n_x = x.numel()
        shared = isinstance(out, torch.Tensor) and out.data_ptr() < x.data_ptr() + 2 * n_x and x.data_ptr() < out.data_ptr() + 2 * out.numel()
        rows, gp, gm, n_y = plan_watermark(rows, payloads, strength, n_x, _out_arg(out)[0], shared)
        chips = self._watermark_chips(key)
        y, R = self._out(out, n_y), len(rows)
        rows_d, rows_h = self._upload(rows)
        window, tw = self._denoise_tables
        ws = self._ws(self.lib.vv_pcm_watermark_ws_bytes(R))
        self._call(self.lib.vv_pcm_watermark, x.data_ptr(), n_x, rows_d.data_ptr(), rows_h.data_ptr(), R, chips.data_ptr(), chips.numel(), gp, gm,
                   window.data_ptr(), tw.data_ptr(), y.data_ptr(), y.numel(), ws.data_ptr(), ws.numel() * 8)
        return y

    def pcm_watermark_detect(self, x: torch.Tensor, rows, key: int, cells: bool = False):
        """The detector's statistic of R clips in one call (vv_pcm_watermark_detect), equal to
        core.audio_processor.watermark_stats: x int16 flat on the device, rows = HOST rows (x_off, n), n <= 2^24 -> stats, the int64 device
        tensor [R][256][24][2] of {num, den} per alignment and bit (core.audio_processor.watermark_decide turns a clip's into the result
        record); with ``cells`` (stats, cells, frame_offs): the int32 device tensor [frames][320] of the cell values, request r's frames
        cells[frame_offs[r] : frame_offs[r + 1]].  The rows are validated here; the call never synchronises."""
        assert x.is_cuda and x.dtype == torch.int16 and x.is_contiguous() and x.dim() == 1
        from .core.audio_processor import WATERMARK_K, WATERMARK_NB, WATERMARK_Q
        rows, frame_offs = plan_watermark_detect(rows, x.numel())
        chips = self._watermark_chips(key)
        (rows_d, rows_h), R = self._upload(rows), len(rows)
        window, tw = self._denoise_tables
        stats = torch.empty((R, WATERMARK_Q, WATERMARK_NB, 2), dtype=torch.int64, device=self.device)
        cell = torch.empty((frame_offs[-1], WATERMARK_K), dtype=torch.int32, device=self.device) if cells else None
        ws = self._ws(self.lib.vv_pcm_watermark_detect_ws_bytes(frame_offs[-1], R))
        self._call(self.lib.vv_pcm_watermark_detect, x.data_ptr(), x.numel(), rows_d.data_ptr(), rows_h.data_ptr(), R, chips.data_ptr(), chips.numel(),
                   window.data_ptr(), tw.data_ptr(), stats.data_ptr(), stats.numel(), _ptr(cell), 0 if cell is None else cell.numel(), ws.data_ptr(),
                   ws.numel() * 8)
        return (stats, cell, frame_offs) if cells else stats

    def _watermark(self, buf: torch.Tensor, offs, lens, key: int, payloads, strength: float):
        """The watermark step of finish_output: the requests with a payload go through pcm_watermark into a copy of the buffer, the others
        stay as they are."""
        sel = [i for i, p in enumerate(payloads) if p is not None and lens[i] > 0]
        if not sel:
            return buf
        new = buf.clone()
        self.pcm_watermark(buf, [[offs[i], lens[i], offs[i]] for i in sel], key, [payloads[i] for i in sel], strength, out=new)
        return new

    # ------------------------------------------------------------------ FLAC output (N15, N16)
    def pcm_flac(self, x: torch.Tensor, rows, sample_rate: int, lpc_order: int = 0):
        """FLAC frames of R final signals in one call (vv_pcm_flac), byte for byte core.audio_processor.flac_encode_frames.
        lpc_order 1 ... 12: with LPC subframes (vv_pcm_flac_lpc; N16), byte for byte the mirror with that order; 0 = vv_pcm_flac as ever.
        x int16 flat on the device; rows = HOST rows (src_off, n, frame0, last): x[src_off, +n) becomes ceil(n / 4096) frames numbered from
        frame0; last = 0 = a block of a stream (n a multiple of 4096).  -> (y, info): y the uint8 device buffer with the frames of all rows
        back to back, info the (R + 1) x 3 int64 device tensor {offset of the row's first frame, smallest frame, largest frame} with
        info[R][0] = the total bytes.  The rows are validated here; the call never synchronises."""
        assert x.is_cuda and x.dtype == torch.int16 and x.is_contiguous() and x.dim() == 1
        lpc_order, rows, n_y, frames = plan_flac(rows, x.numel(), sample_rate, lpc_order)
        (rows_d, rows_h), R = self._upload(rows), len(rows)
        y = torch.empty((n_y,), dtype=torch.uint8, device=self.device)
        info = torch.empty((R + 1, 3), dtype=torch.int64, device=self.device)
        ws = self._ws(self.lib.vv_pcm_flac_lpc_ws_bytes(frames, R, lpc_order) if lpc_order else self.lib.vv_pcm_flac_ws_bytes(frames, R))
        fn, order = (self.lib.vv_pcm_flac_lpc, [lpc_order]) if lpc_order else (self.lib.vv_pcm_flac, [])
        self._call(fn, x.data_ptr(), x.numel(), rows_d.data_ptr(), rows_h.data_ptr(), R, int(sample_rate), *order, y.data_ptr(), n_y, info.data_ptr(),
                   ws.data_ptr(), ws.numel() * 8)
        return y, info

    # ------------------------------------------------------------------ FLAC input (N17)
    def flac_index(self, data: torch.Tensor, rows):
        """vv_flac_index: the frames of R FLAC clips whose frame bytes lie back to back in ``data`` (uint8 on the device,
        each clip 4-byte aligned, 8 bytes of padding behind the last).  rows = HOST rows {byte offset, n_bytes, channels, bits, min block,
        max block, rate, total}.  -> (info R x 4 int64 on the device {status, byte, frames, samples}, the workspace flac_decode consumes).
        The rows are validated here before anything is launched; the call never synchronises."""
        assert data.is_cuda and data.dtype == torch.uint8 and data.is_contiguous() and data.dim() == 1
        n_bytes = data.numel()
        rows = plan_flac_index(rows, n_bytes, data.data_ptr() % 8 == 0)
        (rows_d, rows_h), R = self._upload(rows), len(rows)
        info = torch.empty((R, 4), dtype=torch.int64, device=self.device)
        ws = self._ws(self.lib.vv_flac_index_ws_bytes(n_bytes, R))
        self._call(self.lib.vv_flac_index, data.data_ptr(), n_bytes, rows_d.data_ptr(), rows_h.data_ptr(), R, info.data_ptr(), ws.data_ptr(), ws.numel() * 8)
        return info, (ws, rows_h, rows_d)

    def flac_decode(self, data: torch.Tensor, index, lay, pcm: torch.Tensor):
        """vv_flac_decode: the clips ``flac_index`` passed, into ``pcm`` (uint8 on the device) as the interleaved little-endian PCM
        vv_ingest_pcm reads.  index = flac_index's second result; lay = HOST rows {pcm byte offset, frames, samples} per clip (a refused
        clip: frames = samples = 0).  -> info2 R x 2 int64 on the device {status, byte}: non-zero where a restored sample left its range."""
        ws, rows_h, rows_d = index
        assert data.is_cuda and data.dtype == torch.uint8 and pcm.is_cuda and pcm.dtype == torch.uint8 and pcm.is_contiguous() and pcm.dim() == 1
        R, n_pcm = rows_h.shape[0], pcm.numel()
        full, F, P = plan_flac_decode(lay, rows_h.tolist(), n_pcm)
        info2 = torch.empty((R, 2), dtype=torch.int64, device=self.device)
        ws2 = self._ws(self.lib.vv_flac_decode_ws_bytes(P, F))
        lay_d, lay_h = self._upload(full)
        self._call(self.lib.vv_flac_decode, data.data_ptr(), data.numel(), rows_d.data_ptr(), rows_h.data_ptr(), R, lay_d.data_ptr(), lay_h.data_ptr(),
                   ws.data_ptr(), ws.numel() * 8, pcm.data_ptr(), n_pcm, info2.data_ptr(), ws2.data_ptr(), ws2.numel() * 8)
        return info2

    def flac_clips(self, files, pcm: Optional[torch.Tensor] = None, pcm_offsets=None):
        """Complete FLAC files (bytes) -> their PCM on the device, without a decoded sample crossing the bus: container parsing on the
        host, one upload of the frame bytes, flac_index, ONE small readback of info (32 R bytes, the synchronisation), flac_decode, one
        small readback of info2.  -> (pcm uint8 on the device, [per file: (byte offset, frames, width, rate, channels) or the FlacError
        the mirror would raise]).  A refused file does not disturb the others.  With ``pcm`` / ``pcm_offsets`` None the buffer is laid
        out here (4-byte aligned clips); else ``pcm_offsets(sizes) -> (buffer, offsets)`` lets the caller place the clips in a buffer
        it shares with other PCM."""
        from .core.audio_processor import FlacError, flac_container
        infos, parts, rows, pos = [], [], [], 0
        for data in files:
            data = bytes(data)
            try:
                fi = flac_container(data)
            except FlacError as e:
                infos.append(e)
                continue
            infos.append(fi)
            body = data[fi.start:]
            rows.append([pos, len(body), fi.channels, fi.bits, fi.min_block, fi.max_block, fi.rate, fi.total])
            parts.append(body + b"\0" * (-len(body) % 4))
            pos += len(parts[-1])
        live = [i for i, fi in enumerate(infos) if not isinstance(fi, FlacError)]
        out, sizes, lay = list(infos), [0] * len(files), []
        if live:
            buf = torch.frombuffer(bytearray(b"".join(parts) + b"\0" * (-pos % 8 + 8)), dtype=torch.uint8).to(self.device)
            info_d, index = self.flac_index(buf, rows)
            info = info_d.cpu().tolist()                          # the one synchronisation in front of the layout
            for i, (status, byte, frames, samples), row in zip(live, info, rows):
                if status:
                    out[i] = FlacError(status, infos[i].start + byte)
                    lay.append([0, 0])
                else:
                    sizes[i] = samples * row[2] * _FLAC_WIDTH[row[3]]
                    lay.append([frames, samples])
        if pcm_offsets is None:
            offs, end = _place(sizes, 4)
            pcm = torch.empty((max(-(-end // 4) * 4, 8),), dtype=torch.uint8, device=self.device)
        else:
            pcm, offs = pcm_offsets(sizes)
        if live:
            at = 0
            for j, i in enumerate(live):                          # a refused clip sits, empty, where the previous one ended
                if lay[j][1]:
                    at = offs[i]
                lay[j] = [at] + lay[j]
                at += sizes[i]
            info2 = self.flac_decode(buf, index, lay, pcm).cpu().tolist()
            for j, i in enumerate(live):
                if isinstance(out[i], FlacError):
                    continue
                if info2[j][0]:
                    out[i] = FlacError(info2[j][0], infos[i].start + info2[j][1])
                else:
                    out[i] = (offs[i], lay[j][2], _FLAC_WIDTH[rows[j][3]], rows[j][6], rows[j][2])
        return pcm, out

    def _flac_files(self, buf: torch.Tensor, offs, lens, sample_rate: int, lpc_order: int = 0):
        """The last step of finish_output with encoding "flac": one vv_pcm_flac (lpc_order > 0: vv_pcm_flac_lpc) call over the requests, ONE small copy of info (24 (R + 1)
        bytes, the one synchronisation), one copy of exactly info[R][0] bytes; the host puts each request's stream header in front, with
        its true sample count and its frame sizes.  An empty request is a header alone."""
        import numpy as np
        from .core.audio_processor import flac_stream_header
        sel, frames = [i for i, n in enumerate(lens) if n > 0], {}
        if sel:
            y, info = self.pcm_flac(buf, [[offs[i], lens[i], 0, 1] for i in sel], sample_rate, lpc_order)
            info = info.cpu().numpy()
            total = int(info[len(sel), 0])
            host = y[:total].cpu().numpy()
            for j, i in enumerate(sel):
                end = int(info[j + 1, 0]) if j + 1 < len(sel) else total
                frames[i] = (host[int(info[j, 0]): end], int(info[j, 1]), int(info[j, 2]))
        out = []
        for i, n in enumerate(lens):
            data, lo, hi = frames.get(i, (np.zeros(0, np.uint8), 0, 0))
            out.append(np.concatenate([np.frombuffer(flac_stream_header(sample_rate, n, lo, hi), np.uint8), data]))
        return out

    # ------------------------------------------------------------------ IMA ADPCM output, ADPCM / G.711 input (N25)
    def pcm_adpcm(self, x: torch.Tensor, rows, samples_per_block: int, n_y: Optional[int] = None, out: Optional[torch.Tensor] = None) -> torch.Tensor:
        """IMA ADPCM blocks of R final signals in one call (vv_pcm_adpcm), byte for byte
        core.audio_processor.adpcm_encode_blocks.  x int16 flat on the device; rows = HOST rows (src_off, n, dst_off in bytes, a multiple of
        4, ascending): x[src_off, +n) becomes ceil(n / samples_per_block) blocks of (samples_per_block - 1) / 2 + 4 bytes at dst_off.
        -> y, the uint8 device buffer [n_y] (out = an existing one).  The size is the host's to know: nothing is read back.  The rows are
        validated here; the call never synchronises."""
        assert x.is_cuda and x.dtype == torch.int16 and x.is_contiguous() and x.dim() == 1
        spb, rows, n_y, _most = plan_adpcm(rows, x.numel(), samples_per_block, n_y if out is None else out.numel())
        y = self._out(out, n_y, torch.uint8, floor=8)
        rows_d, rows_h = self._upload(rows)
        self._call(self.lib.vv_pcm_adpcm, x.data_ptr(), x.numel(), rows_d.data_ptr(), rows_h.data_ptr(), len(rows), spb, y.data_ptr(), y.numel())
        return y[:n_y]

    def wav_decode(self, data: torch.Tensor, rows, pcm: torch.Tensor) -> torch.Tensor:
        """vv_wav_decode: the coded data chunks of R G.711 / IMA ADPCM WAVE clips in ``data`` (uint8 on the device, each clip
        16-byte aligned) into ``pcm`` (uint8 on the device) as the interleaved int16 frames vv_ingest_pcm reads, sample for sample
        core.audio_processor.wav_coded_frames.  rows = HOST rows {data byte offset, n_bytes, tag, channels, block align, frames, pcm byte
        offset}.  -> status R x 2 int64 on the device {reason, byte inside the clip's data}.  The rows are validated here; the call never
        synchronises."""
        assert data.is_cuda and data.dtype == torch.uint8 and data.is_contiguous() and data.dim() == 1
        assert pcm.is_cuda and pcm.dtype == torch.uint8 and pcm.is_contiguous() and pcm.dim() == 1
        rows = plan_wav_decode(rows, data.numel(), pcm.numel())
        rows_d, rows_h = self._upload(rows)
        status = torch.empty((len(rows), 2), dtype=torch.int64, device=self.device)
        self._call(self.lib.vv_wav_decode, data.data_ptr(), data.numel(), rows_d.data_ptr(), rows_h.data_ptr(), len(rows), pcm.data_ptr(), pcm.numel(),
                   status.data_ptr())
        return status

    def wav_clips(self, infos, pcm_offsets=None):
        """The coded WAVE clips ``infos`` (core.audio_processor.WavInfo of tag 6, 7 or 0x11) -> their PCM on the device, without a decoded
        sample crossing the bus: one upload of the data chunks, vv_wav_decode, one small readback of the status (16 R bytes).
        -> (pcm uint8 on the device, [per clip: (byte offset, frames, 2, rate, channels) or the WavError the mirror would raise]).  A
        refused clip does not disturb the others.  ``pcm_offsets(sizes) -> (buffer, offsets)`` lets the caller place the clips (16-byte
        aligned) in a buffer it shares with other PCM."""
        from .core.audio_processor import WavError, wav_coded_frame_count
        parts, rows, pos = [], [], 0
        for fi in infos:
            n = len(fi.data)
            rows.append([pos, n, fi.tag, fi.channels, fi.block_align, wav_coded_frame_count(fi), 0])
            parts.append(fi.data + b"\0" * (-n % 16))
            pos += len(parts[-1])
        sizes = [r[5] * r[3] * 2 for r in rows]
        if pcm_offsets is None:
            offs, end = _place(sizes, 16)
            pcm = torch.empty((max(-(-end // 16) * 16, 16),), dtype=torch.uint8, device=self.device)
        else:
            pcm, offs = pcm_offsets(sizes)
        for r, o in zip(rows, offs):
            r[6] = o
        buf = torch.frombuffer(bytearray(b"".join(parts) + b"\0" * 16), dtype=torch.uint8).to(self.device)
        status = self.wav_decode(buf, rows, pcm).cpu().tolist()
        out = [WavError(code, fi.data_at + byte) if code else (r[6], r[5], 2, fi.rate, fi.channels) for (code, byte), fi, r in zip(status, infos, rows)]
        return pcm, out

    def _adpcm_files(self, buf: torch.Tensor, offs, lens, sample_rate: int):
        """The last step of finish_output with encoding "adpcm": one vv_pcm_adpcm call over the requests and ONE copy of the blocks -- their
        sizes are the host's to know; it puts each request's RIFF header in front, with the true sample count.  An empty request is a
        header alone."""
        import numpy as np
        from .core.audio_processor import adpcm_block_align, adpcm_samples_per_block, adpcm_wav
        ba = adpcm_block_align(sample_rate)
        spb = adpcm_samples_per_block(ba)
        sizes = [-(-n // spb) * ba for n in lens]
        out_offs, end = _place(sizes)
        rows = [[o, n, do] for o, n, do in zip(offs, lens, out_offs) if n > 0]
        host = self.pcm_adpcm(buf, rows, spb, n_y=end).cpu().numpy() if rows else np.zeros(0, np.uint8)
        return [adpcm_wav(host[do: do + nb], sample_rate, n) for do, nb, n in zip(out_offs, sizes, lens)]

    def finish_output(self, pcm: torch.Tensor, plans, cross_fade_duration: float, sample_rate: int, rate: Optional[int] = None,
                      encoding: str = "pcm16", loudness=None, peak_dbfs: float = -1.0, limiter=None, pitch=None, tempo=None, flac_lpc_order: int = 0,
                      formants=None, denoise=None, denoise_bias=None, watermark=None, watermark_key=None, watermark_strength: float = 0.2):
        """The whole output stage of R requests on the caller's stream: join (-> denoiser) (-> pitch and tempo) (-> watermark) (-> loudness) (-> limiter) (-> output rate)
        (-> G.711), then ONE device-to-host copy of the final bytes.  pcm int16 on the device, plans = per request its chunks' (src_off, len)
        spans.  pitch (semitones) / tempo = one value for every request, or a per-request list with None entries (N14; all None = nothing
        new is called): core.audio_processor.prosody_plan turns them into a WSOLA stretch and a rate conversion on the joined signal, and
        every later step runs on the result, so levels and the ceiling are those of what is heard.
        loudness = a target in LUFS for every request, or a per-request list with None entries (N12; None = nothing new is called);
        peak_dbfs = its sample-peak ceiling.  limiter = None | "sample" | "true" for every request, or a per-request list (N13; None =
        nothing new is called): a request with a limiter is measured only (pcm_loudness, out="measure") and takes its uncapped loudness
        gain, or the gain 1 without a target, through pcm_limit in place; the others keep the capped gain of N12.
        encoding "flac" (N15): the final PCM goes through pcm_flac instead of the one copy: a small copy of the frames' sizes, then a copy
        of exactly the frames' bytes; each request comes back as a complete FLAC file.  flac_lpc_order 1 ... 12 (N16) adds LPC subframes
        (vv_pcm_flac_lpc instead of vv_pcm_flac) and is refused with another encoding.
        formants (N18) = "shift" | "keep" for every request, or a per-request list; None = "shift": a request with "keep" and a pitch
        ratio other than 1 has the spectral envelope of its joined signal put back by pcm_formant, directly behind the rate conversion
        that makes the pitch; a request with tempo alone or without prosody runs nothing new.
        denoise (N19) = one strength (0 < s <= 16) for every request, or a per-request list with None entries; None or all None = nothing
        new is called.  A request with a strength goes through pcm_denoise directly behind the join and before pitch and tempo, into a new
        buffer, against denoise_bias: 513 values or a float64 device tensor, None = the model's own (vocoder_bias).
        watermark (N22) = one payload (0 ... 65535) for every request, or a per-request list with None entries; None or all None = nothing
        new is called.  A request with a payload goes through pcm_watermark under watermark_key (0 ... 2^64 - 1; a payload without a key is
        refused) at watermark_strength, directly behind pitch and tempo (and formants) and before the loudness step, into a new buffer: the
        loudness gain, the peak ceiling and the limiter's promise hold for what is heard, and the detector does not mind a constant gain.
        encoding "adpcm" (N25): the final PCM goes through pcm_adpcm; the blocks' sizes follow from the lengths, so there is no size
        readback, and each request comes back as a complete IMA ADPCM WAVE file (60 header bytes made on the host, then the blocks).
        -> a list of R numpy arrays: int16 at ``rate`` (None = sample_rate), uint8 G.711 codes, or the uint8 bytes of a FLAC or ADPCM file."""
        from .core.audio_processor import check_flac_lpc_order, resample_len
        if check_flac_lpc_order(flac_lpc_order) and encoding != "flac":
            raise ValueError("finish_output: flac_lpc_order belongs to the encoding 'flac'")
        buf, offs, lens = self.join_chunks(pcm, plans, cross_fade_duration, sample_rate)
        denoise = plan_finish_denoise(len(lens), denoise)
        if denoise is not None:
            buf = self._denoise(buf, offs, lens, denoise, denoise_bias)
        pitch, tempo, groups = plan_finish(len(lens), loudness, limiter, pitch, tempo)
        if formants is not None:
            from .core.audio_processor import check_formants
            formants = [check_formants(f) for f in _per_request("finish_output", formants, len(lens), "formants entry per request")]
        if pitch is not None:
            buf, offs, lens = self._prosody(buf, offs, lens, pitch, tempo, formants)
        watermark = plan_finish_watermark(len(lens), watermark, watermark_key, watermark_strength)
        if watermark is not None:
            buf = self._watermark(buf, offs, lens, *watermark)
        for mode, sel, tg in groups:       # in place on the joined buffer: the apply passes are elementwise
            rows, meas = [[offs[i], lens[i], offs[i]] for i in sel], None
            if mode is None:
                self.pcm_loudness(buf, rows, sample_rate, tg, peak_dbfs, out=buf)
                continue
            if any(t is not None for t in tg):
                _none, meas = self.pcm_loudness(buf, rows, sample_rate, tg, peak_dbfs, out="measure", stats=True)
            self.pcm_limit(buf, rows, sample_rate, peak_dbfs, mode, meas=meas, targets=tg if meas is not None else None, out=buf)
        if rate is not None and int(rate) != int(sample_rate):
            _taps, up, down, _skip = self._output_taps(int(sample_rate), int(rate))
            out_lens = [resample_len(n, up, down) for n in lens]
            out_offs, end = _place(out_lens)
            rows = [[o, n, do, dn, 0, 0] for o, n, do, dn in zip(offs, lens, out_offs, out_lens)]
            buf, offs, lens = (self.pcm_resample(buf, rows, sample_rate, rate, n_y=end) if end else buf[:0]), out_offs, out_lens
        if encoding == "flac":             # N15: variable-length output -- the frames' total comes back first, then exactly that many bytes
            return self._flac_files(buf, offs, lens, int(sample_rate) if rate is None else int(rate), flac_lpc_order)
        if encoding == "adpcm":            # N25: blocks of a size the host knows -- one copy, then each request's RIFF header in front
            return self._adpcm_files(buf, offs, lens, int(sample_rate) if rate is None else int(rate))
        if encoding != "pcm16":
            out_offs, end = _place(lens)
            rows = [[o, n, do] for o, n, do in zip(offs, lens, out_offs)]
            buf = self.pcm_encode(buf, rows, encoding, n_y=end) if end else torch.empty((0,), dtype=torch.uint8, device=self.device)
            offs = out_offs
        host = buf.cpu().numpy()
        return [host[o: o + n] for o, n in zip(offs, lens)]

    def output_stream_backends(self, sample_rate: int, rate: Optional[int], encoding: str, max_upload: int = 1 << 18):
        """(resample, encode) callables for core.audio_processor.OutputStream on this device: host blocks go up in pieces of at most
        ``max_upload`` samples (0.5 MB), through vv_pcm_resample / vv_pcm_encode, and come back.  With encoding "flac" the second one is
        the ``encode(pcm, frame0, last[, lpc_order])`` of core.audio_processor.FlacStream (vv_pcm_flac, vv_pcm_flac_lpc), which sits behind
        the OutputStream; with "adpcm" it is the ``encode(pcm)`` of core.audio_processor.AdpcmStream (vv_pcm_adpcm), in the same place."""
        import numpy as np

        def up_(x):
            parts = [torch.from_numpy(np.ascontiguousarray(x[i: i + max_upload])).to(self.device) for i in range(0, x.size, max_upload)]
            return parts[0] if len(parts) == 1 else torch.cat(parts)

        def resample(x, m0, i0, n_out):
            x = np.asarray(x, dtype=np.int16).reshape(-1)
            if n_out <= 0:
                return np.zeros(0, np.int16)
            xd = up_(x) if x.size else torch.zeros((8,), dtype=torch.int16, device=self.device)
            return self.pcm_resample(xd, [[0, x.size, 0, n_out, m0, i0]], sample_rate, rate, n_y=n_out).cpu().numpy()

        def encode(y):
            y = np.asarray(y, dtype=np.int16).reshape(-1)
            if y.size == 0:
                return np.zeros(0, np.uint8)
            return self.pcm_encode(up_(y), [[0, y.size, 0]], encoding, n_y=y.size).cpu().numpy()

        def flac(pcm, frame0, last, lpc_order=0):      # FlacStream's back end (N15, N16): whole blocks (last = False) and the final short frame alike
            pcm = np.asarray(pcm, dtype=np.int16).reshape(-1)
            if pcm.size == 0:
                return np.zeros(0, np.uint8)
            y, info = self.pcm_flac(up_(pcm), [[0, pcm.size, int(frame0), 1 if last else 0]], sample_rate if rate is None else rate, lpc_order)
            return y[: int(info[1, 0])].cpu().numpy()

        def adpcm(pcm):                                # AdpcmStream's back end (N25): whole blocks, or the final one to be padded
            from .core.audio_processor import adpcm_block_align, adpcm_samples_per_block
            pcm = np.asarray(pcm, dtype=np.int16).reshape(-1)
            if pcm.size == 0:
                return np.zeros(0, np.uint8)
            spb = adpcm_samples_per_block(adpcm_block_align(sample_rate if rate is None else rate))
            return self.pcm_adpcm(up_(pcm), [[0, pcm.size, 0]], spb).cpu().numpy()

        return (resample if rate is not None and int(rate) != int(sample_rate) else None), \
            (flac if encoding == "flac" else adpcm if encoding == "adpcm" else encode if encoding != "pcm16" else None)
