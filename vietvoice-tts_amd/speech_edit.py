"""Host plan of a speech edit: which samples of the source clip are kept, where the regenerated spans go, and the
frame mask that conditions the acoustic model.  Pure numpy; the device work is HipSynth.edit_batch (csrc/vv_edit.hip).

F5-TTS's edit arithmetic (speech_edit.py + CFM.sample(edit_mask=...)) with every boundary on the hop grid, so that the frame mask
and the splice agree exactly (F5 rounds sample and frame lengths separately and can drift by a frame):

  H = S // hop,  a_i = min(r(s_i sr / hop), H) hop,  b_i = min(r(e_i sr / hop), H) hop,  g_i = r(d_i sr / hop),  r(x) = floor(x + 1/2)
  spliced = src[0:a_1] | zeros(g_1 hop) | src[b_1:a_2] | ... | zeros(g_P hop) | src[b_P:S]   (length L)
  N = L // hop + 1 frames; keep[t] = 0 on the frames of a gap, 1 elsewhere.

g_i = 0 is a pure deletion, a_i = b_i a pure insertion; an edit reaching the end keeps the source's final partial hop.
"""
from __future__ import annotations

import math
from dataclasses import dataclass
from typing import List, Optional, Sequence, Tuple

import numpy as np


def _r(x: float) -> int:
    return int(math.floor(x + 0.5))


@dataclass(frozen=True)
class EditPlan:
    segments: Tuple[Tuple[int, int, int], ...]    # (src_off, dst_off, n): source samples copied into the spliced clip, n > 0, in order
    gaps: Tuple[Tuple[int, int], ...]             # per part: the frames [f0, f1) regenerated (f0 == f1 for a deletion)
    spliced_len: int                              # L samples
    n_frames: int                                 # N = L // hop + 1
    keep: np.ndarray                              # uint8 [N]: 0 inside a gap, 1 elsewhere

    def rows(self, item: int = 0, src_base: int = 0) -> List[List[int]]:
        """Splice descriptor rows {item, src_off, dst_off, n} for HipSynth.edit_splice, the source clip at src_base."""
        return [[int(item), src_base + so, do, n] for so, do, n in self.segments]


def plan_edit(n_src: int, parts: Sequence[Tuple[float, float]], fix_duration: Optional[Sequence[float]], sample_rate: int, hop: int,
              n_fft: int, max_frames: int) -> EditPlan:
    """n_src: source samples; parts: [(start, end)] seconds to edit, in order; fix_duration: the new length of each part in seconds
    (default: its old length).  Raises ValueError for a request that cannot be planned."""
    S, sr = int(n_src), int(sample_rate)
    parts = [(float(s), float(e)) for s, e in parts]
    for s, e in parts:
        if not (0.0 <= s <= e <= S / sr):
            raise ValueError(f"edit span ({s}, {e}) must satisfy 0 <= start <= end <= {S / sr:.6f} s (the source clip)")
    if fix_duration is None:
        durs = [e - s for s, e in parts]
    else:
        durs = [float(d) for d in fix_duration]
        if len(durs) != len(parts):
            raise ValueError(f"fix_duration has {len(durs)} entries for {len(parts)} parts")
    for d in durs:
        if not (math.isfinite(d) and d >= 0.0):
            raise ValueError(f"a new span length must be a finite number of seconds >= 0, got {d}")
    H = S // hop
    ab = [(min(_r(s * sr / hop), H) * hop, min(_r(e * sr / hop), H) * hop) for s, e in parts]
    for i in range(1, len(ab)):
        if ab[i - 1][1] > ab[i][0]:
            raise ValueError(f"edit spans {parts[i - 1]} and {parts[i]} are out of order or overlap on the hop grid")
    segments, gaps = [], []
    src, dst = 0, 0
    for (a, b), d in zip(ab, durs):
        if a > src:
            segments.append((src, dst, a - src))
        dst += a - src
        g = _r(d * sr / hop)
        gaps.append((dst // hop, dst // hop + g))
        dst += g * hop
        src = b
    if S > src:
        segments.append((src, dst, S - src))
    L = dst + (S - src)
    if L <= n_fft / 2:
        raise ValueError(f"the edited clip would have {L} samples; the mel front end needs more than n_fft / 2 = {n_fft / 2:g}")
    N = L // hop + 1
    if N > max_frames:
        raise ValueError(f"the edited clip would have {N} frames, more than the {max_frames} the model's position tables hold")
    keep = np.ones(N, dtype=np.uint8)
    for f0, f1 in gaps:
        keep[f0:f1] = 0
    return EditPlan(tuple(segments), tuple(gaps), L, N, keep)
