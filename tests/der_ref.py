"""The diarization error rate, restated for the tests from the RULE in score.py's docstring and not from its code: plain Python loops over
frames, the reference speakers' activity as a union of intervals found by a sweep over start / end events, and scipy's
linear_sum_assignment for `correct`.  Also the generators of the reference turn sets and hypothesis tables that the CPU and GPU tests share."""
from __future__ import annotations

import math

import numpy as np
from scipy.optimize import linear_sum_assignment

RATE, HOP, FIRST = 16000, 270, 495


def samples(t: float) -> int:
    return int(math.floor(t * RATE + 0.5))


def n_frames(n_samples: int) -> int:
    """The frames g >= 0 whose centre 270 g + 495 lies inside the recording."""
    g = 0
    while HOP * g + FIRST < n_samples:
        g += 1
    return g


def number_names(turns):
    first = {}
    for a, _, name in turns:
        s = samples(a)
        if name not in first or s < first[name]:
            first[name] = s
    return sorted(first, key=lambda nm: (first[nm], nm))


def intervals(turns, name):
    """The maximal intervals of the union of `name`'s non-empty turns [s0, s1) (abutting turns join): a sweep over events, starts first."""
    ev = []
    for a, b, nm in turns:
        if nm == name and samples(b) > samples(a):
            ev += [(samples(a), 0), (samples(b), 1)]
    out, depth, open_at = [], 0, None
    for pos, kind in sorted(ev):
        if kind == 0:
            if depth == 0:
                open_at = pos
            depth += 1
        else:
            depth -= 1
            if depth == 0:
                out.append((open_at, pos))
    joined = []
    for a, b in out:                                           # an interval that closes where the next opens is one interval
        if joined and joined[-1][1] == a:
            joined[-1] = (joined[-1][0], b)
        else:
            joined.append((a, b))
    return joined


def reference_frames(turns, n_samples: int, collar_s: float = 0.0, skip_overlap: bool = False):
    """-> (names, mask: one Python int per frame with bit i = speaker i active, scored: one bool per frame)."""
    names = number_names(turns)
    spans = [intervals(turns, nm) for nm in names]
    c = samples(collar_s) if collar_s > 0 else 0
    mask, scored = [], []
    for g in range(n_frames(n_samples)):
        centre = HOP * g + FIRST
        m = 0
        for i, sp in enumerate(spans):
            if any(a <= centre < b for a, b in sp):
                m |= 1 << i
        ok = True
        if c > 0 and any(abs(centre - edge) < c for sp in spans for ab in sp for edge in ab):
            ok = False
        if skip_overlap and bin(m).count("1") >= 2:
            ok = False
        mask.append(m)
        scored.append(ok)
    return names, mask, scored


def tallies(mask, scored, speakers, S: int, K: int):
    """-> (co [S, K] int64, [scored, total, missed, false_alarm, both])."""
    co = np.zeros((S, K), np.int64)
    t = [0, 0, 0, 0, 0]
    for g, (m, ok) in enumerate(zip(mask, scored)):
        if not ok:
            continue
        hyp = [int(v) for v in speakers[g] if v >= 0]
        nref, nhyp = bin(m).count("1"), len(hyp)
        t[0] += 1
        t[1] += nref
        t[2] += max(0, nref - nhyp)
        t[3] += max(0, nhyp - nref)
        t[4] += min(nref, nhyp)
        for i in range(S):
            if m >> i & 1:
                for j in set(hyp):
                    if j < K:
                        co[i, j] += 1
    return co, t


def optimum(co) -> int:
    co = np.asarray(co, dtype=np.int64)
    if co.size == 0:
        return 0
    r, c = linear_sum_assignment(co, maximize=True)
    return int(co[r, c].sum())


def der_ref(speakers, n_samples: int, turns, collar_s: float = 0.0, skip_overlap: bool = False, K=None) -> dict:
    speakers = np.asarray(speakers).reshape(-1, 2)
    names, mask, scored = reference_frames(turns, n_samples, collar_s, skip_overlap)
    assert len(mask) == len(speakers)
    if K is None:
        K = int(speakers.max()) + 1 if speakers.size else 0
    co, (n_sc, total, missed, fa, both) = tallies(mask, scored, speakers, len(names), max(K, 0))
    correct = optimum(co)
    err = missed + fa + both - correct
    der = (0.0 if err == 0 else math.inf) if total == 0 else err / total
    return dict(names=names, mask=mask, scored_frames=scored, co=co, scored=n_sc, total=total, missed=missed, false_alarm=fa, both=both,
                correct=correct, confusion=both - correct, der=der)


# ------------------------------------------------------------------------------------------------ shared cases
def random_turns(rng, S: int, n_samples: int):
    """S named speakers with turn sets that exercise the preparation: turns that overlap and abut others of the same speaker, zero-length
    and reversed turns, turns that run past the end and turns wholly behind it.  Names are shuffled against the order of first start."""
    dur = max(n_samples / RATE, 0.5)
    ids = rng.permutation(S)
    turns = []
    for i in range(S):
        name = f"spk{int(ids[i]):02d}"
        a = float(np.round(rng.uniform(0, dur), 4))
        b = float(np.round(a + rng.uniform(0.05, 0.4 * dur), 4))
        turns.append((a, b, name))
        kind = int(rng.integers(0, 6))
        if kind == 0:
            turns.append((b, float(np.round(b + rng.uniform(0.05, 1.0), 4)), name))                    # abuts
        elif kind == 1:
            turns.append((float(np.round((a + b) / 2, 4)), float(np.round(b + rng.uniform(0.0, 1.0), 4)), name))   # overlaps
        elif kind == 2:
            turns.append((a, a, name))                                                                 # zero length, at a boundary
            turns.append((float(np.round(rng.uniform(0, dur), 4)),) * 2 + (name,))                     # zero length, anywhere
        elif kind == 3:
            turns.append((float(np.round(max(dur - 0.3, 0.0), 4)), float(np.round(dur + 2.0, 4)), name))   # runs past the end
            turns.append((float(np.round(dur + 3.0, 4)), float(np.round(dur + 4.0, 4)), name))         # wholly behind the end
        elif kind == 4:
            turns.append((b + 0.2, b + 0.1, name))                                                     # reversed: no turn
    order = rng.permutation(len(turns))
    return [turns[int(k)] for k in order]


def random_speakers(rng, G: int, K: int):
    """speakers [G, 2] int32 with rows of all three kinds: (-1, -1), (k, -1), (k, j) with j != k."""
    sp = np.full((G, 2), -1, np.int32)
    if K == 0 or G == 0:
        return sp
    kind = rng.integers(0, 3 if K >= 2 else 2, G)
    first = rng.integers(0, K, G)
    second = (first + rng.integers(1, max(K, 2), G)) % max(K, 2)
    sp[kind >= 1, 0] = first[kind >= 1]
    sp[kind == 2, 1] = second[kind == 2]
    return sp
