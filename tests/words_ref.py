"""An independent reference for words.py: the attribution of words to diarization frames and the word-level error rate, written as plain
per-word, per-frame Python loops over Python integers (not the vectorised restatement words.attribute_host), with a brute-force assignment
for small tables.  Imports nothing from the product."""
from __future__ import annotations

import itertools
import math

import numpy as np

HOP, FIRST, RATE = 270, 495, 16000


def global_frames(n_samples: int) -> int:
    g = 0
    while HOP * g + FIRST < n_samples:
        g += 1
    return g


def to_samples(t: float) -> int:
    return int(math.floor(t * RATE + 0.5))


def gap_frames(max_gap_s: float) -> int:
    return to_samples(max_gap_s) // HOP


def named(entry, K):
    """The speakers a frame names, in entry order, each once."""
    out = []
    for h in entry:
        h = int(h)
        if 0 <= h < K and h not in out:
            out.append(h)
    return out


def attribute_word(speakers, K: int, s0: int, s1: int, gap: int):
    G = len(speakers)
    if G == 0:
        return [-1, 0, 0, 0, -1, 0, -1, 0]
    frames = [g for g in range(G) if s0 <= HOP * g + FIRST < s1]
    if frames:
        g0, g1 = frames[0], frames[-1] + 1
    else:
        m = (s0 + s1) // 2
        g0 = min(range(G), key=lambda g: (abs(HOP * g + FIRST - m), -g))    # m exactly between two centres (m = 270 g + 630): the later one
        g1 = g0 + 1
    v, u = {}, {}
    for g in range(g0, g1):
        on = named(speakers[g], K)
        for k in on:
            v[k] = v.get(k, 0) + 1
            if len(on) == 1:
                u[k] = u.get(k, 0) + 1
    order = sorted(v, key=lambda k: (-v[k], -u.get(k, 0), k))
    if order:
        a = order[0]
        b = order[1] if len(order) > 1 else -1
        return [a, v[a], u.get(a, 0), g1 - g0, b, v[b] if b >= 0 else 0, 0, g0]
    for d in range(1, gap + 1):
        for g in (g0 - d, g1 - 1 + d):                                       # the earlier side first
            if 0 <= g < G:
                on = named(speakers[g], K)
                if on:
                    return [on[0], 0, 0, g1 - g0, -1, 0, d, g0]
    return [-1, 0, 0, g1 - g0, -1, 0, -1, g0]


def attribute_ref(speakers, K: int, words, gap: int) -> np.ndarray:
    """speakers [G][2], words [(s0, s1)] in samples -> rows [W, 8] int32."""
    sp = [[int(a), int(b)] for a, b in np.asarray(speakers).reshape(-1, 2)]
    return np.asarray([attribute_word(sp, K, int(s0), int(s1), gap) for s0, s1 in words], dtype=np.int32).reshape(-1, 8)


def best_assignment(co) -> int:
    """The maximum of sum co[i, m(i)] over injective partial maps, by trying every one (small tables only)."""
    co = [[int(x) for x in row] for row in co]
    S, K = len(co), len(co[0]) if co else 0
    if S == 0 or K == 0:
        return 0
    if S > K:
        co, S, K = [list(c) for c in zip(*co)], K, S
    return max(sum(co[i][j] for i, j in enumerate(perm)) for perm in itertools.permutations(range(K), S))


def wder_ref(hyp, reference, K: int, exact: bool = True):
    """hyp [W] speakers (-1: none), reference [W] labels (None, "UU": not scored) -> dict(names, co, scored, unassigned, words, correct, wder);
    correct by brute force (exact=False leaves it out: tables too large to enumerate)."""
    names = []
    for lab in reference:
        if lab is not None and lab != "UU" and lab not in names:
            names.append(lab)
    co = [[0] * K for _ in names]
    scored = unassigned = 0
    for h, lab in zip(hyp, reference):
        if lab is None or lab == "UU":
            continue
        scored += 1
        if 0 <= int(h) < K:
            co[names.index(lab)][int(h)] += 1
        else:
            unassigned += 1
    out = dict(names=names, co=np.asarray(co, dtype=np.int32).reshape(len(names), K), scored=scored, unassigned=unassigned, words=len(hyp))
    if exact:
        out["correct"] = best_assignment(co)
        out["wder"] = 0.0 if scored == 0 else 1.0 - out["correct"] / scored
    return out


# ------------------------------------------------------------------------------------------------ generated inputs
def random_speakers(rng, G: int, K: int) -> np.ndarray:
    """[G, 2] int32 in runs: silence, one speaker, two speakers, and now and then a doubled name or an entry >= K."""
    sp = np.full((G, 2), -1, np.int32)
    g = 0
    while g < G:
        n = int(rng.integers(1, 60))
        kind = int(rng.integers(0, 10))
        if K and kind >= 3:
            a = int(rng.integers(0, K))
            sp[g:g + n, 0] = a
            if kind >= 7:
                sp[g:g + n, 1] = int(rng.integers(0, K)) if kind < 9 else (a if kind == 9 and rng.integers(0, 2) else K + int(rng.integers(0, 3)))
            if kind == 6:
                sp[g:g + n] = sp[g:g + n, ::-1]                           # the speaker in the second entry, the first empty
        g += n
    return sp


def random_words(rng, G: int, W: int):
    """W words in samples over (and a little past) a recording of G frames: real-word lengths, a few points and a few long spans."""
    end = HOP * G + FIRST + 2000
    out = []
    for _ in range(W):
        s0 = int(rng.integers(0, max(end, 1)))
        kind = int(rng.integers(0, 10))
        n = 0 if kind == 0 else int(rng.integers(1, 200)) if kind == 1 else int(rng.integers(20000, 60000)) if kind == 2 else int(rng.integers(800, 9000))
        out.append((s0, s0 + n))
    return out


# ------------------------------------------------------------------------------------------------ the edge packs both test files run
def centre(g: int) -> int:
    return HOP * g + FIRST


def cover(a: int, b: int):
    """The word whose frames are exactly a <= g < b."""
    return (centre(a), centre(b - 1) + 1)


def at(g: int):
    """A zero-length word on the centre of frame g: no centre lies in [s, s), the nearest frame is g."""
    return (centre(g), centre(g))


def table(G: int, fill=None) -> np.ndarray:
    sp = np.full((G, 2), -1, np.int32)
    for g, entry in (fill or {}).items():
        sp[g] = entry
    return sp


def runs(G: int, *spans) -> np.ndarray:
    """spans: (from, to, (h0, h1))."""
    sp = np.full((G, 2), -1, np.int32)
    for a, b, entry in spans:
        sp[a:b] = entry
    return sp


def edge_packs():
    """{name: (gap in frames, [(speakers [G, 2], K, [(s0, s1)])] one entry per recording)}: every edge the rule names, at the smallest shapes."""
    packs = {}
    packs["no_frames"] = (29, [(table(0), 2, [(0, 100), (5000, 9000), (7, 7)])])
    packs["empty_middle"] = (29, [(runs(50, (0, 50, (0, -1))), 1, [cover(3, 9), cover(40, 50)]), (runs(40, (0, 40, (1, 0))), 2, []),
                                  (runs(30, (5, 30, (1, -1))), 2, [cover(0, 3), cover(4, 30)])])
    packs["no_speakers"] = (29, [(runs(30, (0, 30, (0, 1))), 0, [cover(2, 8), at(4)]), (runs(30, (0, 30, (0, 1))), 2, [cover(2, 8)])])
    # before sample 495, past the last centre, zero length, 100 samples between two centres, a midpoint half way between two centres
    sp = runs(20, (0, 1, (1, -1)), (5, 6, (0, -1)), (6, 7, (2, -1)), (19, 20, (3, -1)))
    packs["points"] = (0, [(sp, 4, [(0, 400), (100, 494), (centre(25), centre(25) + 3000), (centre(19) + 1, centre(19) + 50), (3000, 3000),
                                    (1900, 2000), (1970, 1990), (centre(5) + 1, centre(6)), (centre(5), centre(5) + 1), (2000, 1900)])])
    # spans of exactly 63, 64, 65, 128, 129 and 5 000 frames over a table that changes every few frames
    G = 5200
    sp = np.full((G, 2), -1, np.int32)
    g = np.arange(G)
    sp[:, 0] = np.where(g % 11 < 8, (g // 13) % 5, -1)
    sp[:, 1] = np.where(g % 7 < 2, (g // 5) % 5, -1)
    packs["spans"] = (29, [(sp, 5, [cover(10, 10 + n) for n in (1, 2, 18, 63, 64, 65, 128, 129, 5000)] + [cover(100, 5200), (0, centre(G) + 999)])])
    packs["ties"] = (29, [
        (table(3, {0: (0, 1), 1: (0, 2), 2: (1, -1)}), 3, [cover(0, 3)]),             # v0 = v1 = 2, u1 = 1 > u0 = 0: speaker 1, second 0
        (table(2, {0: (2, 1), 1: (1, 2)}), 3, [cover(0, 2)]),                         # v and u equal: the lower id, 1
        (table(3, {0: (3, 3), 1: (3, 3), 2: (3, 3)}), 4, [cover(0, 3)]),              # named twice: once, and alone
        (table(3, {0: (5, 1), 1: (2, 1), 2: (-1, 0)}), 2, [cover(0, 3), cover(1, 2)]),   # 5 and 2 name nobody with K = 2
    ])
    sp = runs(200, (100, 101, (-1, 0)))
    packs["gap_edge"] = (29, [(sp, 1, [at(71), at(70), at(129), at(130), cover(60, 72), cover(60, 71), cover(129, 140), cover(130, 140)])])
    packs["gap_zero"] = (0, [(runs(20, (5, 6, (0, -1))), 1, [at(4), at(6), at(5)])])
    packs["gap_sides"] = (29, [(runs(100, (50, 51, (1, -1)), (60, 61, (0, -1))), 2, [at(55), cover(54, 57), at(56), at(54)])])
    # a silent word at the first and at the last frame of the middle recording; the neighbours' adjacent frames are voiced
    packs["neighbours"] = (29, [(runs(30, (0, 30, (0, -1))), 2, [cover(28, 30)]), (runs(40, (20, 21, (1, -1))), 2, [at(0), at(39), cover(0, 2), cover(37, 40)]),
                                (runs(30, (0, 30, (0, -1))), 2, [cover(0, 2)]),
                                (runs(30, (0, 30, (0, -1))), 1, [at(29)]), (table(40), 2, [at(0), at(39)]), (runs(30, (0, 30, (0, -1))), 1, [at(0)])])
    packs["gap_long"] = (100, [(runs(300, (150, 151, (0, 1)), (299, 300, (1, -1))), 2, [at(60), at(49), at(50), at(220), at(240), at(224), at(225)])])
    for K in (1, 64, 65, 1024):
        lo = max(K - 2, 0)
        sp = runs(12, (0, 5, (lo, K - 1)), (5, 8, (K - 1, -1)), (8, 10, (lo, -1)), (11, 12, (K, -1)))
        packs[f"speakers_{K}"] = (29, [(sp, K, [cover(0, 12), cover(0, 5), cover(8, 10), at(11)])])
    return packs


def random_pack(seed: int, K_choices=(0, 1, 3, 64, 200), R: int = 5, max_frames: int = 2000, max_words: int = 300):
    rng = np.random.default_rng(seed)
    recs = []
    for r in range(R):
        G, K = int(rng.integers(1, max_frames + 1)), int(rng.choice(K_choices))
        recs.append((random_speakers(rng, G, K), K, random_words(rng, G, int(rng.integers(0, max_words + 1)))))
    return int(rng.integers(0, 80)), recs


def random_reference(rng, W: int, S: int):
    """W reference labels over S names, with None and "UU" among them."""
    pool = [f"spk{i}" for i in range(S)] + [None, "UU"]
    return [pool[int(rng.integers(0, len(pool)))] for _ in range(W)]
