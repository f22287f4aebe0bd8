"""An independent reference for samples.py: the runs of solo frames as a plain per-frame walk over Python integers (not the grouped
restatement samples.runs_host, and not the device's scan), the clip scores as per-clip loops with math.fsum.  Imports nothing from the
product; the generated hypothesis tables are words_ref's."""
from __future__ import annotations

import math

import numpy as np

import words_ref as WR

HOP, RATE = WR.HOP, WR.RATE
WAVE, WORKGROUP, SPAN = 64, 256, 2048          # the widths the device scan is built from (csrc/samples.hip: SM_NT, SM_SPAN)


def min_frames(min_s: float) -> int:
    return max(1, -(-WR.to_samples(min_s) // HOP))


def kind_of(entry, K: int) -> int:
    """-1 silent, -2 overlapped, k when the frame names exactly {k}."""
    on = WR.named(entry, K)
    return -1 if not on else on[0] if len(on) == 1 else -2


def runs_ref(speakers, K: int, gap: int, min_fr: int) -> np.ndarray:
    """speakers [G][2] -> rows [N, 4] int32 (speaker, g0, g1, solo): walk the frames, and from every solo frame walk its run."""
    kinds = [kind_of((int(a), int(b)), K) for a, b in np.asarray(speakers).reshape(-1, 2)]
    G, rows, g = len(kinds), [], 0
    while g < G:
        k = kinds[g]
        if k < 0:
            g += 1
            continue
        end, solo, silent, h = g + 1, 1, 0, g + 1
        while h < G:
            if kinds[h] == k:
                end, solo, silent = h + 1, solo + 1, 0
            elif kinds[h] == -1:
                silent += 1
                if silent > gap:
                    break
            else:
                break
            h += 1
        if solo >= min_fr:
            rows.append((k, g, end, solo))
        g = end
    return np.asarray(rows, dtype=np.int32).reshape(-1, 4)


def pack_ref(gap: int, min_fr: int, recs):
    """-> (run_off [R + 1] int32, rows [N, 4] int32) of a pack [(speakers, K)]."""
    per = [runs_ref(sp, K, gap, min_fr) for sp, K in recs]
    off = np.concatenate([[0], np.cumsum([len(p) for p in per])]).astype(np.int32)
    return off, np.concatenate(per).astype(np.int32).reshape(-1, 4)


# ------------------------------------------------------------------------------------------------ scores
def _dot(a, b) -> float:
    return math.fsum(float(x) * float(y) for x, y in zip(a, b))


def score_ref(E, clip_off, clip_spk, spk_off):
    """-> dict(mean [S, d], own [M], rival [M], rival_speaker [M], windows [M], alone [M], rest_ratio [M] = |m_s - c_i| / |m_s| (inf where m_s
    is 0), rival_gap [M] = best minus second-best rival cosine (inf with fewer than two)).  Every sum is a math.fsum of float64 values."""
    E = np.asarray(E, dtype=np.float64)
    M, S, d = len(clip_spk), int(spk_off[-1]), E.shape[1]
    c = [[math.fsum(E[w, j] for w in range(int(clip_off[i]), int(clip_off[i + 1]))) for j in range(d)] for i in range(M)]
    m, n_win = [], []
    for s in range(S):
        mine = [i for i in range(M) if int(clip_spk[i]) == s]
        m.append([math.fsum(c[i][j] for i in mine) for j in range(d)])
        n_win.append(sum(int(clip_off[i + 1] - clip_off[i]) for i in mine))
    out = dict(mean=np.asarray([[x / n for x in row] if n else [0.0] * d for row, n in zip(m, n_win)], dtype=np.float64).reshape(S, d),
               own=np.zeros(M), rival=np.zeros(M), rival_speaker=np.full(M, -1, np.int32), windows=np.zeros(M, np.int32), alone=np.zeros(M, np.int32),
               rest_ratio=np.full(M, np.inf), rival_gap=np.full(M, np.inf))
    m_norm = [math.sqrt(_dot(row, row)) for row in m]
    for i in range(M):
        s = int(clip_spk[i])
        r = max(q for q in range(len(spk_off) - 1) if int(spk_off[q]) <= s)
        rest = [a - b for a, b in zip(m[s], c[i])]
        nc, nr = math.sqrt(_dot(c[i], c[i])), math.sqrt(_dot(rest, rest))
        out["windows"][i] = int(clip_off[i + 1] - clip_off[i])
        if nc == 0.0 or nr == 0.0:
            out["alone"][i] = 1
        else:
            out["own"][i] = _dot(c[i], rest) / (nc * nr)
            out["rest_ratio"][i] = nr / m_norm[s]
        if nc == 0.0:
            continue
        cands = sorted(((-_dot(c[i], m[t]) / (nc * m_norm[t]), t) for t in range(int(spk_off[r]), int(spk_off[r + 1])) if t != s and m_norm[t] > 0.0))
        if cands:
            out["rival"][i], out["rival_speaker"][i] = -cands[0][0], cands[0][1] - int(spk_off[r])
            if len(cands) > 1:
                out["rival_gap"][i] = cands[1][0] - cands[0][0]
    return out


def score_case(seed: int, d: int, layout, max_windows: int = 12):
    """layout: per recording a list over its speakers of the windows of every clip (None: draw 1 .. max_windows), e.g. [[None], [3, 0, None]].
    The clips of a recording are dealt to its speakers in turn (interleaved).  Unit fp32 rows: a direction per speaker plus noise.
    -> (E [W, d] fp32, clip_off [M + 1], clip_spk [M], spk_off [R + 1])."""
    rng = np.random.default_rng(seed)
    spk_off = np.concatenate([[0], np.cumsum([len(rec) for rec in layout])]).astype(np.int64)
    clip_spk, counts = [], []
    for r, rec in enumerate(layout):
        for pos in range(max((len(cl) for cl in rec), default=0)):
            for k, cl in enumerate(rec):
                if pos < len(cl):
                    clip_spk.append(int(spk_off[r]) + k)
                    counts.append(int(rng.integers(1, max_windows + 1)) if cl[pos] is None else int(cl[pos]))
    base = rng.standard_normal((int(spk_off[-1]), d))
    base /= np.linalg.norm(base, axis=1, keepdims=True)
    rows = []
    for s, n in zip(clip_spk, counts):
        x = base[s] + 0.6 * rng.standard_normal((n, d)) / np.sqrt(d)
        rows.append(x / np.linalg.norm(x, axis=1, keepdims=True))
    E = np.concatenate(rows).astype(np.float32) if rows else np.zeros((0, d), np.float32)
    return E, np.concatenate([[0], np.cumsum(counts)]).astype(np.int64), np.asarray(clip_spk, np.int64), spk_off


# a speaker with one clip (alone), a clip without windows, a recording with one speaker, interleaved clips, a speaker without any clip
SCORE_LAYOUT = [[[None], [None, None, 0, None], [None, None, None]], [[None, None, None]], [[None, None], [], [None, None, None, None], [None, None], [5, 7]]]
SCORE_CASES = {64: (41, 64, SCORE_LAYOUT, 190), 192: (42, 192, SCORE_LAYOUT, 12), 256: (43, 256, SCORE_LAYOUT, 12), 512: (44, 512, SCORE_LAYOUT, 8)}
# the widths at which a second column is live for a part of the workgroup only (ss_clip_sum's blockDim = 256 with columns tid + 256 q, ss_score's
# lane + 64 q with 5 and 7 of 8 registers live), at the fewest windows the layout allows: one per drawn clip, beside its clips of 5, 7 and 0
SCORE_CASES.update({320: (45, 320, SCORE_LAYOUT, 1), 448: (46, 448, SCORE_LAYOUT, 1)})


def second_column_weight(name: str, E, clip_off, clip_spk, spk_off, ref: dict, bound: float = 1e-12) -> float:
    """partial_width.weight of a score case wider than 256 columns: score_ref without the columns 256.. of the rows against `ref`."""
    import partial_width as PW
    cut = score_ref(PW.first_columns(E), clip_off, clip_spk, spk_off)
    return PW.weight(name, ints=[(ref[q], cut[q]) for q in ("rival_speaker", "windows", "alone")], floats=[(ref[q], cut[q]) for q in ("mean", "own", "rival")],
                     bound=bound)


# ------------------------------------------------------------------------------------------------ the packs both test files run
def filled(rng, G: int, K: int) -> np.ndarray:
    return WR.random_speakers(rng, G, K)


def edge_packs():
    """{name: (gap frames, min_frames, [(speakers [G, 2], K)] one entry per recording)}: every case the rule and the scan name."""
    runs, table = WR.runs, WR.table
    rng = np.random.default_rng(5)
    packs = {}
    packs["no_frames_one_frame"] = (3, 1, [(table(0), 2), (table(1, {0: (0, -1)}), 1), (table(0), 0), (table(1), 1), (table(1, {0: (1, 0)}), 2)])
    packs["silent_overlapped_solo"] = (3, 1, [(table(100), 2), (runs(100, (0, 100, (0, 1))), 2), (runs(100, (0, 100, (1, -1))), 2)])
    sp = runs(12, (0, 4, (1023, -1)), (4, 6, (1023, 1022)), (6, 9, (-1, 1022)), (9, 12, (1024, -1)))
    packs["speakers_0_1_1024"] = (2, 1, [(runs(30, (0, 30, (0, -1))), 0), (runs(30, (3, 20, (0, -1)), (20, 25, (1, -1))), 1), (sp, 1024)])
    # a run that ends on the last frame of a recording, the next recording begins solo for the same local speaker: never joined
    packs["neighbours"] = (29, 1, [(runs(40, (30, 40, (0, -1))), 2), (runs(50, (0, 7, (0, -1)), (45, 50, (1, -1))), 2), (table(0), 2),
                                   (runs(20, (0, 20, (-1, 1))), 2), (table(5), 1), (runs(9, (2, 3, (0, -1))), 1)])
    packs["gap_exact"] = (5, 1, [(runs(40, (2, 6, (0, -1)), (11, 15, (0, -1))), 1), (runs(40, (2, 6, (0, -1)), (12, 15, (0, -1))), 1),
                                 (runs(40, (0, 1, (0, -1)), (6, 7, (0, -1)), (13, 14, (0, -1)), (19, 20, (0, -1))), 1)])
    packs["gap_zero"] = (0, 1, [(runs(20, (2, 6, (0, -1)), (6, 9, (0, 0)), (10, 12, (0, -1))), 1), (runs(8, (0, 8, (-1, 0))), 1), (table(6, {1: (0, -1), 3: (0, -1)}), 1)])
    # entries >= K and < -1 name nobody: (2, 0) and (-5, 0) are solo for 0, (7, -3) is silent, (2, 2) is silent
    packs["nobody_entries"] = (1, 1, [(table(10, {0: (2, 0), 1: (-5, 0), 2: (7, -3), 3: (0, 9), 5: (2, 2), 6: (1, -2), 7: (1, 1), 8: (-1, 1), 9: (1, 0)}), 2),
                                      (table(4, {0: (0, -1), 1: (3, 1), 2: (-7, -7), 3: (1, 3)}), 3), (table(3, {0: (5, 5), 1: (4, -1)}), 4)])
    packs["forms"] = (0, 1, [(table(6, {0: (1, 1), 1: (1, -1), 2: (-1, 1), 3: (0, 0), 4: (-1, 0), 5: (0, -1)}), 2), (table(3, {0: (0, 0), 1: (0, 1), 2: (1, 1)}), 2),
                             (table(2, {0: (-1, 0), 1: (0, -1)}), 1)])
    # solo == min_frames kept, min_frames - 1 dropped; a dropped run between two kept ones; silent frames do not count as solo
    packs["min_frames"] = (2, 4, [(runs(30, (0, 5, (0, -1)), (5, 8, (1, -1)), (8, 12, (0, -1)), (14, 16, (0, -1)), (20, 23, (1, -1))), 2),
                                  (runs(20, (0, 2, (0, -1)), (4, 5, (0, -1)), (10, 14, (1, -1))), 2), (runs(10, (0, 3, (0, -1))), 1)])
    packs["single_frames"] = (0, 1, [(table(9, {0: (0, -1), 2: (1, -1), 4: (0, 1), 5: (0, -1), 8: (2, -1)}), 3), (table(3, {1: (0, -1)}), 1), (table(2, {0: (0, 0), 1: (1, 1)}), 2)])
    for name, w in (("wave", WAVE), ("workgroup", WORKGROUP), ("span", SPAN)):
        packs[f"sizes_{name}"] = (7, 3, [(filled(rng, n, 3), 3) for n in (w - 1, w, w + 1)] + [(runs(w + 1, (0, w + 1, (0, -1))), 1), (runs(w, (w - 1, w, (0, -1))), 1)])
    # one run over more than three scan blocks (pauses of at most gap inside), another recording's boundary inside a block, then one more long run
    G = 3 * SPAN + 700
    sp = np.full((G, 2), -1, np.int32)
    sp[5:G - 3, 0] = 1
    sp[np.arange(40, G - 40, 97)[:, None] + np.arange(4)[None, :], 0] = -1
    packs["long_run"] = (4, 30, [(runs(1000, (100, 900, (0, -1))), 1), (sp, 2), (runs(700, (0, 700, (-1, 2))), 3), (sp[::-1][:, ::-1].copy(), 2)])
    return packs


def random_pack(seed: int, K_choices=(0, 1, 3, 5, 64), R: int = 5, max_frames: int = 3000):
    rng = np.random.default_rng(seed)
    recs = [(WR.random_speakers(rng, int(rng.integers(1, max_frames + 1)), K), K) for K in (int(rng.choice(K_choices)) for _ in range(R))]
    return int(rng.integers(0, 70)), int(rng.integers(1, 40)), recs
