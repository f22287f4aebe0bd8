"""The fusion rule of fuse.py restated frame by frame in plain Python loops (Python integers; no numpy in the rule itself, and nothing of
fuse.py's host path: only score.assignment_host, the exact assignment that has its own tests, is borrowed for `correct`), and the packs the
CPU and GPU tests of the fusion share: the hand-worked cases of every step and seeded random packs."""
from __future__ import annotations

import numpy as np

from conftest import sub

sc = sub("score")

B = 256                                        # fuse.FUSE_BLOCK_FRAMES
RANK_WEIGHTS = [int(65536 * (k + 1) ** -0.1) for k in range(8)]   # recomputed here; test_fuse_cpu compares the module's literals with it
MAX_LABELS = 64


def pair_list(H):
    return [(a, b) for a in range(H) for b in range(a + 1, H)]


def bits_of(m: int, K: int) -> list:
    return [k for k in range(min(K, 64)) if (int(m) >> k) & 1]


def masks_ref(speakers, K: int) -> list:
    out = []
    for row in np.asarray(speakers).reshape(-1, 2).tolist():
        m = 0
        for x in row:
            if 0 <= x < K:
                m |= 1 << x
        out.append(m)
    return out


def fuse_ref(masks, frame_off, K, weights=None, cap=2) -> dict:
    """masks [H][G] (anything int() takes), frame_off [R + 1], K [H][R] -> the tables of fuse.fuse_host, by the same names."""
    H, R = len(K), len(frame_off) - 1
    pl = pair_list(H)
    P = len(pl)
    G = int(frame_off[-1])
    out = {"speakers": [[-1, -1] for _ in range(G)], "tallies": [], "dis": [], "order": [], "weight": [], "n_labels": [], "overflow": []}
    label_flat = {}
    co_q, tally_q, correct_q, map_q = {}, {}, {}, {}
    for r in range(R):
        g0, g1 = int(frame_off[r]), int(frame_off[r + 1])
        Kr = [int(K[h][r]) for h in range(H)]
        act = [[bits_of(masks[h][g], Kr[h]) for g in range(g0, g1)] for h in range(H)]
        # 1 pairs
        co = {}
        for p, (a, b) in enumerate(pl):
            t = [[0] * Kr[b] for _ in range(Kr[a])]
            smax = smin = 0
            for f in range(g1 - g0):
                for i in act[a][f]:
                    for j in act[b][f]:
                        t[i][j] += 1
                smax += max(len(act[a][f]), len(act[b][f]))
                smin += min(len(act[a][f]), len(act[b][f]))
            mapping, correct = sc.assignment_host(np.asarray(t, dtype=np.int64).reshape(Kr[a], Kr[b]))
            co[(a, b)] = t
            q = p * R + r
            co_q[q], tally_q[q], correct_q[q], map_q[q] = t, [smax, smin], int(correct), [int(x) for x in mapping]
        # 2 rank
        dis = [[0] * H for _ in range(H)]
        for p, (a, b) in enumerate(pl):
            dis[a][b] = dis[b][a] = tally_q[p * R + r][0] - correct_q[p * R + r]
        order = sorted(range(H), key=lambda h: (sum(dis[h]), h))
        w = [0] * H
        for rank, h in enumerate(order):
            w[h] = int(weights[h]) if weights is not None else RANK_WEIGHTS[rank]
        # 3 labels
        label = [[-1] * Kr[h] for h in range(H)]
        label[order[0]] = list(range(Kr[order[0]]))
        L, overflow = Kr[order[0]], 0
        for k in range(1, H):
            h = order[k]
            A = [[0] * Kr[h] for _ in range(L)]
            for hp in order[:k]:
                for i in range(Kr[hp]):
                    u = label[hp][i]
                    if u < 0:
                        continue
                    for j in range(Kr[h]):
                        A[u][j] += co[(hp, h)][i][j] if hp < h else co[(h, hp)][j][i]
            used_u, done_j = set(), set()
            while True:
                best = None
                for u in range(L):
                    for j in range(Kr[h]):
                        if u in used_u or j in done_j or A[u][j] <= 0:
                            continue
                        if best is None or A[u][j] > best[0]:               # scanned in (u, j) order: a tie keeps the earlier
                            best = (A[u][j], u, j)
                if best is None:
                    break
                label[h][best[2]] = best[1]
                used_u.add(best[1])
                done_j.add(best[2])
            for j in range(Kr[h]):
                if j in done_j:
                    continue
                if L < MAX_LABELS:
                    label[h][j] = L
                    L += 1
                else:
                    overflow += 1
        for h in range(H):
            assert len({u for u in label[h] if u >= 0}) == sum(u >= 0 for u in label[h])      # two speakers of one hypothesis never share a label
            label_flat[(h, r)] = label[h]
        # 4 vote, 5 tallies
        W = sum(w)
        speech = overlap = unanimous = 0
        for f in range(g1 - g0):
            seen = [{label[h][i] for i in act[h][f] if label[h][i] >= 0} for h in range(H)]
            v = {}
            for h in range(H):
                for u in seen[h]:
                    v[u] = v.get(u, 0) + w[h]
            n = min(cap, (2 * sum(w[h] * len(act[h][f]) for h in range(H)) + W) // (2 * W))
            ranked = sorted(v, key=lambda u: (-v[u], u))[:n]
            out["speakers"][g0 + f] = (ranked + [-1, -1])[:2]
            speech += len(ranked) >= 1
            overlap += len(ranked) >= 2
            unanimous += all(s == seen[0] for s in seen)
        out["tallies"].append([speech, overlap, unanimous, overflow])
        out["dis"].append(dis), out["order"].append(order), out["weight"].append(w), out["n_labels"].append(L), out["overflow"].append(overflow)
    out["speakers"] = np.asarray(out["speakers"], np.int32).reshape(G, 2)
    out["tallies"] = np.asarray(out["tallies"], np.int64).reshape(R, 4)
    out["dis"] = np.asarray(out["dis"], np.int64).reshape(R, H, H)
    out["order"], out["weight"] = np.asarray(out["order"], np.int32).reshape(R, H), np.asarray(out["weight"], np.int32).reshape(R, H)
    out["n_labels"], out["overflow"] = np.asarray(out["n_labels"], np.int32), np.asarray(out["overflow"], np.int32)
    out["label_of"] = np.asarray([u for h in range(H) for r in range(R) for u in label_flat[(h, r)]], np.int32)
    out["co"] = np.asarray([x for q in range(P * R) for row in co_q[q] for x in row], np.int32)
    out["tally"] = np.asarray([tally_q[q] for q in range(P * R)], np.int64).reshape(P * R, 2)
    out["correct"] = np.asarray([correct_q[q] for q in range(P * R)], np.int64)
    out["mapping"] = np.asarray([x for q in range(P * R) for x in map_q[q]], np.int32)
    return out


EXACT = ("speakers", "tallies", "dis", "order", "weight", "label_of", "n_labels", "overflow", "co", "tally", "correct")   # `mapping` is any optimal map


def same(got: dict, want: dict, names=EXACT):
    """Exact integer equality of the named tables (shape and every element) -> the first name that differs, or None."""
    for n in names:
        g, w = np.asarray(got[n]), np.asarray(want[n])
        if g.shape != w.shape or not np.array_equal(g.astype(np.int64), w.astype(np.int64)):
            return n
    return None


# ------------------------------------------------------------------------------------------------ packs
def to_masks(rows) -> np.ndarray:
    """[H][G] lists of speaker lists -> uint64 [H, G]."""
    return np.asarray([[sum(1 << k for k in ks) for ks in row] for row in rows], dtype=np.uint64).reshape(len(rows), -1)


def pack(rows_per_recording, K):
    """rows_per_recording[r][h][g] = the speakers hypothesis h names in frame g of recording r; K [H][R] -> (masks [H, G], frame_off, K)."""
    H = len(K)
    masks = np.concatenate([to_masks(rec) for rec in rows_per_recording], axis=1) if rows_per_recording else np.zeros((H, 0), np.uint64)
    frame_off = np.concatenate([[0], np.cumsum([len(rec[0]) for rec in rows_per_recording])]).astype(np.int64)
    return masks, frame_off, np.asarray(K, dtype=np.int64).reshape(H, -1)


def case_transpose():
    """order puts the higher h first: hypothesis 2 agrees with both others more than they agree with each other, so it is the anchor and
    the pair tables (0, 2) and (1, 2) are read transposed.  Hypothesis 2 numbers the two speakers the other way round."""
    a = [[0]] * 6 + [[1]] * 6 + [[0]] * 2
    b = [[0]] * 5 + [[1]] * 7 + [[]] * 2
    c = [[1]] * 6 + [[0]] * 6 + [[]] * 2
    # dis(a, b) = 1 confusion + 2 count = 3, dis(a, c) = 2, dis(b, c) = 1: D = (5, 4, 3)
    return pack([[a, b, c]], [[2], [2], [2]])


def case_overflow():
    """Three hypotheses of 40 speakers each, disjoint in time: nothing co-occurs, 64 labels, overflow 56."""
    rows = [[[] for _ in range(120)] for _ in range(3)]
    for h in range(3):
        for i in range(40):
            rows[h][40 * h + i] = [i]
    return pack([rows], [[40], [40], [40]])


def case_greedy_tie():
    """A[0][0] = A[0][1] = A[1][0] = 2 frames, A[1][1] = 0: the lowest u, then the lowest j wins (0, 0); then only A[1][1] = 0 is left, so
    speaker 1 of hypothesis 1 gets the new label 2."""
    a = [[0], [0], [0], [0], [1], [1]]
    b = [[0], [0], [1], [1], [0], [0]]
    return pack([[a, b]], [[2], [2]])


def random_pack(seed: int, H: int, G_r, K_choices=(0, 1, 2, 5, 64), stray: bool = True):
    """Masks with 0 to 4 bits a frame in runs of 1 .. 12 frames, K mixed across hypotheses and recordings, stray bits at or above K."""
    rng = np.random.default_rng(seed)
    R = len(G_r)
    K = rng.choice(np.asarray(K_choices), size=(H, R))
    G = int(sum(G_r))
    masks = np.zeros((H, G), np.uint64)
    off = np.concatenate([[0], np.cumsum(G_r)]).astype(np.int64)
    for r in range(R):
        truth = np.zeros(int(G_r[r]), np.int64)                         # a shared activity pattern, so that the hypotheses have something to agree on
        g = 0
        while g < G_r[r]:
            n = int(rng.integers(1, 13))
            truth[g:g + n] = int(rng.integers(0, 5))
            g += n
        for h in range(H):
            k = int(K[h, r])
            perm = rng.permutation(max(k, 1))
            for f in range(int(G_r[r])):
                m = 0
                n_bits = int(truth[f]) if rng.random() < 0.8 else int(rng.integers(0, 5))
                for i in range(n_bits):
                    if k:
                        m |= 1 << int(perm[(int(truth[f]) + i + (0 if rng.random() < 0.85 else int(rng.integers(0, k)))) % k])
                if stray and k < 64 and rng.random() < 0.1:
                    m |= 1 << int(rng.integers(k, 64))
                masks[h, off[r] + f] = np.uint64(m)
    return masks, off, K.astype(np.int64)


EDGE_FRAMES = [0, 1, B - 1, B, B + 1, 3 * B + 7]                      # a workgroup starts, ends and crosses recordings; one recording is empty
