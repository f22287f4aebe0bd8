"""Test-side checker of the diarization's assignment stage (diarize.py "assignment" and "constrained assignment"; sdk_diarize_centroids,
sdk_diarize_assign): the stated rule in loop form, float64, written from the rule and sharing no code with diarize.py.

  centroids     per cluster, its training rows added one by one in ascending row order, divided by the count, divided by the norm
  cosines       one float64 dot product per (candidate row, centroid)
  constrained   per chunk, EVERY map of the candidates to clusters is formed (n = min(m, K) candidates get pairwise different clusters, the
                other m - n get -1), its total summed in slot order; the largest total wins, ties to the smallest label tuple in slot
                order with -1 after every cluster.  No use is made of "a row's m largest cosines suffice".  The loop over maps is plain Python
                while a chunk has at most PLAIN_MAPS tuples; above that (K = 40 or 300 with three candidates: up to 2.7e7 maps per chunk) the
                loop over the first candidate's cluster stays and the other one or two run as numpy axes - the same totals, formed in the
                same order, every one of them, and numpy's first maximum in C order IS the smallest label tuple.
                tests/test_diarize_assign_cpu.py checks the two forms against each other where both run.
  margin        per chunk, the decisive margin: the best total minus the best total of a map with a different label tuple (infinity when
                there is no other map).  Unconstrained: the least best-minus-second cosine of the chunk's candidates.
"""
from __future__ import annotations

import itertools

import numpy as np

PLAIN_MAPS = 4096


def candidates(info):
    flat = np.asarray(info).reshape(-1, 4)
    return [r for r in range(flat.shape[0]) if flat[r, 3] != 0 and flat[r, 0] > 0]


def centroids(E, info, train_rows, train_labels):
    """-> float64 unit centroids [K, d] ([0, d] when there is neither a training row nor a candidate)."""
    d = np.asarray(E).shape[1]
    if len(train_rows):
        groups = [[r for r, lab in zip(train_rows, train_labels) if lab == k] for k in range(int(max(train_labels)) + 1)]
    else:
        cand = candidates(info)
        groups = [cand] if cand else []
    out = []
    for rows in groups:
        m = np.zeros(d)
        for r in rows:
            m = m + np.asarray(E[r], np.float64)
        m = m / len(rows)
        out.append(m / max(np.linalg.norm(m), 1e-300))
    return np.stack(out) if out else np.zeros((0, d))


def chunk_plain(cos):
    """cos [m][K] -> (labels tuple, total, margin): every map in a plain loop."""
    m, K = len(cos), len(cos[0])
    n = min(m, K)
    found = []
    for lab in itertools.product(list(range(K)) + [-1], repeat=m):
        used = [k for k in lab if k >= 0]
        if len(used) != n or len(set(used)) != n:
            continue
        tot = 0.0
        for i in range(m):
            if lab[i] >= 0:
                tot = tot + cos[i][lab[i]]
        found.append((tot, tuple(k if k >= 0 else K for k in lab), lab))
    best = None
    for f in found:
        if best is None or f[0] > best[0] or (f[0] == best[0] and f[1] < best[1]):
            best = f
    others = [f[0] for f in found if f[2] != best[2]]
    return best[2], best[0], (best[0] - max(others)) if others else np.inf


def chunk_axes(cos):
    """The same for K >= m >= 2: plain loop over the first candidate's cluster, the other candidates as numpy axes."""
    cos = np.asarray(cos, np.float64)
    m, K = cos.shape
    assert K >= m >= 2
    best, second = None, -np.inf
    diag = np.arange(K)
    for k0 in range(K):
        if m == 2:
            tot = cos[0, k0] + cos[1]                                          # [K]
            tot[k0] = -np.inf                                                  # not a map: a cluster used twice
        else:
            tot = (cos[0, k0] + cos[1])[:, None] + cos[2][None, :]             # [K, K]: (c0 + c1) + c2, slot order
            tot[k0, :] = -np.inf
            tot[:, k0] = -np.inf
            tot[diag, diag] = -np.inf
        j = int(np.argmax(tot))                                                # first maximum in C order: the smallest (k1, k2)
        v = float(tot.flat[j])
        tot.flat[j] = -np.inf
        runner = float(tot.max()) if tot.size > 1 else -np.inf
        lab = (k0,) + tuple(int(x) for x in np.unravel_index(j, tot.shape))
        if best is None or v > best[0]:                                        # k0 ascends: a tie keeps the earlier, smaller tuple
            if best is not None:
                second = max(second, best[0])
            best = (v, lab)
            second = max(second, runner)
        else:
            second = max(second, v)
    return best[1], best[0], (best[0] - second) if second > -np.inf else np.inf


def assign(E, info, train_rows, train_labels, constrained=True, cent=None):
    """-> dict(labels [C, 3] int32, centroids [K, d] float64, score [C, 3] float64 (cosine of each assigned row, 0 where -1),
    total [C] (sum of the chunk's assigned cosines), margin [C] (decisive margin, inf without a second map), m [C] candidates per chunk,
    bites [C] bool: two candidates of the chunk share their nearest centroid).  cent: centroids to use instead of the training rows'."""
    flat = np.asarray(info).reshape(-1, 4)
    Cn = flat.shape[0] // 3
    cent = centroids(E, info, train_rows, train_labels) if cent is None else np.asarray(cent, np.float64)
    K = cent.shape[0]
    labels = np.full((Cn, 3), -1, np.int32)
    score = np.zeros((Cn, 3))
    total, margin = np.zeros(Cn), np.full(Cn, np.inf)
    ms, bites = np.zeros(Cn, np.int64), np.zeros(Cn, bool)
    for c in range(Cn):
        slots = [s for s in range(3) if flat[3 * c + s, 3] != 0 and flat[3 * c + s, 0] > 0]
        ms[c] = len(slots)
        if not slots or K == 0:
            continue
        cos = [[float(np.dot(np.asarray(E[3 * c + s], np.float64), cent[k])) for k in range(K)] for s in slots]
        near = []
        for row in cos:
            b = 0
            for k in range(1, K):
                if row[k] > row[b]:
                    b = k
            near.append(b)
        bites[c] = len(set(near)) < len(near)
        if not constrained:
            lab, gaps = near, []
            for row, b in zip(cos, near):
                others = [row[k] for k in range(K) if k != b]
                gaps.append(row[b] - max(others) if others else np.inf)
            mg = min(gaps)
        elif len(slots) == 1 or (K + 1) ** len(slots) <= PLAIN_MAPS or K < len(slots):
            lab, _, mg = chunk_plain(cos)
        else:
            lab, _, mg = chunk_axes(cos)
        tot = 0.0
        for i, s in enumerate(slots):
            labels[c, s] = lab[i]
            if lab[i] >= 0:
                score[c, s] = cos[i][lab[i]]
                tot = tot + cos[i][lab[i]]
        total[c], margin[c] = tot, mg
    return dict(labels=labels, centroids=cent, score=score, total=total, margin=margin, m=ms, bites=bites)


def make_case(seed, Cn, K, d=192, noise=0.25, p_bite=0.3, train_per_cluster=3, nan_fill=True):
    """Seeded inputs for the assignment: K unit centres; every candidate row is a centre plus noise, normalised in float64 and rounded to
    fp32; chunks with 0, 1, 2 and 3 candidates (weights 1 : 3 : 5 : 1; chunk 0 has three); in chunk 0, and with probability p_bite
    elsewhere, two candidates of a chunk come from the same centre; rows that are no candidates hold NaN.  Training rows:
    train_per_cluster extra chunks per centre with one clean speaker each, appended BEHIND the Cn chunks (C' = Cn + K train_per_cluster) so
    that every cluster has rows.  -> (E [3 C', d] fp32, info [C', 3, 4] int32, train rows, labels)"""
    rng = np.random.default_rng(seed)
    centres = rng.standard_normal((K, d))
    centres /= np.linalg.norm(centres, axis=1, keepdims=True)
    Ct = Cn + K * train_per_cluster
    E = np.full((3 * Ct, d), np.nan if nan_fill else 0.0, np.float32)
    info = np.zeros((Ct, 3, 4), np.int32)

    def row(k):
        v = centres[k] + noise * rng.standard_normal(d) / np.sqrt(d)
        return (v / np.linalg.norm(v)).astype(np.float32)
    for c in range(Cn):
        m = 3 if c == 0 else int(rng.choice(4, p=[0.1, 0.3, 0.5, 0.1]))
        slots = sorted(rng.choice(3, m, replace=False).tolist())
        ks = rng.integers(0, K, m)
        if m >= 2 and (c == 0 or rng.random() < p_bite):
            ks[1] = ks[0]
        for s, k in zip(slots, ks):
            E[3 * c + s] = row(int(k))
            info[c, s] = (int(rng.integers(1, 500)), int(rng.integers(0, 100)), 1, 1)
        for s in set(range(3)) - set(slots):                                   # the ways of not being a candidate
            info[c, s] = [(0, 0, 0, 0), (0, 0, 0, 1), (40, 0, 0, 0)][int(rng.integers(0, 3))]
    train, tl = [], []
    for k in range(K):
        for t in range(train_per_cluster):
            c = Cn + k * train_per_cluster + t
            E[3 * c] = row(k)
            info[c, 0] = (300, 300, 1, 1)
            train.append(3 * c)
            tl.append(k)
    return E, info, np.array(train, np.int64), np.array(tl, np.int32)
