"""numpy float64 restatements for the speaker-count bounds (`speakers=`): the k-means rule of cluster.kmeans_cluster with every sum in the
stated order, the level search of cluster.agglomerative_cluster rule 7 written as loops, its brute-force reference (one flat partition per
level), the bounds' target, and diarize_ref's host pipeline extended with both."""
from __future__ import annotations

import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import ahc_ref as AHC  # noqa: E402
import partial_width as PW  # noqa: E402

SEGMENT = 1024                    # rows per segment of the centre sums (cluster.KMEANS_SEGMENT)


def dot_in_order(A: np.ndarray, B: np.ndarray) -> np.ndarray:
    """A [m, d], B [K, d] float64 -> [m, K]: every entry one sum over the columns in ascending order."""
    acc = np.zeros((A.shape[0], B.shape[0]))
    for j in range(A.shape[1]):
        acc += A[:, j, None] * B[None, :, j]
    return acc


def seeds(X: np.ndarray, k: int):
    """Maximin: row 0, then the row whose largest cosine to the seeds so far is smallest (first minimum: the lowest row)."""
    rows, maxcos = [0], None
    for _ in range(1, k):
        cos = dot_in_order(X, X[rows[-1]][None])[:, 0]
        maxcos = cos if maxcos is None else np.maximum(maxcos, cos)
        rows.append(int(np.argmin(maxcos)))
    return rows


def sums_in_order(X: np.ndarray, labels: np.ndarray, k: int):
    """s [k, d], counts [k]: per segment of SEGMENT rows the rows of a label added in ascending order from 0.0 (cumsum is sequential), then
    the segments' partials added in segment order from 0.0."""
    N, d = X.shape
    s, cnt = np.zeros((k, d)), np.zeros(k, np.int64)
    for t0 in range(0, N, SEGMENT):
        lab = labels[t0:t0 + SEGMENT]
        for c in range(k):
            idx = t0 + np.flatnonzero(lab == c)
            part = np.cumsum(X[idx], axis=0)[-1] if idx.size else np.zeros(d)
            s[c] = s[c] + part
            cnt[c] += idx.size
    return s, cnt


def canonical(lab):
    return AHC.canonical(lab)


def kmeans(E32: np.ndarray, k: int, max_iters: int = 20, rows=None) -> dict:
    """The rule of cluster.kmeans_cluster on fp32 rows -> dict(labels canonical, raw, n_clusters, n_iter, counts, cent64 [K, d] unit,
    margins: per iteration the [N] best-minus-second cosines (inf at k = 1), least: the least of them all)."""
    X = np.asarray(E32, np.float32)[np.arange(len(E32)) if rows is None else np.asarray(rows)].astype(np.float64)
    if not np.isfinite(X).all():
        raise ValueError("non-finite row")
    N = X.shape[0]
    C = X[seeds(X, k)].copy()
    labels, margins, n_iter = np.full(N, -1), [], 0
    for it in range(max_iters):
        cos = dot_in_order(X, C)
        cos = np.where(cos == cos, cos, -np.inf)                          # a NaN never wins
        new = np.argmax(cos, axis=1)                                      # first maximum: the lower centre
        srt = np.sort(cos, axis=1)
        margins.append(srt[:, -1] - srt[:, -2] if k > 1 else np.full(N, np.inf))
        changed = bool((new != labels).any())
        labels, n_iter = new, it + 1
        if (it >= 1 and not changed) or it + 1 == max_iters:
            break
        s, cnt = sums_in_order(X, labels, k)
        nrm = np.sqrt((s * s).sum(1))
        ok = (cnt > 0) & (nrm > 0)
        C[ok] = s[ok] / nrm[ok, None]
    can = canonical(labels)
    K = int(can.max()) + 1
    cent = np.zeros((K, X.shape[1]))
    for c in range(K):
        idx = np.flatnonzero(can == c)
        cent[c] = np.cumsum(X[idx], axis=0)[-1] / idx.size               # sdk_diarize_centroids: ascending rows, then the mean
    cent /= np.linalg.norm(cent, axis=1, keepdims=True)
    return dict(labels=can, raw=labels, n_clusters=K, n_iter=n_iter, counts=np.bincount(can, minlength=K), cent64=cent, margins=margins,
                least=float(min(m.min() for m in margins)))


def second_column_weight(name: str, E32: np.ndarray, k: int, cent_bound: float, ref: dict = None, **kw) -> float:
    """partial_width.weight for kmeans on rows wider than 256: the labels and counts without the columns 256.. against those of `ref` (the run on
    the full rows), the unit centres against cent_bound."""
    ref = kmeans(E32, k, **kw) if ref is None else ref
    cut = kmeans(PW.first_columns(E32), k, **kw)
    return PW.weight(name, ints=[(ref["labels"], cut["labels"]), (ref["counts"], cut["counts"])], floats=[(ref["cent64"], cut["cent64"])], bound=cent_bound)


# ------------------------------------------------------------------------------------------------ bounds and the level search
def target_of(found: int, lo, hi, n_rows: int):
    """None when the count found stands, else the count to force (lo / hi: ints or None)."""
    lo = 1 if lo is None else lo
    if n_rows < 2 or (found >= lo and (hi is None or found <= hi)):
        return None
    return min(max(lo if found < lo else hi, 1), n_rows)


def eff_size(min_cluster_size: int, N: int) -> int:
    return min(min_cluster_size, max(1, round(0.1 * N)))


def cut_merges(Z: np.ndarray, threshold: float) -> int:
    for t in range(Z.shape[0]):
        if Z[t, 2] > threshold:
            return t
    return Z.shape[0]


def level_counts(Z: np.ndarray, eff: int):
    """L[t], t = 0 .. N - 1, in one pass over the sizes in Z."""
    N = Z.shape[0] + 1
    size = {i: 1 for i in range(N)}
    L = [N if 1 >= eff else 0]
    for t in range(N - 1):
        a, b = int(Z[t, 0]), int(Z[t, 1])
        size[N + t] = int(Z[t, 3])
        L.append(L[-1] + int(size[N + t] >= eff) - int(size[a] >= eff) - int(size[b] >= eff))
    return L


def pick_level(L, t0: int, target: int) -> int:
    return min(range(len(L)), key=lambda t: (abs(L[t] - target), abs(t - t0), t))


def level_search(Z: np.ndarray, eff: int, t0: int, target: int) -> int:
    return pick_level(level_counts(Z, eff), t0, target)


def level_search_brute(Z: np.ndarray, eff: int, t0: int, target: int, partition) -> int:
    """One flat partition per level (partition(Z, N, t) -> labels), the sizes counted, the same tuple."""
    N = Z.shape[0] + 1
    return pick_level([int((np.bincount(partition(Z, N, t)) >= eff).sum()) for t in range(N)], t0, target)


def fold(E: np.ndarray, lab: np.ndarray, min_cluster_size: int) -> np.ndarray:
    """Rules 1 - 4 of cluster.agglomerative_cluster on a flat partition, as ahc_ref.threshold_rule folds the cut."""
    N = len(lab)
    eff = eff_size(min_cluster_size, N)
    K = int(lab.max()) + 1
    sizes = [int((lab == c).sum()) for c in range(K)]
    large = [c for c in range(K) if sizes[c] >= eff]
    if not large:
        return np.zeros(N, np.int32)
    E = np.asarray(E, np.float64)
    cent = {c: E[lab == c].mean(axis=0) for c in range(K)}
    out = lab.copy()
    for c in range(K):
        if sizes[c] >= eff:
            continue
        best, bd = None, None
        for g in large:
            dist = 1.0 - cent[c] @ cent[g] / (np.linalg.norm(cent[c]) * np.linalg.norm(cent[g]))
            if bd is None or dist < bd:
                best, bd = g, dist
        out[lab == c] = best
    return AHC.canonical(out)


def ahc_bounded(Z: np.ndarray, E_train: np.ndarray, threshold: float, min_cluster_size: int, lo, hi):
    """-> (labels, forced or None): the threshold rule, then the level search when the count lies outside lo .. hi."""
    N = E_train.shape[0]
    lab = AHC.threshold_rule(Z, E_train, threshold, min_cluster_size)
    found = int(lab.max()) + 1
    target = target_of(found, lo, hi, N)
    if target is None:
        return lab, None
    eff = eff_size(min_cluster_size, N)
    level = level_search(Z, eff, cut_merges(Z, threshold), target)
    out = fold(E_train, AHC.partition_after(Z, N, level), min_cluster_size)
    return out, dict(found=found, target=target, method="level", level=level, n_iter=None, reachable=target in level_counts(Z, eff))
