"""Float64 reference of the adaptive score normalisation (AS-norm) rule, written from the rule's statement and sharing no code with snorm.py:
a full sort per row, np.mean, np.std, the floor, z, a stable argsort for ties, and the aggregation of per-window winners into result rows.

  cohort statistics of x : the K largest of the M cosines <x, c_j> (a multiset); their mean and population standard deviation, the latter
                           floored at STD_FLOOR
  z(n, p)                : ((s - mean(e_n)) / std(e_n) + (s - mean(p)) / std(p)) / 2, s = <e_n, p>
  top-k                  : the k largest z per window, ties to the lowest profile index, NaN never wins; nothing finite: idx -1, z 0, raw 0
  aggregation            : a window votes for the speaker of its top-1 row when z >= threshold; similarity = mean raw cosine of the votes,
                           norm_score = mean z of the votes; rows by norm_score descending, then speaker id
"""
import numpy as np

STD_FLOOR = 1e-6


def cosines(A, B):
    return np.asarray(A, dtype=np.float64) @ np.asarray(B, dtype=np.float64).T


def cohort_stats(E, cohort, K):
    S = cosines(E, cohort)
    mean, std = np.empty(len(S)), np.empty(len(S))
    for n, row in enumerate(S):
        top = np.sort(row)[::-1][:K]
        mean[n] = np.mean(top)
        std[n] = max(float(np.std(top)), STD_FLOOR) if not np.isnan(top).any() else np.nan
    return mean, std


def second_column_weight_stats(name, E, cohort, K, ref, bound):
    """partial_width.weight of a statistics case wider than 256 columns: cohort_stats without the columns 256.. of the rows against ref = (mean, std)."""
    import partial_width as PW
    cut = cohort_stats(PW.first_columns(E), cohort, K)
    return PW.weight(name, floats=list(zip(ref, cut)), bound=bound)


def second_column_weight_topk(name, E, mean_e, std_e, P, mean_p, std_p, k, ref, bound):
    """The same for topk: ref = topk's tuple on the full rows; the indices as integers, z against `bound` (the largest element bound in use)."""
    import partial_width as PW
    cut = topk(PW.first_columns(E), mean_e, std_e, P, mean_p, std_p, k)
    return PW.weight(name, ints=[(ref[0], cut[0])], floats=[(ref[1], cut[1]), (ref[2], cut[2])], bound=bound)


def zscores(E, mean_e, std_e, P, mean_p, std_p):
    S = cosines(E, P)
    Z = np.empty_like(S)
    with np.errstate(invalid="ignore", divide="ignore"):
        for n in range(S.shape[0]):
            for p in range(S.shape[1]):
                s = S[n, p]
                Z[n, p] = 0.5 * ((s - float(mean_e[n])) / float(std_e[n]) + (s - float(mean_p[p])) / float(std_p[p]))
    return Z, S


def topk(E, mean_e, std_e, P, mean_p, std_p, k):
    """(idx [N, k] int32, z [N, k], raw [N, k], Z [N, Pn], S [N, Pn])"""
    Z, S = zscores(E, mean_e, std_e, P, mean_p, std_p)
    N = Z.shape[0]
    idx, z, raw = np.full((N, k), -1, np.int32), np.zeros((N, k)), np.zeros((N, k))
    for n in range(N):
        ok = [p for p in range(Z.shape[1]) if not np.isnan(Z[n, p])]
        ok.sort(key=lambda p: -Z[n, p])                      # list.sort is stable: equal z keep ascending p
        for j, p in enumerate(ok[:k]):
            idx[n, j], z[n, j], raw[n, j] = p, Z[n, p], S[n, p]
    return idx, z, raw, Z, S


def aggregate(best_idx, best_z, best_raw, spans, speaker_ids, embedding_ids, threshold):
    votes = {}
    for w in range(len(best_idx)):
        row = int(best_idx[w])
        if row < 0 or not float(best_z[w]) >= threshold:
            continue
        votes.setdefault(speaker_ids[row], []).append((w, row))
    rows = []
    for sid, vs in votes.items():
        count = {}
        for _, row in vs:
            count[row] = count.get(row, 0) + 1
        most = max(count.values())
        win = min(r for r, c in count.items() if c == most)
        sim = float(np.mean(np.array([best_raw[w] for w, _ in vs], dtype=np.float64)))
        rows.append({"speaker_id": sid, "similarity": sim, "confidence": sim,
                     "norm_score": float(np.mean(np.array([best_z[w] for w, _ in vs], dtype=np.float64))), "embedding_id": embedding_ids[win],
                     "segment": (spans[vs[0][0]][0], spans[vs[-1][0]][1]), "n_segments": len(vs)})
    return sorted(rows, key=lambda r: (-r["norm_score"], r["speaker_id"]))
