"""An independent float64 reference of the PLDA log-likelihood-ratio scoring (plda_score.py states the rule) for tests/test_plda_score_*.py.
It shares no code with the package: the score is written in Kaldi's direct form (the predictive Gaussian of a window given the speaker's
pooled enrolments, minus the marginal Gaussian, two log-densities subtracted), the pooling and the top-k are plain loops, and
`llr_joint` evaluates, per dimension, the joint Gaussian of (x, u_1 .. u_n) with slogdet / solve - it never sees a pooled mean.
"""
from __future__ import annotations

import math

import numpy as np

LOG_2PI = math.log(2.0 * math.pi)


def pool(Xp, group, S):
    """(mean [S, D] of every speaker's rows, added in ascending row order; m [S] their number).  Labels outside [0, S) belong to nobody."""
    Xp = np.asarray(Xp, dtype=np.float64)
    sums = np.zeros((S, Xp.shape[1]))
    m = np.zeros(S, np.int64)
    for p in range(Xp.shape[0]):
        s = int(group[p])
        if 0 <= s < S:
            sums[s] = sums[s] + Xp[p]
            m[s] += 1
    return sums / np.maximum(m, 1)[:, None], m


def valid(m, n_eff):
    n_eff = np.asarray(n_eff, dtype=np.float64)
    return (m > 0) & np.isfinite(n_eff) & (n_eff > 0)


def log_normal(x, mean, var):
    """sum_d ln N(x_d | mean_d, var_d)."""
    return float(-0.5 * np.sum(LOG_2PI + np.log(var) + (x - mean) ** 2 / var))


def llr_direct(X, U, m, n_eff, Phi):
    """[N, S]: ln N(x | n Phi / (n Phi + 1) u, 1 + Phi / (n Phi + 1)) - ln N(x | 0, 1 + Phi); NaN for a speaker that is not valid."""
    X, U, Phi = np.asarray(X, dtype=np.float64), np.asarray(U, dtype=np.float64), np.asarray(Phi, dtype=np.float64)
    ok = valid(m, n_eff)
    L = np.full((X.shape[0], U.shape[0]), np.nan)
    for s in range(U.shape[0]):
        if not ok[s]:
            continue
        n = float(n_eff[s])
        mean = n * Phi / (n * Phi + 1.0) * U[s]
        var = 1.0 + Phi / (n * Phi + 1.0)
        for i in range(X.shape[0]):
            L[i, s] = log_normal(X[i], mean, var) - log_normal(X[i], 0.0, 1.0 + Phi)
    return L


def llr_joint(x, rows, Phi):
    """The same ratio for n = len(rows) enrolment rows, from the model itself: per dimension (x, u_1 .. u_n) is Gaussian with covariance
    Phi_d 1 1^T + I, and the ratio is ln p(x, u) - ln p(x) - ln p(u)."""
    x, rows, Phi = np.asarray(x, dtype=np.float64), np.asarray(rows, dtype=np.float64), np.asarray(Phi, dtype=np.float64)
    n = rows.shape[0]

    def logp(vec, phi):
        k = len(vec)
        C = phi * np.ones((k, k)) + np.eye(k)
        return -0.5 * (k * LOG_2PI + np.linalg.slogdet(C)[1] + vec @ np.linalg.solve(C, vec))

    out = 0.0
    for d in range(x.shape[0]):
        joint = np.concatenate([[x[d]], rows[:, d]])
        out += logp(joint, Phi[d]) - logp(joint[:1], Phi[d]) - logp(joint[1:], Phi[d])
    assert n >= 1
    return float(out)


def table(Xp, group, n_eff, Phi):
    """(G [S, 2 D], r [S], U [S, D], m [S]): the speaker table, speaker by speaker."""
    Phi = np.asarray(Phi, dtype=np.float64)
    n_eff = np.asarray(n_eff, dtype=np.float64)
    S, D = len(n_eff), len(Phi)
    U, m = pool(Xp, group, S)
    ok = valid(m, n_eff)
    G, r = np.zeros((S, 2 * D)), np.full(S, np.nan)
    for s in range(S):
        if not ok[s]:
            continue
        n = float(n_eff[s])
        a = n * Phi / (n * Phi + 1.0)
        v = 1.0 + Phi / (n * Phi + 1.0)
        G[s, :D] = a / v * U[s]
        G[s, D:] = -0.5 * (1.0 / v - 1.0 / (1.0 + Phi))
        r[s] = float(np.sum(-0.5 * (np.log(v) - np.log(1.0 + Phi)) - (a * U[s]) ** 2 / (2.0 * v)))
    return G, r, U, m


def two_prod(a, b):
    """a * b = p + e exactly, element by element (Veltkamp's split and Dekker's product; no overflow at these magnitudes)."""
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    p = a * b

    def split(v):
        c = 134217729.0 * v                                   # 2^27 + 1
        hi = c - (c - v)
        return hi, v - hi
    ah, al = split(a)
    bh, bl = split(b)
    return p, ((ah * bh - p) + ah * bl + al * bh) + al * bl


def llr_table(X, G, r):
    """[N, S] from a table, CORRECTLY ROUNDED: every term x_d G[s, d] and x_d^2 G[s, D + d] is expanded into doubles whose sum is the exact
    product (two_prod; x^2 = hi + lo, each times G), and math.fsum rounds the exact sum of all of them and r_s once.  A row with a
    non-finite entry gives NaN."""
    X, G, r = np.asarray(X, dtype=np.float64), np.asarray(G, dtype=np.float64), np.asarray(r, dtype=np.float64)
    N, D = X.shape
    L = np.full((N, G.shape[0]), np.nan)
    for i in range(N):
        if not np.isfinite(X[i]).all():
            continue
        sq, sq_lo = two_prod(X[i], X[i])
        parts = two_prod(X[i][None, :], G[:, :D]) + two_prod(sq[None, :], G[:, D:]) + two_prod(sq_lo[None, :], G[:, D:])
        terms = np.concatenate(parts + (r[:, None],), axis=1)
        fin = np.isfinite(terms).all(axis=1)
        for s, row in enumerate(terms.tolist()):
            if fin[s]:
                L[i, s] = math.fsum(row)
    return L


def magnitude(X, G, r):
    """A [N, S] = |r_s| + sum_d (|x_d G[s, d]| + |x_d^2 G[s, D + d]|): what the rounding errors of a score scale with."""
    X = np.asarray(X, dtype=np.float64)
    D = X.shape[1]
    with np.errstate(invalid="ignore"):
        return np.abs(r)[None, :] + np.abs(X) @ np.abs(G[:, :D]).T + (X * X) @ np.abs(G[:, D:]).T


def topk(L, k):
    """(idx [N, k] int32, score [N, k]): the k largest per row, ties to the lower column, a NaN never taken, (-1, 0) where nothing is left."""
    N, S = L.shape
    idx, sc = np.full((N, k), -1, np.int32), np.zeros((N, k))
    for i in range(N):
        ok = [s for s in range(S) if L[i, s] == L[i, s]]
        ok.sort(key=lambda s: -L[i, s])                      # list.sort is stable: equal scores keep ascending s
        for j, s in enumerate(ok[:k]):
            idx[i, j], sc[i, j] = s, L[i, s]
    return idx, sc


def sigmoid(l):
    return 1.0 / (1.0 + math.exp(-l)) if l >= 0 else math.exp(l) / (1.0 + math.exp(l))


def aggregate(best_idx, best_llr, spans, speaker_ids, embedding_ids, threshold):
    """Result rows from per-window winners.  speaker_ids / embedding_ids: one per PROFILE ROW of the batch, in batch order; best_idx counts
    speakers in order of first appearance."""
    order = []
    for sid in speaker_ids:
        if sid not in order:
            order.append(sid)
    rows = {}
    for w in range(len(best_idx)):
        s, l = int(best_idx[w]), float(best_llr[w])
        if s < 0 or math.isnan(l) or l < threshold:
            continue
        rows.setdefault(order[s], []).append((l, spans[w]))
    out = []
    for sid, hits in rows.items():
        llr = sum(np.float64(h[0]) for h in hits) / np.float64(len(hits))
        mine = [i for i, x in enumerate(speaker_ids) if x == sid]
        out.append({"speaker_id": sid, "llr": float(llr), "similarity": sigmoid(float(llr)), "confidence": sigmoid(float(llr)),
                    "embedding_id": embedding_ids[mine[0]], "n_embeddings": len(mine), "segment": (hits[0][1][0], hits[-1][1][1]),
                    "n_segments": len(hits)})
    return sorted(out, key=lambda r: (-r["llr"], r["speaker_id"]))


def planted(rng, N, S, D, Phi, rows_per=(1, 5)):
    """Planted inputs: speaker centres ~ N(0, Phi), 1 - 5 enrolment rows each at unit noise, interleaved over the speakers; window n at unit
    noise around speaker n mod S -> (X [N, D], Xp [P, D], group [P] int32, counts [S])."""
    Phi = np.asarray(Phi, dtype=np.float64)
    centres = rng.standard_normal((S, D)) * np.sqrt(Phi)
    counts = rng.integers(rows_per[0], rows_per[1] + 1, size=S)
    group = rng.permutation(np.repeat(np.arange(S), counts)).astype(np.int32)
    Xp = centres[group] + rng.standard_normal((len(group), D))
    X = centres[np.arange(N) % S] + rng.standard_normal((N, D))
    return np.ascontiguousarray(X), np.ascontiguousarray(Xp), group, counts
