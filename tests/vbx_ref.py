"""Test-side checker of the VBx clustering (cluster.vbx_cluster, plda.py, csrc/vbx.hip): the stated rule in numpy loops and plain sums, written
from the statement and sharing no code with the package.

Every sum runs term by term in index order: sums over dimensions ascending, sums over rows ascending or - reverse=True - descending, which is
what a different summation order over the rows costs.  dtype is np.float64 or np.longdouble; every decision (the stop test, the kept
speakers, the hard labels) is taken in that dtype.  The prepared model (Phi, T) comes in as float64 values and is widened exactly.
"""
from __future__ import annotations

import numpy as np

LN_2PI = "1.837877066409345483560659472811235279722794947275566825634303080965531391854520"
MIN_PI = 1e-7


def _unit_rows(v, dtype):
    q = np.zeros(v.shape[0], dtype)
    for j in range(v.shape[1]):
        q = q + v[:, j] * v[:, j]
    return v / np.maximum(np.sqrt(q), dtype("1e-300"))[:, None]


def transform(E, mean1, lda, mean2, mu, T, dtype=np.float64):
    """E [n, d_in] fp32 unit rows, T [D, D0] -> X [n, D]:  x1 = sqrt(d_in) unit(e - mean1);  x2 = sqrt(D0) unit(lda^T x1 - mean2);
    x = ((x2 - mu) T^T)[:D]."""
    E, mean1, lda, mean2, mu, T = (np.asarray(a).astype(dtype) for a in (E, mean1, lda, mean2, mu, T))
    d_in, D0 = lda.shape
    x1 = np.sqrt(dtype(d_in)) * _unit_rows(E - mean1[None, :], dtype)
    y = np.zeros((E.shape[0], D0), dtype)
    for i in range(d_in):
        y = y + x1[:, i, None] * lda[i][None, :]
    x2 = np.sqrt(dtype(D0)) * _unit_rows(y - mean2[None, :], dtype)
    z = x2 - mu[None, :]
    X = np.zeros((E.shape[0], T.shape[0]), dtype)
    for k in range(D0):
        X = X + z[:, k, None] * T[:, k][None, :]
    return X


def _row_order(n, reverse):
    return range(n - 1, -1, -1) if reverse else range(n)


def vbx(X, Phi, init_labels, S, Fa=0.07, Fb=0.8, max_iters=20, epsilon=1e-4, init_smoothing=7.0, dtype=np.float64, reverse=False):
    """-> dict(gamma [n, S], pi [S], elbo [n_iter], n_iter), all in dtype."""
    X, Phi = np.asarray(X).astype(dtype), np.asarray(Phi).astype(dtype)
    n, D = X.shape
    Fa, Fb, eps = dtype(Fa), dtype(Fb), dtype(epsilon)
    half = dtype(1) / dtype(2)
    rho = X * np.sqrt(Phi)[None, :]
    x2 = np.zeros(n, dtype)
    for d in range(D):
        x2 = x2 + X[:, d] * X[:, d]
    G = -half * (x2 + dtype(D) * dtype(LN_2PI))
    # gamma0 = softmax_s(init_smoothing [label == s]), the maximum subtracted
    a = np.zeros((n, S), dtype)
    a[np.arange(n), np.asarray(init_labels)] = dtype(init_smoothing)
    a = np.exp(a - a.max(1)[:, None])
    den = np.zeros(n, dtype)
    for s in range(S):
        den = den + a[:, s]
    gamma = a / den[:, None]
    pi = np.full(S, dtype(1) / dtype(S), dtype)
    elbo = []
    fab = Fa / Fb
    for ii in range(max_iters):
        N = np.zeros(S, dtype)
        F = np.zeros((S, D), dtype)
        for t in _row_order(n, reverse):
            N = N + gamma[t]
            F = F + gamma[t][:, None] * rho[t][None, :]
        invL = dtype(1) / (dtype(1) + fab * N[:, None] * Phi[None, :])
        alpha = fab * invL * F
        dot = np.zeros((n, S), dtype)
        for d in range(D):
            dot = dot + rho[:, d, None] * alpha[:, d][None, :]
        c = np.zeros(S, dtype)
        e2 = np.zeros(S, dtype)
        for d in range(D):
            c = c + (invL[:, d] + alpha[:, d] * alpha[:, d]) * Phi[d]
            e2 = e2 + (np.log(invL[:, d]) - invL[:, d] - alpha[:, d] * alpha[:, d] + dtype(1))
        logp = Fa * (dot - half * c[None, :] + G[:, None])
        with np.errstate(divide="ignore"):
            z = logp + np.log(pi)[None, :]                                # pi == 0: -inf
        m = z.max(1)
        se = np.zeros(n, dtype)
        for s in range(S):
            se = se + np.exp(z[:, s] - m)
        lse = m + np.log(se)
        gamma = np.exp(z - lse[:, None])
        L = dtype(0)
        for t in _row_order(n, reverse):
            L = L + lse[t]
        tail = dtype(0)
        for s in range(S):
            tail = tail + e2[s]
        elbo.append(L + half * Fb * tail)
        Ng = np.zeros(S, dtype)
        for t in _row_order(n, reverse):
            Ng = Ng + gamma[t]
        tot = dtype(0)
        for s in range(S):
            tot = tot + Ng[s]
        pi = Ng / tot
        if ii > 0 and elbo[-1] - elbo[-2] < eps:
            break
    return dict(gamma=gamma, pi=pi, elbo=np.array(elbo, dtype), n_iter=len(elbo))


def result(gamma, pi, E, dtype=np.float64, reverse=False):
    """-> dict(keep [K], labels [n] over the kept speakers (ties to the lower), cent [K, d] unit): the speakers with pi > 1e-7 and their
    centroids sum_t gamma[t, k] e_t / sum_t gamma[t, k] over the original rows, re-normalised.  A kept speaker without any weight has the zero
    centroid; with no speaker kept every label is -1."""
    gamma, E = np.asarray(gamma).astype(dtype), np.asarray(E).astype(dtype)
    n, d = E.shape
    keep = [s for s in range(len(pi)) if pi[s] > dtype(MIN_PI)]
    cent = np.zeros((len(keep), d), dtype)
    for k, s in enumerate(keep):
        acc = np.zeros(d, dtype)
        w = dtype(0)
        for t in _row_order(n, reverse):
            acc = acc + gamma[t, s] * E[t]
            w = w + gamma[t, s]
        if w > 0:
            acc = acc / w
        q = dtype(0)
        for j in range(d):
            q = q + acc[j] * acc[j]
        cent[k] = acc / max(np.sqrt(q), dtype("1e-300"))
    labels = np.zeros(n, np.int32)
    for t in range(n):
        best = 0
        for k in range(1, len(keep)):
            if gamma[t, keep[k]] > gamma[t, keep[best]]:
                best = k
        labels[t] = best if keep else -1
    return dict(keep=np.array(keep, np.int32), labels=labels, cent=cent)


# ------------------------------------------------------------------------------------------------ generated mixtures
def _on_sphere(centre, dirs, radius):
    """Per row: the point centre + a dir / |dir| with a > 0 and norm `radius` (|centre| < radius)."""
    u = dirs / np.linalg.norm(dirs, axis=1, keepdims=True)
    b = u @ centre
    a = -b + np.sqrt(b * b + radius * radius - centre @ centre)
    return centre[None, :] + a[:, None] * u


def mixture(seed, N, d_in, D0, D, S, n_true, plda_arrays, T_full):
    """A mixture in PLDA space carried back to unit embeddings: n_true speaker means drawn at scale sqrt(Phi) (all D0 dimensions), rows
    x ~ N(mean, I), mapped back through the inverse of the transform's linear parts (its two length normalisations only rescale), and the true
    speakers split at random into S >= n_true initial clusters.  plda_arrays = (mean1, lda, mean2, mu, Phi_full [D0]); lda has orthonormal
    columns.  -> (E [R, d_in] fp32 unit rows with R > N, rows [N] ascending strict subset, init_labels [N] int32 in [0, S), true [N])."""
    mean1, lda, mean2, mu, Phi_full = plda_arrays
    rng = np.random.default_rng(seed)
    R = N + max(3, N // 5)
    rows = np.sort(rng.choice(R, N, replace=False)).astype(np.int32)
    true_all = rng.integers(0, n_true, R)
    true_all[rows[:min(n_true, N)]] = np.arange(min(n_true, N))           # every speaker has a row (when N allows)
    means = rng.standard_normal((n_true, D0)) * np.sqrt(Phi_full)[None, :]
    x = means[true_all] + rng.standard_normal((R, D0))
    y = mu[None, :] + x @ np.linalg.inv(T_full).T                         # x = (y - mu) T^T
    x1 = _on_sphere(mean2, y, np.sqrt(d_in)) @ lda.T                       # lda^T x1 - mean2 is parallel to y, |x1| = sqrt(d_in)
    E = _on_sphere(mean1, x1, 1.0).astype(np.float32)                      # e - mean1 is parallel to x1, |e| = 1
    true = true_all[rows]
    # split: initial cluster s belongs to true speaker s % n_true; a speaker's rows are dealt to its clusters in turn
    init = np.zeros(N, np.int32)
    for v in range(n_true):
        mine = rng.permutation(np.arange(v, S, n_true)) if v < S else np.array([v % S])
        idx = np.flatnonzero(true == v)
        init[idx] = mine[np.arange(len(idx)) % len(mine)]
    return E, rows, init, true
