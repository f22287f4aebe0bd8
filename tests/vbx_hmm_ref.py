"""Test-side checker of VBx with its HMM (cluster.vbx_cluster(loop_prob > 0), sdk_vbx_hmm): the stated rule in numpy loops over the rows, written
from the statement and sharing no code with the package.  The signature style is vbx_ref.vbx's.

The chain runs row by row.  Every sum over speakers runs term by term (np.cumsum's last element: a strictly sequential sum) in ascending
order, every sum over rows in a Python loop in ascending order; reverse=True turns both around, which is what a different summation order
costs.  dtype is np.float64 or np.longdouble; every decision is taken in that dtype.  jitter=seed moves the result of every exp, log and log1p
by one ulp with a seeded random sign: what a differently rounded exp / log costs once the chain has compounded it over n steps.
"""
from __future__ import annotations

import numpy as np

LN_2PI = "1.837877066409345483560659472811235279722794947275566825634303080965531391854520"


class _Fn:
    """exp, log, log1p in dtype; with a seed, every result moved by one ulp up or down."""

    def __init__(self, dtype, jitter=None):
        self.dtype = dtype
        self.rng = None if jitter is None else np.random.default_rng(jitter)

    def _move(self, v):
        if self.rng is None:
            return v
        v = np.asarray(v, self.dtype)
        up = self.rng.integers(0, 2, v.shape).astype(bool)
        inf = self.dtype(np.inf)
        out = np.where(up, np.nextafter(v, inf), np.nextafter(v, -inf))
        return np.where(np.isfinite(v) & (v != 0), out, v).astype(self.dtype)      # -inf, 0 (an exact result) and NaN stay

    def exp(self, v):
        return self._move(np.exp(v))

    def log(self, v):
        with np.errstate(divide="ignore"):
            return self._move(np.log(v))

    def log1p(self, v):
        return self._move(np.log1p(v))


def _seq_sum(v, reverse):
    """The sum of a vector term by term, ascending (descending with reverse)."""
    return np.cumsum(v[::-1] if reverse else v)[-1]


def _logaddexp(a, b, fn):
    """max + log1p(exp(min - max)); an argument of -inf returns the other exactly; both -inf: -inf."""
    hi, lo = np.maximum(a, b), np.minimum(a, b)
    with np.errstate(invalid="ignore"):
        d = lo - hi                                                       # NaN where both are -inf
    out = hi + fn.log1p(fn.exp(np.where(np.isnan(d), -np.inf, d)))
    return np.where(hi == -np.inf, hi, out)


def _lse(u, fn, reverse):
    mx = u.max()
    return mx + fn.log(_seq_sum(fn.exp(u - mx), reverse))


def forward_backward(logp, pi, loop_prob, dtype=np.float64, reverse=False, fn=None):
    """One pass of the chain -> dict(lf, lb [n, S], m [n], tll, gamma [n, S], pinew [S] (not normalised))."""
    fn = fn or _Fn(dtype)
    n, S = logp.shape
    P = dtype(loop_prob)
    lnP, ln1mP = fn.log(P), fn.log1p(-P)
    if P == 0:
        lnP, ln1mP = dtype(-np.inf), dtype(0)                             # exact whatever the jitter
    lnpi = fn.log(pi)                                                     # pi == 0: -inf
    c = ln1mP + lnpi
    lf = np.zeros((n, S), dtype)
    lb = np.zeros((n, S), dtype)
    m = np.zeros(n, dtype)
    lf[0] = logp[0] + lnpi
    for t in range(1, n):
        m[t - 1] = _lse(lf[t - 1], fn, reverse)
        lf[t] = logp[t] + _logaddexp(lnP + lf[t - 1], c + m[t - 1], fn)
    m[n - 1] = _lse(lf[n - 1], fn, reverse)
    for t in range(n - 2, -1, -1):
        q = logp[t + 1] + lb[t + 1]
        r = ln1mP + _lse(lnpi + q, fn, reverse)
        lb[t] = _logaddexp(lnP + q, r, fn)
    tll = m[n - 1]
    gamma = fn.exp(lf + lb - tll)
    x = fn.exp(m[:-1, None] + logp[1:] + lb[1:] - tll) if n > 1 else np.zeros((0, S), dtype)
    acc = np.zeros(S, dtype)
    for t in (range(n - 2, -1, -1) if reverse else range(n - 1)):
        acc = acc + x[t]
    pinew = gamma[0] + ((dtype(1) - P) * pi) * acc
    return dict(lf=lf, lb=lb, m=m, tll=tll, gamma=gamma, pinew=pinew)


def vbx_hmm(X, Phi, init_labels, S, loop_prob, Fa=0.07, Fb=0.8, max_iters=20, epsilon=1e-4, init_smoothing=7.0, dtype=np.float64, reverse=False,
            jitter=None, fb=None):
    """-> dict(gamma [n, S], pi [S], elbo [n_iter], n_iter, lf, lb [n, S] of the last iteration), all in dtype.  The rows of X are in time
    order.  fb: another forward_backward (the dense one of the CPU tests)."""
    fn = _Fn(dtype, jitter)
    fb = fb or forward_backward
    X, Phi = np.asarray(X).astype(dtype), np.asarray(Phi).astype(dtype)
    n, D = X.shape
    Fa, Fb, eps = dtype(Fa), dtype(Fb), dtype(epsilon)
    half = dtype(1) / dtype(2)
    rows = range(n - 1, -1, -1) if reverse else range(n)
    rho = X * np.sqrt(Phi)[None, :]
    x2 = np.zeros(n, dtype)
    for d in range(D):
        x2 = x2 + X[:, d] * X[:, d]
    G = -half * (x2 + dtype(D) * dtype(LN_2PI))
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
    out = None
    for ii in range(max_iters):
        N = np.zeros(S, dtype)
        F = np.zeros((S, D), dtype)
        for t in rows:
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
            e2 = e2 + (fn.log(invL[:, d]) - invL[:, d] - alpha[:, d] * alpha[:, d] + dtype(1))
        logp = Fa * (dot - half * c[None, :] + G[:, None])
        out = fb(logp, pi, loop_prob, dtype, reverse, fn)
        gamma = out["gamma"]
        elbo.append(out["tll"] + half * Fb * _seq_sum(e2, reverse))
        pi = out["pinew"] / _seq_sum(out["pinew"], reverse)
        if ii > 0 and elbo[-1] - elbo[-2] < eps:
            break
    return dict(gamma=gamma, pi=pi, elbo=np.array(elbo, dtype), n_iter=len(elbo), lf=out["lf"], lb=out["lb"])


def speaker_runs(true, rng, mean_run=12):
    """A permutation that lays rows out as a conversation: runs of one speaker, of 1 .. 2 mean_run rows, the speakers taking turns at
    random until their rows are used up -> order [n] (indices into the rows).  So the chain matters: neighbours mostly share a speaker."""
    pools = {v: list(np.flatnonzero(true == v)) for v in np.unique(true)}
    order = []
    last = None
    while pools:
        live = [v for v in pools if v != last] or list(pools)
        v = live[int(rng.integers(len(live)))]
        k = int(rng.integers(1, 2 * mean_run + 1))
        order += pools[v][:k]
        pools[v] = pools[v][k:]
        if not pools[v]:
            del pools[v]
        last = v
    return np.array(order, np.int64)
