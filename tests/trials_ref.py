"""An independent brute-force reference for verification trials (the rule: the docstring of the package's trials.py).  It shares no code with
trials.py: from raw score arrays it forms the integer score q of every trial and evaluates the error counts at EVERY integer threshold at which
either can change - the distinct q that occur and each of them plus 1 (and 0 and 2^24) - so its EER and minDCF are exact on the q scale.

A score below the range is q = -1 (rejected by every threshold), one above it is q = 2^24 (accepted by every threshold 0 .. 2^24).
"""
from __future__ import annotations

import math

import numpy as np

QMAX = 1 << 24


def quantise(S, lo, hi):
    """-> (q int64 with -1 below and 2^24 above, nan mask).  t = (s - lo) * scale in two float64 roundings, scale = 2^24 / (hi - lo)."""
    S = np.asarray(S, dtype=np.float64)
    scale = np.float64(QMAX) / (np.float64(hi) - np.float64(lo))
    with np.errstate(invalid="ignore", over="ignore"):
        d = S - np.float64(lo)
        t = d * scale
    nan = np.isnan(t)
    q = np.full(S.shape, -1, np.int64)
    mid = ~nan & (t >= 0) & (t < QMAX)
    q[mid] = np.floor(t[mid]).astype(np.int64)
    q[~nan & (t >= QMAX)] = QMAX
    return q, nan


def classes(la, sa, lb, sb):
    """[N, M]: 1 target, 0 nontarget, -1 excluded - written as loops over the rule's sentences."""
    la, sa, lb, sb = (np.asarray(a, dtype=np.int64) for a in (la, sa, lb, sb))
    out = np.empty((len(la), len(lb)), np.int64)
    for i in range(len(la)):
        same_session = (sb == sa[i]) if sa[i] >= 0 else np.zeros(len(lb), bool)
        row = np.where(lb == la[i], 1, 0)
        row[(lb < 0) | same_session] = -1
        if la[i] < 0:
            row[:] = -1
        out[i] = row
    return out


def dcf_value(miss, fa, T, Nn, p, cm, cf):
    return (cm * p * (miss / T) + cf * (1 - p) * (fa / Nn)) / min(cm * p, cf * (1 - p))


def metrics(S, cls, lo, hi, p=0.01, cm=1.0, cf=1.0):
    """Brute force over every integer threshold that matters -> dict; eer is None when the curves do not cross at any t <= 2^24."""
    S, cls = np.asarray(S, dtype=np.float64).ravel(), np.asarray(cls).ravel()
    q, nan = quantise(S, lo, hi)
    scale = float(np.float64(QMAX) / (np.float64(hi) - np.float64(lo)))
    live = (cls >= 0) & ~nan
    tq, nq = np.sort(q[live & (cls == 1)]), np.sort(q[live & (cls == 0)])
    T, Nn = len(tq), len(nq)
    out = {"T": T, "Nn": Nn, "n_nan": int(((cls >= 0) & nan).sum()), "n_excluded": int((cls < 0).sum())}
    if T == 0 or Nn == 0:
        return out
    assert T * Nn < 2 ** 62
    seen = np.unique(np.concatenate([tq, nq]))
    ts = np.unique(np.concatenate([[0, QMAX], seen, seen + 1]))
    ts = ts[(ts >= 0) & (ts <= QMAX)]
    miss = np.searchsorted(tq, ts, side="left")                      # targets with q < t
    fa = Nn - np.searchsorted(nq, ts, side="left")                   # nontargets with q >= t
    ok = np.flatnonzero(miss * Nn >= fa * T)
    if len(ok) == 0:
        out["eer"] = None
    else:
        t = int(ts[ok[0]])
        out["t_star"] = t
        out["eer_threshold"] = lo + t / scale
        if t == 0:
            out["eer"] = (int(miss[ok[0]]) / T + int(fa[ok[0]]) / Nn) / 2
        else:
            m0, f0 = int(np.searchsorted(tq, t - 1, side="left")), Nn - int(np.searchsorted(nq, t - 1, side="left"))
            m1, f1 = int(miss[ok[0]]), int(fa[ok[0]])
            pm0, pf0, pm1, pf1 = m0 / T, f0 / Nn, m1 / T, f1 / Nn
            d0, d1 = pf0 - pm0, pm1 - pf1
            out["eer"] = pm0 + d0 / (d0 + d1) * (pm1 - pm0)
    vals = [dcf_value(int(m), int(f), T, Nn, p, cm, cf) for m, f in zip(miss.tolist(), fa.tolist())]
    vals += [dcf_value(0, Nn, T, Nn, p, cm, cf), dcf_value(T, 0, T, Nn, p, cm, cf)]          # accept all, reject all
    out["min_dcf"] = min(vals)
    assert math.isfinite(out["min_dcf"])
    return out
