"""An independent restatement of the calibration rule of trials.py in np.longdouble, for the tests: plain loops over the trials for the sums,
a textbook O(n^2) pool-adjacent-violators.  It shares no code with trials.py.

z = a * s + c is formed in float64 with its two roundings, as the rule states it (so the reference and the code under test start from the
same z, bit for bit); everything after it is extended precision.  v = w (1 - w) is evaluated as e / (1 + e)^2, which is the same number
without the cancellation of 1 - w."""
from __future__ import annotations

import math

import numpy as np

LD = np.longdouble
NAMES = ("L", "W0", "W1", "H0", "H1", "H2", "S1")


def classes(la, sa, lb, sb):
    """[N, M]: 1 target, 0 nontarget, -1 excluded."""
    out = np.zeros((len(la), len(lb)), np.int64)
    for i in range(len(la)):
        for j in range(len(lb)):
            if la[i] < 0 or lb[j] < 0 or (sa[i] >= 0 and sa[i] == sb[j]):
                out[i, j] = -1
            else:
                out[i, j] = 1 if la[i] == lb[j] else 0
    return out


def scores(A, B, r):
    """The product in extended precision, rounded once to float64."""
    with np.errstate(invalid="ignore", over="ignore"):
        return (A.astype(LD) @ B.T.astype(LD) + r.astype(LD)[None, :]).astype(np.float64)


def terms(s, y, a, c):
    """The seven terms of finite float64 scores s [n] with y = +1 / -1 -> [7, n] longdouble."""
    s = np.asarray(s, np.float64)
    with np.errstate(over="ignore"):
        z = (np.float64(a) * s) + np.float64(c)          # float64: one rounded product, one rounded sum
    m = z.astype(LD) * np.asarray(y, LD)
    e = np.exp(-np.abs(m))
    loss = np.where(m < 0, -m, LD(0)) + np.log1p(e)
    w = np.where(m >= 0, e / (1 + e), 1 / (1 + e))
    v = e / ((1 + e) * (1 + e))
    sl = s.astype(LD)
    return np.stack([loss, w, w * sl, v, v * sl, v * sl * sl, sl])


def sums(S, cls, a, c):
    """One pass -> dict(n [2], sums [2][7] longdouble, mag [2][7] = the sums of |term|, nonfinite [2], excluded)."""
    S, cls = np.asarray(S, np.float64).ravel(), np.asarray(cls).ravel()
    n, nonfinite, excluded = [0, 0], [0, 0], 0
    tot = [[LD(0)] * 7, [LD(0)] * 7]
    mag = [[LD(0)] * 7, [LD(0)] * 7]
    t1, t0 = terms(np.where(np.isfinite(S), S, 0.0), 1.0, a, c), terms(np.where(np.isfinite(S), S, 0.0), -1.0, a, c)
    for i in range(len(S)):
        k = int(cls[i])
        if k < 0:
            excluded += 1
            continue
        if not math.isfinite(S[i]):
            nonfinite[k] += 1
            continue
        n[k] += 1
        t = t1 if k else t0
        for q in range(7):
            x = t[q, i]
            tot[k][q] = tot[k][q] + x
            mag[k][q] = mag[k][q] + abs(x)
    return dict(n=n, sums=np.asarray(tot, LD), mag=np.asarray(mag, LD), nonfinite=nonfinite, excluded=excluded)


def objective(res, prior):
    """J, gradient and Hessian in (a, b) from a pass at c = b + theta."""
    n0, n1 = res["n"]
    u0, u1 = LD(1 - prior) / n0, LD(prior) / n1
    x0, x1 = res["sums"]
    J = u1 * x1[0] + u0 * x0[0]
    g = np.asarray([u0 * x0[2] - u1 * x1[2], u0 * x0[1] - u1 * x1[1]], LD)
    H = np.asarray([[u0 * x0[5] + u1 * x1[5], u0 * x0[4] + u1 * x1[4]], [u0 * x0[4] + u1 * x1[4], u0 * x0[3] + u1 * x1[3]]], LD)
    return J, g, H


def cllr(res):
    n0, n1 = res["n"]
    return (res["sums"][1][0] / n1 + res["sums"][0][0] / n0) / (2 * np.log(LD(2)))


def pav_min_cllr(t, n):
    """Cells in score order with t targets and n nontargets each -> the minimum Cllr of the quantised score.  The textbook algorithm: start
    with one block per non-empty cell; while some adjacent pair violates the order of the target fractions, pool the first such pair."""
    blocks = [[int(a), int(b)] for a, b in zip(t, n) if a + b > 0]
    while True:
        for i in range(len(blocks) - 1):
            (a0, b0), (a1, b1) = blocks[i], blocks[i + 1]
            if a0 * (a1 + b1) > a1 * (a0 + b0):                     # fraction of block i above that of block i + 1
                blocks[i:i + 2] = [[a0 + a1, b0 + b1]]
                break
        else:
            break
    T, N = sum(b[0] for b in blocks), sum(b[1] for b in blocks)
    ct = cn = LD(0)
    for a, b in blocks:
        if a:
            ct += a * np.log1p(LD(b) * T / (LD(a) * N))
        if b:
            cn += b * np.log1p(LD(a) * N / (LD(b) * T))
    return (ct / T + cn / N) / (2 * np.log(LD(2)))


def quantise(S, lo, hi):
    """q of every score (float64 arithmetic of the rule) -> (q int64 with -1 below and 2^24 above, nan mask)."""
    scale = np.float64(2 ** 24) / (np.float64(hi) - np.float64(lo))
    with np.errstate(invalid="ignore", over="ignore"):
        t = (np.asarray(S, np.float64) - np.float64(lo)) * scale
    nan = np.isnan(t)
    q = np.where(nan, 0, np.where(t < 0, -1, np.where(t >= 2.0 ** 24, 2 ** 24, np.floor(np.where(np.isfinite(t), t, 0))))).astype(np.int64)
    return q, nan


def dcf_at(S, cls, lo, hi, tq, p, cm, cf):
    """The normalised DCF of accepting q >= tq, by counting."""
    q, nan = quantise(S, lo, hi)
    cls = np.asarray(cls)
    T = Nn = miss = fa = 0
    for qi, k, bad in zip(q.ravel().tolist(), cls.ravel().tolist(), nan.ravel().tolist()):
        if k < 0 or bad:
            continue
        if k == 1:
            T += 1
            miss += qi < tq
        else:
            Nn += 1
            fa += qi >= tq
    return (cm * p * (miss / T) + cf * (1 - p) * (fa / Nn)) / min(cm * p, cf * (1 - p))
