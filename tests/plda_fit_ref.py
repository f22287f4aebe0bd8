"""Test-side checker of the PLDA training's device half (plda.fit, csrc/plda_fit.hip): the statistics and the projection of the stated rule in
numpy loops and plain sums, written from the statement and sharing no code with the package; and a generator of labelled rows from a planted
two-covariance model.

Every sum over rows runs row by row, ascending or - reverse=True - descending, which is what a different summation order over the rows costs;
sums over dimensions ascending.  dtype is np.float64 or np.longdouble.
"""
from __future__ import annotations

import numpy as np


def _row_order(n, reverse):
    return range(n - 1, -1, -1) if reverse else range(n)


def _unit_rows(v, dtype):
    q = np.zeros(v.shape[0], dtype)
    for j in range(v.shape[1]):
        q = q + v[:, j] * v[:, j]
    return v / np.maximum(np.sqrt(q), dtype("1e-300"))[:, None]


def stage1_rows(E, mean1, dtype=np.float64):
    """x1 = sqrt(d_in) unit(e - mean1); mean1 None: the rows as they are."""
    E = np.asarray(E).astype(dtype)
    if mean1 is None:
        return E
    return np.sqrt(dtype(E.shape[1])) * _unit_rows(E - np.asarray(mean1).astype(dtype)[None, :], dtype)


def project(E, mean1, lda, mean2, dtype=np.float64):
    """x2 = sqrt(D0) unit(lda^T x1 - mean2) [N, D0]."""
    lda, mean2 = np.asarray(lda).astype(dtype), np.asarray(mean2).astype(dtype)
    d_in, D0 = lda.shape
    x1 = stage1_rows(E, mean1, dtype)
    y = np.zeros((x1.shape[0], D0), dtype)
    for i in range(d_in):
        y = y + x1[:, i, None] * lda[i][None, :]
    return np.sqrt(dtype(D0)) * _unit_rows(y - mean2[None, :], dtype)


def stats(X, labels, K, dtype=np.float64, reverse=False, scatter=True):
    """Rows X [N, d] (already transformed) -> dict(counts [K] int64, sums [K, d], total [d], scatter [d, d]) in dtype, row by row."""
    X = np.asarray(X).astype(dtype)
    N, d = X.shape
    counts = np.zeros(K, np.int64)
    sums = np.zeros((K, d), dtype)
    total = np.zeros(d, dtype)
    S = np.zeros((d, d), dtype)
    for i in _row_order(N, reverse):
        x = X[i]
        if labels is not None:
            counts[labels[i]] += 1
            sums[labels[i]] = sums[labels[i]] + x
        total = total + x
        if scatter:
            S = S + x[:, None] * x[None, :]
    return dict(counts=counts, sums=sums, total=total, scatter=S)


def second_column_weight(name, ref, cut, tolerance) -> float:
    """partial_width.weight of a case wider than 256 columns, quantity by quantity: ref and cut are {quantity: array} of this module's functions on
    the full input and on its first 256 columns alone (partial_width.first_columns), tolerance {quantity: the case's bound}.  -> the least ratio."""
    import partial_width as PW
    return min(PW.weight(f"{name} {q}", floats=[(np.asarray(ref[q], np.float64), np.asarray(cut[q], np.float64))], bound=tolerance[q]) for q in tolerance)


# ------------------------------------------------------------------------------------------------ planted two-covariance model
class Planted:
    """Speaker means y ~ N(0, diag(between)), rows y + N(0, diag(within)), rotated by a seeded orthogonal matrix, shifted, and put on the unit
    sphere (fp32).  between falls from 9 to 0.02 over the dimensions, within from 1.5 to 0.5."""

    def __init__(self, seed, d_in):
        rng = np.random.default_rng(seed)
        self.d_in = d_in
        self.between = np.geomspace(9.0, 0.02, d_in)
        self.within = np.geomspace(1.5, 0.5, d_in)
        self.Q = np.linalg.qr(rng.standard_normal((d_in, d_in)))[0]
        self.shift = 0.3 * rng.standard_normal(d_in)

    def speakers(self, rng, K):
        return rng.standard_normal((K, self.d_in)) * np.sqrt(self.between)[None, :]

    def rows(self, rng, means, labels):
        x = means[labels] + rng.standard_normal((len(labels), self.d_in)) * np.sqrt(self.within)[None, :]
        e = x @ self.Q.T + self.shift[None, :]
        return (e / np.linalg.norm(e, axis=1, keepdims=True)).astype(np.float32)


def labelled_rows(seed, N, d_in, K, unused=(), singles=(), scramble=True):
    """-> (E [N, d_in] fp32 unit rows, labels [N] int32 in [0, K), model).  The ids in `unused` get no row, those in `singles` exactly one, the
    others uneven sizes (at least one row each); scramble: the rows come in random order, else sorted by label."""
    rng = np.random.default_rng(seed)
    model = Planted(seed + 1, d_in)
    used = np.array([k for k in range(K) if k not in set(unused)])
    free = np.array([k for k in used if k not in set(singles)])
    rest = N - len(used)
    assert rest >= 0 and (rest == 0 or len(free))
    extra = rng.multinomial(rest, rng.dirichlet(np.full(len(free), 0.7))) if len(free) else np.zeros(0, np.int64)
    labels = np.concatenate([used, np.repeat(free, extra)]).astype(np.int32)
    labels = rng.permutation(labels) if scramble else np.sort(labels)
    means = model.speakers(rng, K)
    return model.rows(rng, means, labels), labels.astype(np.int32), model


# ------------------------------------------------------------------------------------------------ the labelling rule of Diarizer.plda_rows
POWERSET = [(), (0,), (1,), (2,), (0, 1), (0, 2), (1, 2)]          # the local speakers of the seven classes


def label_row(active, count, q, ref_masks):
    """One training row (a chunk's local speaker).  active [F] bool: the chunk frames where that speaker is active; count [F]: the speakers
    active per chunk frame; q: the chunk's offset, global frame g = i - q; ref_masks [R, G] bool: the reference speakers' activity per global
    frame.  -> the reference speaker of the largest tally (ties to the lower) when 2 * tally >= the frames tallied over, else -1."""
    R, G = ref_masks.shape
    tally = [0] * R
    n = 0
    for i in range(len(active)):
        g = i - q
        if not (active[i] and count[i] < 2) or g < 0 or g >= G:
            continue
        n += 1
        for r in range(R):
            if ref_masks[r, g]:
                tally[r] += 1
    best = -1
    for r in range(R):
        if best < 0 or tally[r] > tally[best]:
            best = r
    if best < 0 or n == 0 or 2 * tally[best] < n:
        return -1
    return best


def label_rows(cls, starts, train, ref_masks):
    """Every row (c * 3 + s) of one recording: label_row for the rows of `train` (bool per row), -1 for the others."""
    out = np.full(3 * len(cls), -1, np.int32)
    for c in range(len(cls)):
        count = [len(POWERSET[k]) for k in cls[c]]
        q = (135 - int(starts[c])) // 270
        for s in range(3):
            if train[3 * c + s]:
                out[3 * c + s] = label_row([s in POWERSET[k] for k in cls[c]], count, q, ref_masks)
    return out


def class_table(layout, starts, F=589, rate=16000):
    """cls [C, F] of the chunks at `starts` for speakers active as layout = [(speaker, from s, to s)] says, local speakers numbered by first
    appearance in the chunk (at most three per chunk, at most two per frame)."""
    cls = np.zeros((len(starts), F), np.uint8)
    for c in range(len(starts)):
        local = {}
        for i in range(F):
            t = (int(starts[c]) + 270 * i + 495) / rate
            on = sorted({v for v, a, b in layout if a <= t < b})
            for v in on:
                local.setdefault(v, len(local))
            cls[c, i] = POWERSET.index(tuple(sorted(local[v] for v in on)))
    return cls
